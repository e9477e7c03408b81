/* Bit-for-bit check of small_taps.h (the one-launch small path's tap order and window slots) on
 * the host, over smallgeom.cpp's sweep: for every tile, every level k and every output m of the
 * tile's window, the kernel's walks -- the general one (sm_ana_at / sm_ana_tap, sm_syn_at /
 * sm_syn_tap) and, where it applies, the fast one (sm_ana_fast / sm_syn_fast with sm_order) --
 * read a window buffer laid out as the kernel's (slot s holds real index sm_wrap(W.s + s, N)) and
 * must give exactly the bits of wt_ana_point / wt_syn_pass over the full line.  The data spreads
 * over ~40 binades with mixed signs, so a changed summation order changes bits.  Every slot must
 * lie inside its window.  sm_divmod is compared with / and %.  Exit status 0 = pass.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../wavelettransforms_amd/csrc/wt_dwt_core.h"
#include "../../wavelettransforms_amd/csrc/small_taps.h"

static const int SM_ARENA_WORDS = 34 * 1024; /* wtp_internal.h's SM_ARENA: the kernel divides no larger e */

static uint32_t rng_state = 0x9E3779B9u;
static uint32_t rng() { /* xorshift32, fixed seed */
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}
static float rnd_float() { /* +-[1, 2) * 2^e, e in [-20, 20] */
    const uint32_t r = rng();
    const float m = 1.0f + (float)(r & 0x7FFFFFu) / 8388608.0f;
    const float v = std::ldexp(m, (int)((r >> 23) % 41u) - 20);
    return (r >> 31) ? -v : v;
}
static void fill(std::vector<float>& v, int n) {
    v.resize(n);
    for (float& x : v) x = rnd_float();
}
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
/* the kernel's window of a line: slot s holds real index sm_wrap(W.s + s, N) */
static void window(const std::vector<float>& line, SmIvl W, int N, std::vector<float>& w) {
    w.resize(W.len);
    for (int s = 0; s < W.len; ++s) w[s] = line[sm_wrap(W.s + s, N)];
}

static bool specialised(int F) {
#define IS_FT(ft) if (F == ft) return true;
    SM_SPECIALISED(IS_FT)
#undef IS_FT
    return false;
}
/* sm_order<F> (analysis) and sm_order<F / 2> (synthesis) for a run-time specialised F, with
 * plain = (c1 == 0) */
template <class V, class C, class A>
static void order_full(int F, int c1, const V& v, const C& c, const A& acc) {
    switch (F) {
#define ORDER_CASE(ft) case ft: sm_order<ft>(c1, c1 == 0, v, c, acc); break;
        SM_SPECIALISED(ORDER_CASE)
#undef ORDER_CASE
    }
}
template <class V, class C, class A>
static void order_half(int F, int c1, const V& v, const C& c, const A& acc) {
    switch (F) {
#define ORDER_CASE(ft) case ft: sm_order<ft / 2>(c1, c1 == 0, v, c, acc); break;
        SM_SPECIALISED(ORDER_CASE)
#undef ORDER_CASE
    }
}

static int check_axis(int N0, int L, int F, int T) {
    int32_t N[SM_MAX_L + 1];
    N[0] = N0;
    for (int k = 1; k <= L; ++k) N[k] = (N[k - 1] + 1) / 2;
    const int tiles = (N[L] + T - 1) / T, H = F / 2;
    const bool fast = specialised(F);
    std::vector<float> taps[4]; /* dec_lo, dec_hi, rec_lo, rec_hi */
    for (auto& t : taps) fill(t, F);
    /* X[k]: the level-k line the analysis of level k + 1 reads; A[k], D[k]: the level-k lines the
     * synthesis of level k - 1 reads */
    std::vector<float> X[SM_MAX_L + 1], A[SM_MAX_L + 1], D[SM_MAX_L + 1], wx, wa, wd;
    for (int k = 0; k <= L; ++k) { fill(X[k], N[k]); fill(A[k], N[k]); fill(D[k], N[k]); }
    int bad = 0;
    for (int t = 0; t < tiles; ++t) {
        SmAxis ax;
        sm_axis(t, T, L, N, F, &ax);
        for (int k = 1; k <= L; ++k) {
            /* ---- analysis: window fw[k] of line N[k] reads window fw[k-1] of line N[k-1] ---- */
            const SmIvl W = ax.fw[k], Wp = ax.fw[k - 1];
            const int Np = N[k - 1];
            window(X[k - 1], Wp, Np, wx);
            for (int m = 0; m < W.len; ++m) {
                float ra, rd;
                wt_ana_point(sm_wrap(W.s + m, N[k]), Np, F, taps[0].data(), taps[1].data(),
                             [&](int64_t i) { return X[k - 1][i]; }, ra, rd);
                const SmAna an = sm_ana_at(W, N[k], Np, F, m);
                float a = 0.0f, d = 0.0f;
                for (int q = 0; q < F; ++q) {
                    int j;
                    const int sl = sm_ana_tap(an, Wp, Np, q, &j);
                    if (sl < 0 || sl >= Wp.len) { ++bad; continue; }
                    a = a + taps[0][j] * wx[sl];
                    d = d + taps[1][j] * wx[sl];
                }
                if (!same(a, ra) || !same(d, rd)) ++bad;
                const int fb = sm_ana_fast(W, N[k], Wp, Np, F, m);
                if (fast && fb >= 0) {
                    const int s0 = fb >> 5, c1 = fb & 31;
                    if (s0 - F + 1 < 0 || s0 >= Wp.len) { ++bad; continue; }
                    float fa = 0.0f, fd = 0.0f;
                    order_full(F, c1, [&](int j) { return wx[s0 - j]; }, [&](int j) { return j; },
                              [&](int j, float x) { fa = fa + taps[0][j] * x; fd = fd + taps[1][j] * x; });
                    if (!same(fa, ra) || !same(fd, rd)) ++bad;
                }
            }
            /* ---- synthesis: window sv[k-1] of line N[k-1] reads window sv[k] of line N[k] ---- */
            const SmIvl O = ax.sv[k - 1], S = ax.sv[k];
            const int No = N[k - 1], Ns = N[k];
            window(A[k], S, Ns, wa);
            window(D[k], S, Ns, wd);
            for (int m = 0; m < O.len; ++m) {
                const wt_syn_site site = wt_syn_locate(sm_wrap(O.s + m, No), Ns, F);
                float ry = wt_syn_pass(site, Ns, F, taps[2].data(), [&](int64_t i) { return A[k][i]; }, 0.0f);
                ry = wt_syn_pass(site, Ns, F, taps[3].data(), [&](int64_t i) { return D[k][i]; }, ry);
                const SmSyn sy = sm_syn_at(O, No, Ns, F, m);
                float y = 0.0f;
                bool in = true;
                for (int q = 0; q < H; ++q) {
                    int ci;
                    const int sl = sm_syn_tap(sy, S, Ns, q, &ci);
                    if (sl < 0 || sl >= S.len) { in = false; continue; }
                    y = y + taps[2][ci] * wa[sl];
                }
                for (int q = 0; q < H; ++q) {
                    int ci;
                    const int sl = sm_syn_tap(sy, S, Ns, q, &ci);
                    if (sl < 0 || sl >= S.len) { in = false; continue; }
                    y = y + taps[3][ci] * wd[sl];
                }
                if (!in || !same(y, ry)) ++bad;
                const int fb = sm_syn_fast(O, No, S, Ns, F, m);
                if (fast && fb >= 0) {
                    const int s0 = fb >> 6, par = (fb >> 5) & 1, c1 = fb & 31;
                    if (s0 - H + 1 < 0 || s0 >= S.len) { ++bad; continue; }
                    float fy = 0.0f;
                    order_half(F, c1, [&](int j) { return wa[s0 - j]; }, [&](int j) { return taps[2][2 * j + par]; },
                              [&](float cf, float x) { fy = fy + cf * x; });
                    order_half(F, c1, [&](int j) { return wd[s0 - j]; }, [&](int j) { return taps[3][2 * j + par]; },
                              [&](float cf, float x) { fy = fy + cf * x; });
                    if (!same(fy, ry)) ++bad;
                }
            }
        }
    }
    if (bad) std::printf("FAIL N0=%d L=%d F=%d T=%d: %d\n", N0, L, F, T, bad);
    return bad;
}

/* sm_divmod against / and %: every n up to 2048, then every DIVMOD_STRIDE-th n up to
 * wtp_internal.h's SM_LINE_MAX (a window's line is no longer), each with every e below the arena */
static const int DIVMOD_STRIDE = 61;
static int check_divmod() {
    int bad = 0;
    for (int n = 1; n <= 32767; n += (n < 2048 ? 1 : DIVMOD_STRIDE)) {
        const float inv = 1.0f / (float)n;
        for (int e = 0; e < SM_ARENA_WORDS; ++e) {
            int q, r;
            sm_divmod(e, n, inv, &q, &r);
            bad += q != e / n || r != e % n;
        }
    }
    if (bad) std::printf("FAIL sm_divmod: %d\n", bad);
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    const int Fs[] = {2, 4, 6, 8, 10, 12, 16, 18, 20};
    for (int N0 = 1; N0 <= 140; N0 += (N0 < 40 ? 1 : 7))
        for (int F : Fs)
            for (int L = 1; L <= 6; ++L) {
                int n = N0;
                for (int k = 0; k < L; ++k) n = (n + 1) / 2;
                for (int T = 1; T <= n; T = T < 4 ? T + 1 : 2 * T) {
                    bad += check_axis(N0, L, F, T) != 0;
                    ++cases;
                }
            }
    bad += check_axis(784, 3, 6, 4) != 0;
    bad += check_axis(784, 3, 6, 2) != 0;
    bad += check_axis(128, 3, 6, 16) != 0;
    bad += check_divmod() != 0;
    std::printf("%d cases, %d failing\n", cases + 4, bad);
    return bad ? 1 : 0;
}

// Host build of the extension modes' shared core (csrc/wt_modes_core.h: one level of analysis and
// synthesis of a line, the packed geometry) as a stand-alone program, so the CPU suite can check
// its arithmetic against PyWavelets goldens without a GPU, and run it once under
// -fsanitize=address,undefined.  Built by tests/test_modes_core.py with
//   g++ -O2 -std=c++17 -ffp-contract=off
// Usage: modescore IN OUT.  IN is a stream of int32 / float32 words, one record after another:
//   1 mode F N | taps[4F] | x[N]                  -> M | a[M] d[M] | K | y[K]   (dwt, idwt)
//   2 mode F H W L                                 -> R[0..L] C[0..L] PR PC outH outW
//   3 mode F B H W L thr | taps[4F] | x[B H W]     -> PR PC | packed[B PR PC] | out[B H W]
//   4 H W L F                                      -> wtm_tiny_lanes_log2 (-1: not a tiny tensor)
//   5 mode F B H W L NL thr | taps[4F] | x[B H W]  -> as record 3
//   6 mode F H W L                                 -> wtm_levels_ok | R[0..L] C[0..L] offR[1..L] offC[1..L] PR PC
//                                                     of wtm_tiny_geometry | the same of wtm_geom
// Record 3 is wavedec2 + coeffs_to_array, np.where(|c| < thr, 0, c), waverec2 and the crop to
// H x W, level by level as the per-level kernels of csrc/modes.hip run them.  Record 5 is the same
// transform of a tiny tensor as k_mtiny_fwd / k_mtiny_inv run it: wtm_tiny_fwd / wtm_tiny_inv on
// images in groups of NL at lane offsets of one arena of exactly the words the area functions
// report (so a word outside them is a heap overflow under AddressSanitizer), sentinels in it
// before each kernel's part, D zero-filled before the forward and thresholded on load.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../wavelettransforms_amd/csrc/wt_modes_core.h"

static std::vector<uint32_t> g_in;
static size_t g_pos = 0;
static FILE* g_out = nullptr;

static bool have(size_t n) { return g_pos + n <= g_in.size(); }
static int32_t rd_i() { return (int32_t)g_in[g_pos++]; }
static float rd_f() {
    float v;
    memcpy(&v, &g_in[g_pos++], 4);
    return v;
}
static std::vector<float> rd_fv(size_t n) {
    std::vector<float> v(n);
    if (n) memcpy(v.data(), &g_in[g_pos], 4 * n);
    g_pos += n;
    return v;
}
static void wr_i(int32_t v) { fwrite(&v, 4, 1, g_out); }
static void wr_fv(const std::vector<float>& v) {
    if (!v.empty()) fwrite(v.data(), 4, v.size(), g_out);
}

static bool rec_line() {
    if (!have(3)) return false;
    const int mode = rd_i(), F = rd_i(), N = rd_i();
    if (!wtm_line_ok(N, F, mode) || !have((size_t)4 * F + N)) return false;
    const std::vector<float> taps = rd_fv((size_t)4 * F), x = rd_fv((size_t)N);
    const int64_t M = wtm_dec_len(N, F), K = wtm_rec_len(M, F);
    std::vector<float> a(M), d(M), y(K);
    for (int64_t o = 0; o < M; ++o)
        wtm_ana_point(o, N, F, &taps[0], &taps[F], mode, [&](int64_t k) { return x.at((size_t)k); }, a[o], d[o]);
    for (int64_t n = 0; n < K; ++n)
        y[n] = wtm_syn_point(n, F, &taps[2 * F], &taps[3 * F], [&](int64_t k) { return a.at((size_t)k); },
                             [&](int64_t k) { return d.at((size_t)k); });
    wr_i((int32_t)M);
    wr_fv(a);
    wr_fv(d);
    wr_i((int32_t)K);
    wr_fv(y);
    return true;
}

static bool rec_geom() {
    if (!have(5)) return false;
    const int mode = rd_i(), F = rd_i(), H = rd_i(), W = rd_i(), L = rd_i();
    if (L < 0 || L > 32) return false;
    wt_level_geom g;
    wtm_geom(H, W, L, F, mode, &g);
    for (int k = 0; k <= L; ++k) wr_i((int32_t)g.R[k]);
    for (int k = 0; k <= L; ++k) wr_i((int32_t)g.C[k]);
    wr_i((int32_t)g.PR);
    wr_i((int32_t)g.PC);
    wr_i((int32_t)(L ? wtm_out_len(g.R[1], F, mode) : H));
    wr_i((int32_t)(L ? wtm_out_len(g.C[1], F, mode) : W));
    return true;
}

static bool rec_image() {
    if (!have(7)) return false;
    const int mode = rd_i(), F = rd_i(), B = rd_i(), H = rd_i(), W = rd_i(), L = rd_i();
    const float thr = rd_f();
    if (L < 1 || L > 32 || B < 1 || !wtm_line_ok(H, F, mode) || !wtm_line_ok(W, F, mode)) return false;
    if (!have((size_t)4 * F + (size_t)B * H * W)) return false;
    const std::vector<float> taps = rd_fv((size_t)4 * F), x = rd_fv((size_t)B * H * W);
    wt_level_geom g;
    wtm_geom(H, W, L, F, mode, &g);
    const int64_t PR = g.PR, PC = g.PC;
    std::vector<float> P((size_t)(B * PR * PC), 0.0f), out((size_t)B * H * W);
    for (int b = 0; b < B; ++b) {
        float* Pb = &P[(size_t)(b * PR * PC)];
        std::vector<float> cur(x.begin() + (size_t)b * H * W, x.begin() + (size_t)(b + 1) * H * W);
        for (int k = 1; k <= L; ++k) {
            const int64_t R0 = g.R[k - 1], C0 = g.C[k - 1], R = g.R[k], C = g.C[k];
            std::vector<float> lo((size_t)(R * C0)), hi((size_t)(R * C0)), nxt((size_t)(R * C));
            for (int64_t o = 0; o < R; ++o)
                for (int64_t c = 0; c < C0; ++c)
                    wtm_ana_point(o, R0, F, &taps[0], &taps[F], mode, [&](int64_t q) { return cur.at((size_t)(q * C0 + c)); },
                                  lo[(size_t)(o * C0 + c)], hi[(size_t)(o * C0 + c)]);
            for (int64_t r = 0; r < R; ++r)
                for (int64_t o = 0; o < C; ++o) {
                    float aa, ad, da, dd;
                    wtm_ana_point(o, C0, F, &taps[0], &taps[F], mode, [&](int64_t q) { return lo.at((size_t)(r * C0 + q)); }, aa, ad);
                    wtm_ana_point(o, C0, F, &taps[0], &taps[F], mode, [&](int64_t q) { return hi.at((size_t)(r * C0 + q)); }, da, dd);
                    if (k == L) Pb[r * PC + o] = aa;
                    nxt[(size_t)(r * C + o)] = aa;
                    Pb[r * PC + g.offC[k] + o] = ad;
                    Pb[(g.offR[k] + r) * PC + o] = da;
                    Pb[(g.offR[k] + r) * PC + g.offC[k] + o] = dd;
                }
            cur.swap(nxt);
        }
        std::vector<float> a; /* the level above's output, R[k] x C[k] */
        for (int k = L; k >= 1; --k) {
            const int64_t R = g.R[k], C = g.C[k], oH = g.R[k - 1], oW = g.C[k - 1];
            std::vector<float> lo((size_t)(R * oW)), hi((size_t)(R * oW)), y((size_t)(oH * oW));
            for (int64_t r = 0; r < R; ++r)
                for (int64_t n = 0; n < oW; ++n) {
                    lo[(size_t)(r * oW + n)] = wtm_syn_point(
                        n, F, &taps[2 * F], &taps[3 * F],
                        [&](int64_t q) { return k == L ? wt_thr_mask(Pb[r * PC + q], thr) : a.at((size_t)(r * C + q)); },
                        [&](int64_t q) { return wt_thr_mask(Pb[r * PC + g.offC[k] + q], thr); });
                    hi[(size_t)(r * oW + n)] = wtm_syn_point(
                        n, F, &taps[2 * F], &taps[3 * F], [&](int64_t q) { return wt_thr_mask(Pb[(g.offR[k] + r) * PC + q], thr); },
                        [&](int64_t q) { return wt_thr_mask(Pb[(g.offR[k] + r) * PC + g.offC[k] + q], thr); });
                }
            for (int64_t m = 0; m < oH; ++m)
                for (int64_t n = 0; n < oW; ++n)
                    y[(size_t)(m * oW + n)] =
                        wtm_syn_point(m, F, &taps[2 * F], &taps[3 * F], [&](int64_t q) { return lo.at((size_t)(q * oW + n)); },
                                      [&](int64_t q) { return hi.at((size_t)(q * oW + n)); });
            a.swap(y);
        }
        memcpy(&out[(size_t)b * H * W], a.data(), sizeof(float) * (size_t)H * W);
    }
    wr_i((int32_t)PR);
    wr_i((int32_t)PC);
    wr_fv(P);
    wr_fv(out);
    return true;
}

static bool rec_tiny() {
    if (!have(8)) return false;
    const int mode = rd_i(), F = rd_i(), B = rd_i(), H = rd_i(), W = rd_i(), L = rd_i(), NL = rd_i();
    const float thr = rd_f();
    if (B < 1 || NL < 1 || NL > 64 || wtm_tiny_lanes_log2(H, W, L, F) < 0 || !wtm_levels_ok(H, W, L, F, mode)) return false;
    if (!have((size_t)4 * F + (size_t)B * H * W)) return false;
    const std::vector<float> taps = rd_fv((size_t)4 * F), x = rd_fv((size_t)B * H * W);
    wtm_tiny_geom g;
    wtm_tiny_geometry(H, W, L, F, g);
    const int HW = H * W, PP = g.PR * g.PC;
    const int aw = wtm_tiny_area_a(H, W, L, F), tw = wtm_tiny_area_t(H, W, L, F), dw = wtm_tiny_area_d(H, W, L, F);
    if (dw != PP) return false;
    std::vector<float> arena((size_t)(aw + tw + dw) * NL), P((size_t)B * PP), out((size_t)B * HW);
    float *A = arena.data(), *T = A + (size_t)aw * NL, *D = T + (size_t)tw * NL;
    for (int b0 = 0; b0 < B; b0 += NL) {
        const int n = B - b0 < NL ? B - b0 : NL;
        /* k_mtiny_fwd */
        std::fill(arena.begin(), arena.end(), -77.0f);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < HW; ++s) A[(size_t)s * NL + i] = x[(size_t)(b0 + i) * HW + s];
        for (int i = 0; i < NL; ++i)
            for (int s = 0; s < PP; ++s) D[(size_t)s * NL + i] = 0.0f;
        for (int i = 0; i < n; ++i) wtm_tiny_fwd(A + i, T + i, D + i, NL, g, L, F, mode, &taps[0], &taps[F]);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < PP; ++s) P[(size_t)(b0 + i) * PP + s] = D[(size_t)s * NL + i];
        /* k_mtiny_inv */
        std::fill(arena.begin(), arena.end(), -77.0f);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < PP; ++s) D[(size_t)s * NL + i] = wt_thr_mask(P[(size_t)(b0 + i) * PP + s], thr);
        for (int i = 0; i < n; ++i) wtm_tiny_inv(A + i, T + i, D + i, NL, g, L, F, &taps[2 * F], &taps[3 * F]);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < HW; ++s) out[(size_t)(b0 + i) * HW + s] = A[(size_t)s * NL + i];
    }
    wr_i(g.PR);
    wr_i(g.PC);
    wr_fv(P);
    wr_fv(out);
    return true;
}

static bool rec_tiny_geom() {
    if (!have(5)) return false;
    const int mode = rd_i(), F = rd_i(), H = rd_i(), W = rd_i(), L = rd_i();
    if (L < 1 || L > WTM_TINY_LMAX || mode == WTM_PERIODIZATION) return false;
    wtm_tiny_geom t;
    wtm_tiny_geometry(H, W, L, F, t);
    wt_level_geom g;
    wtm_geom(H, W, L, F, mode, &g);
    wr_i(wtm_levels_ok(H, W, L, F, mode));
    for (int k = 0; k <= L; ++k) wr_i(t.R[k]);
    for (int k = 0; k <= L; ++k) wr_i(t.C[k]);
    for (int k = 1; k <= L; ++k) wr_i(t.offR[k]);
    for (int k = 1; k <= L; ++k) wr_i(t.offC[k]);
    wr_i(t.PR);
    wr_i(t.PC);
    for (int k = 0; k <= L; ++k) wr_i((int32_t)g.R[k]);
    for (int k = 0; k <= L; ++k) wr_i((int32_t)g.C[k]);
    for (int k = 1; k <= L; ++k) wr_i((int32_t)g.offR[k]);
    for (int k = 1; k <= L; ++k) wr_i((int32_t)g.offC[k]);
    wr_i((int32_t)g.PR);
    wr_i((int32_t)g.PC);
    return true;
}

static bool rec_lanes() {
    if (!have(4)) return false;
    const int H = rd_i(), W = rd_i(), L = rd_i(), F = rd_i();
    wr_i((int32_t)wtm_tiny_lanes_log2(H, W, L, F));
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    fseek(fi, 0, SEEK_END);
    const long bytes = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    g_in.resize((size_t)bytes / 4);
    const size_t got = g_in.empty() ? 0 : fread(g_in.data(), 4, g_in.size(), fi);
    fclose(fi);
    if (got != g_in.size()) return 2;
    g_out = fopen(argv[2], "wb");
    if (!g_out) return 2;
    int n = 0;
    while (g_pos < g_in.size()) {
        const int kind = rd_i();
        const bool ok = kind == 1   ? rec_line()
                        : kind == 2 ? rec_geom()
                        : kind == 3 ? rec_image()
                        : kind == 4 ? rec_lanes()
                        : kind == 5 ? rec_tiny()
                        : kind == 6 ? rec_tiny_geom()
                                    : false;
        if (!ok) {
            fprintf(stderr, "modescore: bad record %d (kind %d)\n", n, kind);
            fclose(g_out);
            return 1;
        }
        ++n;
    }
    fclose(g_out);
    printf("modescore ok: %d records\n", n);
    return 0;
}

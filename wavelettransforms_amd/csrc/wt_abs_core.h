/* One tiny image (at most 8 x 8) through the absolute-threshold method, entirely in a small
 * arena: all levels forward, the mask, all levels inverse, the crop
 * (ResNet/dwt_pruning_NoEntropy.py:41-52).  Shared by k_abs_tiny (abs.hip: the arena is LDS, one
 * image per lane, word s of an image at arena[s * NL + lane]; wt_tiny_arena.h) and the host-side
 * check (tests/native/abscore.cpp: NL = 1 and 4).
 *
 * The levels are unclamped, so lines are shorter than the filter (a 3 x 3 kernel under an 8-tap
 * filter at level 5 ends in four 1 -> 1 levels) and every tap wraps, often more than once.  Every
 * tap is still multiplied and added on its own, in wt_dwt_core.h's order: abs_ana / abs_syn
 * restate wt_ana_point / wt_syn_point in 32-bit integers with a division-free, branch-free wrap
 * and the tap order split into its two runs (the lengths are wave-uniform on the device, so this
 * index arithmetic is scalar); abs_ana2 / abs_syn2 run two lines through one index sequence.
 * Folding the wrapped taps of a short line into fewer taps would change the rounding.  Build
 * with -ffp-contract=off.
 */
#ifndef WT_ABS_CORE_H
#define WT_ABS_CORE_H

#include "wt_tiny_arena.h"

/* t mod m for m in {1, 2, 3, 4, 6, 8} and |t| <= 128 (F <= 102 taps, lines of at most 8 samples),
 * inv = abs_inv(m): a multiply and a shift, no division and no branch */
WT_CORE int abs_inv(int m) { /* 65536 / m + 1 */
    return m == 3 ? 21846 : (m == 6 ? 10923 : (65536 >> __builtin_ctz((unsigned)m)) + 1);
}
WT_CORE int abs_mod(int t, int m, int inv) {
    t += 192; /* a multiple of every m, so t >= 0 */
    return t - m * ((t * inv) >> 16);
}

/* The tap order of wt_ana_point / wt_syn_pass without a test per tap: the taps that reach past
 * the line's end (j < n1) in descending order, then the others in ascending order.  n1 = 0
 * when the site lies inside the line: all taps ascending. */
template <class Body>
WT_CORE void abs_taps(int n1, int T, const Body& body) {
    n1 = n1 < 0 ? 0 : (n1 > T ? T : n1);
    for (int j = n1 - 1; j >= 0; --j) body(j);
#pragma unroll 4
    for (int j = n1; j < T; ++j) body(j);
}

/* wt_ana_point for two lines at once (the same sample indices, four sums, each in its own order) */
template <class Fetch1, class Fetch2>
WT_CORE void abs_ana2(int o, int N, int F, const float* lo, const float* hi, const Fetch1& f1, const Fetch2& f2,
                      float& sa1, float& sd1, float& sa2, float& sd2) {
    const int i = F / 2 + 2 * o, Ne = N + (N & 1), inv = abs_inv(Ne);
    float a1 = 0.0f, d1 = 0.0f, a2 = 0.0f, d2 = 0.0f;
    abs_taps(i - N + 1, F, [&](int j) {
        /* wt_ext_index: the line extended to even length repeats its last sample */
        int q = abs_mod(i - j, Ne, inv);
        q = q < N ? q : N - 1;
        const float v1 = f1(q), v2 = f2(q);
        const float pa1 = lo[j] * v1, pd1 = hi[j] * v1, pa2 = lo[j] * v2, pd2 = hi[j] * v2;
        a1 = a1 + pa1;
        d1 = d1 + pd1;
        a2 = a2 + pa2;
        d2 = d2 + pd2;
    });
    sa1 = a1;
    sd1 = d1;
    sa2 = a2;
    sd2 = d2;
}

/* wt_ana_point */
template <class Fetch>
WT_CORE void abs_ana(int o, int N, int F, const float* lo, const float* hi, const Fetch& fetch, float& sa, float& sd) {
    const int i = F / 2 + 2 * o, Ne = N + (N & 1), inv = abs_inv(Ne);
    float a = 0.0f, d = 0.0f;
    abs_taps(i - N + 1, F, [&](int j) {
        int q = abs_mod(i - j, Ne, inv);
        q = q < N ? q : N - 1;
        const float v = fetch(q);
        const float pa = lo[j] * v, pd = hi[j] * v;
        a = a + pa;
        d = d + pd;
    });
    sa = a;
    sd = d;
}

/* wt_syn_point for two outputs that share their site (n of the low and of the high half
 * transform): the rec_lo pass over fa1 / fa2, then the rec_hi pass over fd1 / fd2 */
template <class FA1, class FD1, class FA2, class FD2>
WT_CORE void abs_syn2(int n, int N, int F, const float* rlo, const float* rhi, const FA1& fa1, const FD1& fd1,
                      const FA2& fa2, const FD2& fd2, float& y1, float& y2) {
    const wt_syn_site s = wt_syn_locate(n, N, F);
    const int i = (int)s.i, par = s.par, H = F / 2, inv = abs_inv(N);
    const int n1 = s.special ? i + 1 : i - N + 1; /* special: the taps at or right of sample 0 come first */
    float acc1 = 0.0f, acc2 = 0.0f;
    abs_taps(n1, H, [&](int j) {
        const int q = abs_mod(i - j, N, inv);
        const float t = rlo[2 * j + par];
        const float p1 = t * fa1(q), p2 = t * fa2(q);
        acc1 = acc1 + p1;
        acc2 = acc2 + p2;
    });
    abs_taps(n1, H, [&](int j) {
        const int q = abs_mod(i - j, N, inv);
        const float t = rhi[2 * j + par];
        const float p1 = t * fd1(q), p2 = t * fd2(q);
        acc1 = acc1 + p1;
        acc2 = acc2 + p2;
    });
    y1 = acc1;
    y2 = acc2;
}

/* wt_syn_point */
template <class FetchA, class FetchD>
WT_CORE float abs_syn(int n, int N, int F, const float* rlo, const float* rhi, const FetchA& fa, const FetchD& fd) {
    const wt_syn_site s = wt_syn_locate(n, N, F);
    const int i = (int)s.i, par = s.par, H = F / 2, inv = abs_inv(N);
    const int n1 = s.special ? i + 1 : i - N + 1;
    float acc = 0.0f;
    abs_taps(n1, H, [&](int j) { const float p = rlo[2 * j + par] * fa(abs_mod(i - j, N, inv)); acc = acc + p; });
    abs_taps(n1, H, [&](int j) { const float p = rhi[2 * j + par] * fd(abs_mod(i - j, N, inv)); acc = acc + p; });
    return acc;
}

/* level k of an H x W image: its size and the word offset of its three detail blocks in the
 * coefficient area ([cA_L | details of level 1 | level 2 | ...], no padding cells) */
WT_CORE void abs_level(int k, int H, int W, int ca_words, int& R, int& C, int& doff) {
    R = H;
    C = W;
    doff = ca_words;
    for (int j = 1; j <= k; ++j) {
        if (j > 1) doff += 3 * R * C;
        R = (R + 1) >> 1;
        C = (C + 1) >> 1;
    }
}

/* The arena's areas, in words per image: A the image / a level's approximation (the output
 * ends up here, row pitch W), T a level's two half transforms, D the masked coefficients. */
WT_CORE int abs_area_a(int H, int W, int L) {
    const int R1 = (H + 1) >> 1, C1 = (W + 1) >> 1;
    return (L && 4 * R1 * C1 > H * W) ? 4 * R1 * C1 : H * W;
}
WT_CORE int abs_area_t(int H, int W, int L) {
    const int R1 = (H + 1) >> 1, C1 = (W + 1) >> 1;
    return L ? 2 * R1 * (W > 2 * C1 ? W : 2 * C1) : 0;
}
WT_CORE int abs_area_d(int H, int W, int L) {
    if (L == 0) return 0;
    int R = H, C = W, words = 0;
    for (int k = 1; k <= L; ++k) {
        R = (R + 1) >> 1;
        C = (C + 1) >> 1;
        words += 3 * R * C;
    }
    return words + R * C;
}
WT_CORE int abs_tiny_words(int H, int W, int L) { return abs_area_a(H, W, L) + abs_area_t(H, W, L) + abs_area_d(H, W, L); }

/* A wave of k_abs_tiny has 16 KB of LDS: its copy of the four filters (ABS_TAP_WORDS) and the
 * arena (ABS_WAVE_WORDS).  Returns log2 of the lanes used (tiny_lanes_log2), -1 when the image is
 * not a tiny one (a side above ABS_SIDE_MAX, or one image alone does not fit). */
#define ABS_SIDE_MAX 8
#define ABS_TAP_WORDS (4 * ((WTP_MAX_F + 1) / 2 * 2))
#define ABS_WAVE_WORDS (4096 - ABS_TAP_WORDS)
WT_CORE int abs_lanes_log2(int64_t H, int64_t W, int L) {
    if (H < 1 || W < 1 || H > ABS_SIDE_MAX || W > ABS_SIDE_MAX || L < 0) return -1;
    return tiny_lanes_log2(abs_tiny_words((int)H, (int)W, L), ABS_WAVE_WORDS);
}

/* a, tt, dd: the image's word 0 of the areas A (holding the H x W image), T and D; NL: the
 * word stride.  taps: dec_lo, dec_hi, rec_lo, rec_hi. */
WT_CORE void abs_image(float* a, float* tt, float* dd, int NL, int H, int W, int L, int F, const float* dlo,
                       const float* dhi, const float* rlo, const float* rhi, float thr) {
    if (L == 0) {
        for (int s = 0; s < H * W; ++s) a[s * NL] = wt_thr_mask(a[s * NL], thr);
        return;
    }
    int RL, CL, unused;
    abs_level(L, H, W, 0, RL, CL, unused);
    const int caw = RL * CL;
    /* forward: level k reads A (R0 x C0), leaves cA_k in A (R x C) and the masked details in D */
    int R0 = H, C0 = W, doff = caw;
    for (int k = 1; k <= L; ++k) {
        const int R = (R0 + 1) >> 1, C = (C0 + 1) >> 1;
        for (int c = 0; c < C0; ++c)
            for (int o = 0; o < R; ++o) {
                float sa, sd;
                abs_ana(o, R0, F, dlo, dhi, [&](int q) { return a[(q * C0 + c) * NL]; }, sa, sd);
                tt[(o * C0 + c) * NL] = sa;
                tt[((R + o) * C0 + c) * NL] = sd;
            }
        const int last = k == L;
        for (int r = 0; r < R; ++r)
            for (int o = 0; o < C; ++o) {
                float aa, ad, da, d2;
                abs_ana2(o, C0, F, dlo, dhi, [&](int q) { return tt[(r * C0 + q) * NL]; },
                         [&](int q) { return tt[((R + r) * C0 + q) * NL]; }, aa, ad, da, d2);
                const int x = r * C + o;
                if (last) dd[x * NL] = wt_thr_mask(aa, thr);
                else a[x * NL] = aa;
                dd[(doff + x) * NL] = wt_thr_mask(ad, thr);
                dd[(doff + R * C + x) * NL] = wt_thr_mask(da, thr);
                dd[(doff + 2 * R * C + x) * NL] = wt_thr_mask(d2, thr);
            }
        doff += 3 * R * C;
        R0 = R;
        C0 = C;
    }
    /* inverse: level k reads cA_k (D at the top, else A with the row pitch the level above left)
     * and D's details, leaves 2R x 2C in A (the last one cropped to H x W) */
    int lda = CL;
    for (int k = L; k >= 1; --k) {
        int R, C, dk;
        abs_level(k, H, W, caw, R, C, dk);
        const float* ca = (k == L) ? dd : a;
        const float* pad = dd + dk * NL;
        const float* pda = dd + (dk + R * C) * NL;
        const float* pdd = dd + (dk + 2 * R * C) * NL;
        const int C2 = 2 * C;
        for (int r = 0; r < R; ++r)
            for (int n = 0; n < C2; ++n) {
                float vlo, vhi;
                abs_syn2(n, C, F, rlo, rhi, [&](int q) { return ca[(r * lda + q) * NL]; },
                         [&](int q) { return pad[(r * C + q) * NL]; }, [&](int q) { return pda[(r * C + q) * NL]; },
                         [&](int q) { return pdd[(r * C + q) * NL]; }, vlo, vhi);
                tt[(r * C2 + n) * NL] = vlo;
                tt[((R + r) * C2 + n) * NL] = vhi;
            }
        const int oH = (k == 1) ? H : 2 * R, oW = (k == 1) ? W : C2;
        for (int m = 0; m < oH; ++m)
            for (int n = 0; n < oW; ++n)
                a[(m * oW + n) * NL] = abs_syn(m, R, F, rlo, rhi, [&](int q) { return tt[(q * C2 + n) * NL]; },
                                               [&](int q) { return tt[((R + q) * C2 + n) * NL]; });
        lda = oW;
    }
}

#endif

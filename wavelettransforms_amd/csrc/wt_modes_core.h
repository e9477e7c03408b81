/* One level of PyWavelets' float32 filter bank under the signal-extension modes zero, constant,
 * symmetric, reflect and periodic (every mode but periodization, which wt_dwt_core.h holds), the
 * geometry of wavedec2 / coeffs_to_array / waverec2 under them, and the tiny-image kernels'
 * per-image routines (wtm_tiny_fwd / wtm_tiny_inv, at the end).  Shared by the HIP kernels
 * (modes.hip) and the host-side check (tests/native/modescore.cpp).  GATHER forms, each output
 * summed in exactly the order pywt's C code sums it (separate multiply and add -- build with
 * -ffp-contract=off).  The rule was established against pywt.dwt / pywt.idwt bit for bit
 * ("Appendix B"):
 *
 *  analysis (downsampling_convolution): a line of N samples gives floor((N + F - 1) / 2)
 *  outputs; output o is the full convolution at i = 2o + 1, sum over taps j of f[j] * x~[i - j],
 *  x~ the extended line.  Three runs, in this order:
 *     1. the taps that reach past the line's END (i - j >= N, j = 0 .. i - N): from the tap
 *        nearest the data outward, j = i - N down to 0 -- except constant, which runs them
 *        j = 0 up to i - N; zero skips them
 *     2. the taps on the line, j ascending
 *     3. the taps that reach before the line's START (i - j < 0, j = i + 1 .. F - 1), j
 *        ascending (nearest the data outward); zero skips them
 *  A line shorter than the filter is extended as often as the taps need (the extension is
 *  periodic: symmetric 2N, reflect 2N - 2, periodic N); the order rule does not change.
 *  reflect of a one-sample line is undefined (pywt 1.1.1 does not return): wtm_mode_ok.
 *
 *  synthesis (upsampling_convolution_valid_sf, its only branch for these modes): N
 *  coefficients a band give 2N - F + 2 outputs and no tap leaves the line: output n reads
 *  i = F/2 - 1 + n/2 and the taps of parity n & 1, j = 0 .. F/2 - 1 ascending, the rec_lo sum
 *  over cA started from 0 and added to the zeroed output, then the rec_hi sum over cD started
 *  from 0 and added to that: (0 + sum_lo) + sum_hi -- not one running sum, and the 0 + turns a
 *  -0 sum into +0.
 */
#ifndef WT_MODES_CORE_H
#define WT_MODES_CORE_H

#include "wt_tiny_arena.h"

/* == WTP_MODE_* of wtprune.h */
#define WTM_PERIODIZATION 0
#define WTM_ZERO 1
#define WTM_CONSTANT 2
#define WTM_SYMMETRIC 3
#define WTM_REFLECT 4
#define WTM_PERIODIC 5

WT_CORE int wtm_mode_known(int mode) { return mode >= WTM_PERIODIZATION && mode <= WTM_PERIODIC; }
/* whether a line of N samples can be analysed in this mode (F even: the synthesis needs it) */
WT_CORE int wtm_line_ok(int64_t N, int F, int mode) {
    return N >= 1 && F >= 2 && (F & 1) == 0 && !(mode == WTM_REFLECT && N == 1);
}

WT_CORE int64_t wtm_dec_len(int64_t N, int F) { return (N + F - 1) / 2; }
WT_CORE int64_t wtm_rec_len(int64_t N, int F) { return 2 * N - F + 2; }

/* sample index of the extended line at t outside [0, N); -1: the sample is zero */
WT_CORE int64_t wtm_ext_index(int64_t t, int64_t N, int mode) {
    switch (mode) {
        case WTM_CONSTANT: return t < 0 ? 0 : N - 1;
        case WTM_PERIODIC: return wt_pmod(t, N);
        case WTM_SYMMETRIC: {
            const int64_t m = wt_pmod(t, 2 * N);
            return m < N ? m : 2 * N - 1 - m;
        }
        case WTM_REFLECT: {
            const int64_t P = 2 * N - 2, m = wt_pmod(t, P);
            return m < N ? m : P - m;
        }
        default: return -1;
    }
}

/* One analysis output o (both bands) of a line of N samples.  Fetch(k): sample k, 0 <= k < N. */
template <class Fetch>
WT_CORE void wtm_ana_point(int64_t o, int64_t N, int F, const float* lo, const float* hi, int mode,
                           const Fetch& fetch, float& sa, float& sd) {
    const int64_t i = 2 * o + 1;
    float a = 0.0f, d = 0.0f;
    int j0 = (int)(i - N + 1 > 0 ? i - N + 1 : 0);          /* first tap on the line */
    const int j1 = (int)(i < F - 1 ? i : F - 1);             /* last tap on the line */
    if (j0 > F) j0 = F;
    if (mode != WTM_ZERO) {
        if (mode == WTM_CONSTANT) {
            const float v = fetch(N - 1);
            for (int j = 0; j < j0; ++j) {
                const float pa = lo[j] * v, pd = hi[j] * v;
                a = a + pa;
                d = d + pd;
            }
        } else {
            for (int j = j0 - 1; j >= 0; --j) {
                const float v = fetch(wtm_ext_index(i - j, N, mode));
                const float pa = lo[j] * v, pd = hi[j] * v;
                a = a + pa;
                d = d + pd;
            }
        }
    }
    for (int j = j0; j <= j1; ++j) {
        const float v = fetch(i - j);
        const float pa = lo[j] * v, pd = hi[j] * v;
        a = a + pa;
        d = d + pd;
    }
    if (mode != WTM_ZERO) {
        for (int j = j1 + 1; j < F; ++j) {
            const float v = fetch(wtm_ext_index(i - j, N, mode));
            const float pa = lo[j] * v, pd = hi[j] * v;
            a = a + pa;
            d = d + pd;
        }
    }
    sa = a;
    sd = d;
}

/* One synthesis output n of 2N - F + 2.  FetchA / FetchD(k), 0 <= k < N. */
template <class FetchA, class FetchD>
WT_CORE float wtm_syn_point(int64_t n, int F, const float* rlo, const float* rhi, const FetchA& fa,
                            const FetchD& fd) {
    const int H = F / 2, par = (int)(n & 1);
    const int64_t i = H - 1 + n / 2;
    float s = 0.0f;
    for (int j = 0; j < H; ++j) { const float p = rlo[2 * j + par] * fa(i - j); s = s + p; }
    const float y = 0.0f + s;
    s = 0.0f;
    for (int j = 0; j < H; ++j) { const float p = rhi[2 * j + par] * fd(i - j); s = s + p; }
    return y + s;
}

/* ---- geometry: pywt.wavedec2 over axes (-2, -1), pywt.coeffs_to_array, pywt.waverec2 ----
 * R[k] = floor((R[k-1] + F - 1) / 2); the packed image stacks the blocks as wt_geom does (the
 * detail blocks of level k sit at (offR[k], offC[k]), cA_L at the origin), so it is larger than
 * the image and in general not tight: the cells no block covers are zeros, and they belong to the
 * percentile's population.  Level k's synthesis gives 2 R[k] - F + 2 rows, R[k-1] or one more:
 * waverec2 drops that last row before level k - 1 (its inter-level crop), so every level WRITES
 * R[k-1] x C[k-1]; what the reference's final crop sees is wtm_out_len(R[1]). */
WT_CORE void wtm_geom(int64_t H, int64_t W, int L, int F, int mode, wt_level_geom* g) {
    wt_geom(H, W, L, g, mode == WTM_PERIODIZATION ? 2 : F);
}
/* whether every level's input lines can be analysed (wtm_line_ok: a two-sample line becomes a
 * one-sample line under haar, which reflect cannot extend) */
WT_CORE int wtm_levels_ok(int64_t H, int64_t W, int L, int F, int mode) {
    if (mode == WTM_PERIODIZATION) return 1;
    for (int k = 1; k <= L; ++k) {
        if (!wtm_line_ok(H, F, mode) || !wtm_line_ok(W, F, mode)) return 0;
        H = wtm_dec_len(H, F);
        W = wtm_dec_len(W, F);
    }
    return 1;
}
/* the size waverec2 returns along an axis whose level-1 band has N1 coefficients */
WT_CORE int64_t wtm_out_len(int64_t N1, int F, int mode) { return mode == WTM_PERIODIZATION ? 2 * N1 : wtm_rec_len(N1, F); }
/* coefficients the blocks hold (the rest of PR x PC is padding) */
WT_CORE int64_t wtm_block_cells(const wt_level_geom* g, int L) {
    if (L == 0) return g->PR * g->PC;
    int64_t nc = g->R[L] * g->C[L];
    for (int k = 1; k <= L; ++k) nc += 3 * g->R[k] * g->C[k];
    return nc;
}

/* ---- tiny images (both sides <= WTM_SIDE_MAX): k_mtiny_fwd / k_mtiny_inv keep one image per
 * lane in a wave's LDS arena (wt_tiny_arena.h), in words per image: A the image, a level's
 * approximation or a level's synthesis output (R[k] x C[k], k < L); T a level's two half
 * transforms (2 R[k] x C[k-1]); D the packed image (PR x PC, row pitch PC).
 * wtm_tiny_lanes_log2: log2 of the lanes used, -1 when the tensor is not a tiny one. */
#define WTM_SIDE_MAX 8
#define WTM_TINY_LMAX 4
#define WTM_TINY_F_MAX 4
#define WTM_WAVE_WORDS 8192
/* wtm_geom of a tiny image in small ints (1 <= L <= WTM_TINY_LMAX).  The kernels keep it in LDS:
 * the level loops index it, and indexed private arrays would go to scratch. */
struct wtm_tiny_geom {
    int R[WTM_TINY_LMAX + 1], C[WTM_TINY_LMAX + 1], offR[WTM_TINY_LMAX + 1], offC[WTM_TINY_LMAX + 1], PR, PC;
};
WT_CORE void wtm_tiny_geometry(int H, int W, int L, int F, wtm_tiny_geom& g) {
    g.R[0] = H;
    g.C[0] = W;
    for (int k = 1; k <= L; ++k) { g.R[k] = (g.R[k - 1] + F - 1) >> 1; g.C[k] = (g.C[k - 1] + F - 1) >> 1; }
    int aR = g.R[L], aC = g.C[L];
    for (int k = L; k >= 1; --k) { g.offR[k] = aR; g.offC[k] = aC; aR += g.R[k]; aC += g.C[k]; }
    g.PR = aR;
    g.PC = aC;
}
/* The areas walk the sizes in scalars and not out of a wtm_tiny_geom: the kernels place T and D
 * with them, and from the geometry in LDS those offsets cost vector registers. */
WT_CORE int wtm_tiny_area_a(int H, int W, int L, int F) {
    int R = H, C = W, words = H * W;
    for (int k = 1; k < L; ++k) {
        R = (R + F - 1) >> 1;
        C = (C + F - 1) >> 1;
        if (R * C > words) words = R * C;
    }
    return words;
}
WT_CORE int wtm_tiny_area_t(int H, int W, int L, int F) {
    int R = H, C = W, words = 0;
    for (int k = 1; k <= L; ++k) {
        const int C0 = C;
        R = (R + F - 1) >> 1;
        C = (C + F - 1) >> 1;
        if (2 * R * C0 > words) words = 2 * R * C0;
    }
    return words;
}
WT_CORE int wtm_tiny_area_d(int H, int W, int L, int F) {
    int PR, PC;
    tiny_packed_size(H, W, L, F, PR, PC);
    return PR * PC;
}
WT_CORE int wtm_tiny_lanes_log2(int64_t H, int64_t W, int L, int F) {
    if (H < 1 || W < 1 || H > WTM_SIDE_MAX || W > WTM_SIDE_MAX || L < 1 || L > WTM_TINY_LMAX || F > WTM_TINY_F_MAX) return -1;
    const int h = (int)H, w = (int)W;
    const int words = wtm_tiny_area_a(h, w, L, F) + wtm_tiny_area_t(h, w, L, F) + wtm_tiny_area_d(h, w, L, F);
    return tiny_lanes_log2(words, WTM_WAVE_WORDS);
}

/* The per-image routines of k_mtiny_fwd / k_mtiny_inv.  a, tt, dd: the image's word 0 of the
 * areas A, T and D; NL: the word stride.
 * wtm_tiny_fwd: every analysis level of the H x W image in A into the packed image in D (the cells
 * no block covers are not written: the caller zero-fills D). */
WT_CORE void wtm_tiny_fwd(float* a, float* tt, float* dd, int NL, const wtm_tiny_geom& g, int L, int F, int mode,
                          const float* dlo, const float* dhi) {
    const int PC = g.PC;
    for (int k = 1; k <= L; ++k) {
        const int R0 = g.R[k - 1], C0 = g.C[k - 1], R = g.R[k], C = g.C[k];
        for (int c = 0; c < C0; ++c)
            for (int o = 0; o < R; ++o) {
                float sa, sd;
                wtm_ana_point(o, R0, F, dlo, dhi, mode, [&](int64_t q) { return a[((int)q * C0 + c) * NL]; }, sa, sd);
                tt[(o * C0 + c) * NL] = sa;
                tt[((R + o) * C0 + c) * NL] = sd;
            }
        const int last = k == L;
        for (int r = 0; r < R; ++r)
            for (int o = 0; o < C; ++o) {
                float aa, ad, da, d2;
                wtm_ana_point(o, C0, F, dlo, dhi, mode, [&](int64_t q) { return tt[(r * C0 + (int)q) * NL]; }, aa, ad);
                wtm_ana_point(o, C0, F, dlo, dhi, mode, [&](int64_t q) { return tt[((R + r) * C0 + (int)q) * NL]; },
                              da, d2);
                if (last) dd[(r * PC + o) * NL] = aa;
                else a[(r * C + o) * NL] = aa;
                dd[(r * PC + g.offC[k] + o) * NL] = ad;
                dd[((g.offR[k] + r) * PC + o) * NL] = da;
                dd[((g.offR[k] + r) * PC + g.offC[k] + o) * NL] = d2;
            }
    }
}
/* wtm_tiny_inv: every synthesis level out of the packed image in D, already thresholded, into A
 * (H x W, row pitch W).  Level k reads cA_k from D at the top (row pitch PC), else from A where
 * the level above left it, and writes R[k-1] x C[k-1]: waverec2's inter-level crop and, at
 * k = 1, the final one. */
WT_CORE void wtm_tiny_inv(float* a, float* tt, const float* dd, int NL, const wtm_tiny_geom& g, int L, int F,
                          const float* rlo, const float* rhi) {
    const int PC = g.PC;
    for (int k = L; k >= 1; --k) {
        const int R = g.R[k], C = g.C[k], oH = g.R[k - 1], oW = g.C[k - 1];
        const float* ca = (k == L) ? dd : a;
        const int lda = (k == L) ? PC : C;
        const float* pad = dd + g.offC[k] * NL;
        const float* pda = dd + g.offR[k] * PC * NL;
        const float* pdd = dd + (g.offR[k] * PC + g.offC[k]) * NL;
        for (int r = 0; r < R; ++r)
            for (int n = 0; n < oW; ++n) {
                tt[(r * oW + n) * NL] =
                    wtm_syn_point(n, F, rlo, rhi, [&](int64_t q) { return ca[(r * lda + (int)q) * NL]; },
                                  [&](int64_t q) { return pad[(r * PC + (int)q) * NL]; });
                tt[((R + r) * oW + n) * NL] =
                    wtm_syn_point(n, F, rlo, rhi, [&](int64_t q) { return pda[(r * PC + (int)q) * NL]; },
                                  [&](int64_t q) { return pdd[(r * PC + (int)q) * NL]; });
            }
        for (int m = 0; m < oH; ++m)
            for (int n = 0; n < oW; ++n)
                a[(m * oW + n) * NL] =
                    wtm_syn_point(m, F, rlo, rhi, [&](int64_t q) { return tt[((int)q * oW + n) * NL]; },
                                  [&](int64_t q) { return tt[((R + (int)q) * oW + n) * NL]; });
    }
}

#endif


/* abs_image of wt_abs_core.h cut at its mask, for the absolute-threshold sweep (k_abs_tiny_sweep
 * of abs.hip, wtp_prune_abs_sweep_f32): the coefficients do not depend on the threshold, so the
 * forward half runs once and leaves them RAW in the area D, and every threshold's inverse half
 * runs over that same D, masking a coefficient as it reads it.  The mask is pointwise, so masking
 * on the read instead of on the write changes no rounding: abs_forward_raw followed by
 * abs_inverse_masked(thr) leaves in A, bit for bit, what abs_image(thr) leaves there, and the
 * inverse writes A and T only, so it can run again at another threshold.  The areas and their
 * sizes are abs_image's (abs_area_a / _t / _d): the arena does not grow.  Shared by the kernel
 * and the host-side check (tests/native/abssweepcore.cpp).  Build with -ffp-contract=off.
 *
 * Level 0 has no coefficient area (the image in A is its own coefficient array), so both
 * routines leave A as it is there: the caller masks each word as it copies it out.
 */
#ifndef WT_ABS_SWEEP_CORE_H
#define WT_ABS_SWEEP_CORE_H

#include "wt_abs_core.h"

/* a, tt, dd: the image's word 0 of the areas A (holding the H x W image), T and D; NL: the word
 * stride.  Leaves [cA_L | details of level 1 | level 2 | ...] unmasked in D. */
WT_CORE void abs_forward_raw(float* a, float* tt, float* dd, int NL, int H, int W, int L, int F, const float* dlo,
                             const float* dhi) {
    if (L == 0) return;
    int RL, CL, unused;
    abs_level(L, H, W, 0, RL, CL, unused);
    int R0 = H, C0 = W, doff = RL * CL;
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
                if (last) dd[x * NL] = aa;
                else a[x * NL] = aa;
                dd[(doff + x) * NL] = ad;
                dd[(doff + R * C + x) * NL] = da;
                dd[(doff + 2 * R * C + x) * NL] = d2;
            }
        doff += 3 * R * C;
        R0 = R;
        C0 = C;
    }
}

/* The inverse half over the raw D of abs_forward_raw: cA_L and every detail are masked at thr
 * as they are read from D, the reconstructed approximations in A are not (abs_image masks no
 * approximation below level L either).  Reads D, writes T and A; the H x W result ends up in A
 * with row pitch W. */
WT_CORE void abs_inverse_masked(float* a, float* tt, const float* dd, int NL, int H, int W, int L, int F,
                                const float* rlo, const float* rhi, float thr) {
    if (L == 0) return;
    int RL, CL, unused;
    abs_level(L, H, W, 0, RL, CL, unused);
    const int caw = RL * CL;
    int lda = CL;
    for (int k = L; k >= 1; --k) {
        int R, C, dk;
        abs_level(k, H, W, caw, R, C, dk);
        /* cA_k: D's (masked) at the top, else A's as the level above left it -- a NaN threshold
         * masks nothing, so one tap body serves both */
        const float* ca = (k == L) ? dd : a;
        const float tca = (k == L) ? thr : __builtin_nanf("");
        const float* pad = dd + dk * NL;
        const float* pda = dd + (dk + R * C) * NL;
        const float* pdd = dd + (dk + 2 * R * C) * NL;
        const int C2 = 2 * C;
        for (int r = 0; r < R; ++r)
            for (int n = 0; n < C2; ++n) {
                float vlo, vhi;
                abs_syn2(n, C, F, rlo, rhi, [&](int q) { return wt_thr_mask(ca[(r * lda + q) * NL], tca); },
                         [&](int q) { return wt_thr_mask(pad[(r * C + q) * NL], thr); },
                         [&](int q) { return wt_thr_mask(pda[(r * C + q) * NL], thr); },
                         [&](int q) { return wt_thr_mask(pdd[(r * C + q) * NL], thr); }, vlo, vhi);
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

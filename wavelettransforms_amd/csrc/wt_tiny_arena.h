/* The wave arena of the tiny-image kernels (k_abs_tiny / k_abs_tiny_sweep of abs.hip, k_mtiny_fwd /
 * k_mtiny_inv of modes.hip): a wave, which is a workgroup, takes NL images of one tensor, one image
 * per lane, and keeps word s of image i at arena[s * NL + i], so every LDS access is a wave-uniform
 * offset plus the lane.  The per-image routines (abs_image of wt_abs_core.h, wtm_tiny_fwd / wtm_tiny_inv of
 * wt_modes_core.h) get their image's word 0 and the stride NL; here is what surrounds them.  The
 * arena's size is the caller's (ABS_WAVE_WORDS, WTM_WAVE_WORDS).  The device part serves the two
 * k_mtiny_* and k_abs_tiny_sweep; k_abs_tiny measured 0.2 % slower on it and keeps its own text
 * (DESIGN.md). */
#ifndef WT_TINY_ARENA_H
#define WT_TINY_ARENA_H

#include "wt_dwt_core.h"

#define TINY_THREADS 64 /* a wave */

/* A wave takes 64 images unless their words do not fit its arena: then 32, 16, ... (the other
 * lanes idle).  log2 of the lanes used, -1 when one image alone does not fit. */
WT_CORE int tiny_lanes_log2(int words, int wave_words) {
    int lg = 6;
    while (lg > 0 && (words << lg) > wave_words) --lg;
    return (words << lg) <= wave_words ? lg : -1;
}
/* waves of a tensor of B images */
WT_CORE int64_t tiny_waves(int64_t B, int lg) { return (B + (1 << lg) - 1) >> lg; }

/* the packed image's size (wt_geom's for F = 2, wtm_geom's otherwise) without the level arrays */
WT_CORE void tiny_packed_size(int H, int W, int L, int F, int& PR, int& PC) {
    int R = H, C = W, sR = 0, sC = 0;
    for (int k = 1; k <= L; ++k) {
        R = (R + F - 1) >> 1;
        C = (C + F - 1) >> 1;
        sR += R;
        sC += C;
    }
    PR = L ? sR + R : H; /* level L's size counts twice: cA_L beside its details */
    PC = L ? sC + C : W;
}

/* The next segment of a launch table (AbsTable, AbsSweepTable, MTinyTable: nseg, nwave,
 * wave_begin[], s[] whose elements have in, B, H, W, L, nl_log2); the caller fills the rest of it,
 * its output or outputs first. */
template <class Table>
static inline auto& tiny_append(Table& tab, const float* in, int64_t B, int64_t H, int64_t W, int L, int lg) {
    auto& sg = tab.s[tab.nseg];
    sg.in = in;
    sg.B = (int32_t)B;
    sg.H = (uint8_t)H;
    sg.W = (uint8_t)W;
    sg.L = (uint8_t)L;
    sg.nl_log2 = (uint8_t)lg;
    tab.wave_begin[tab.nseg++] = tab.nwave;
    tab.nwave += (int32_t)tiny_waves(B, lg);
    return sg;
}

#if defined(__HIPCC__)
/* the workgroup's segment sg, its place w among the segment's waves and its images [b0, b0 + nimg) */
struct TinyWave {
    int sg, w, nimg;
    int64_t b0;
};
template <class Table>
__device__ __forceinline__ TinyWave tiny_wave(const Table& t) {
    const int gw = blockIdx.x;
    TinyWave v;
    v.sg = 0;
    for (int i = 1; i < t.nseg; ++i) v.sg += gw >= t.wave_begin[i];
    v.w = gw - t.wave_begin[v.sg];
    const int NL = 1 << t.s[v.sg].nl_log2;
    v.b0 = (int64_t)v.w * NL;
    v.nimg = (int)(t.s[v.sg].B - v.b0 < NL ? t.s[v.sg].B - v.b0 : NL);
    return v;
}

/* nimg images of `words` words, dense at src, into the area A: coalesced reads; fn(value) is stored */
template <class Fn>
__device__ __forceinline__ void tiny_load(float* A, int NL, const float* src, int nimg, int words, const Fn& fn) {
    for (int e = threadIdx.x; e < nimg * words; e += TINY_THREADS) {
        const int img = e / words, s = e - img * words;
        A[s * NL + img] = fn(src[e]);
    }
}
/* ... and back, coalesced writes; fn(value) sees every word stored */
template <class Fn>
__device__ __forceinline__ void tiny_store(float* dst, const float* A, int NL, int nimg, int words, const Fn& fn) {
    for (int e = threadIdx.x; e < nimg * words; e += TINY_THREADS) {
        const int img = e / words, s = e - img * words;
        const float v = A[s * NL + img];
        dst[e] = v;
        fn(v);
    }
}

/* the first n taps tap(k, j) of the four filters to ltap[k * pitch + j]: a tap is then a broadcast
 * LDS read that returns in order with the sample reads, so a tap loop keeps several in flight (a
 * scalar load per tap from the kernel argument returns out of order: every tap waits for all) */
template <class Tap>
__device__ __forceinline__ void tiny_stage_taps(float* ltap, int pitch, int n, const Tap& tap) {
    for (int e = threadIdx.x; e < 4 * n; e += TINY_THREADS) {
        const int k = e / n, j = e - k * n;
        ltap[k * pitch + j] = tap(k, j);
    }
}
#endif

#endif

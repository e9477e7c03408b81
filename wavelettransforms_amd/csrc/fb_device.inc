/*
 * fb_device.inc -- what the four filter-bank kernels share on the device (filterbank.hip includes it
 * first): the packed float pair, the extension indices, one analysis output (ana2*) and one
 * synthesis pass (syn_pass_*) in PyWavelets' summation order, the occupancy attributes and the
 * lab's timing probes.  The tile geometry comes from fb_plan.h.
 */
#include "wtp_internal.h"
#include "wt_dwt_core.h"
#include "fb_index.h"
#include "fb_plan.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace wtp {

typedef float f2 __attribute__((ext_vector_type(2)));

/* timing probes for tools/mb/fblab.hip (empty in the library) */
#ifndef WTP_FPROBE
#define WTP_FPROBE(i)
#endif

/* waves per SIMD the filter-bank kernels are register-budgeted for (db8: 5 needs <= 96 VGPRs) */
#define WTP_FB_FWD_WPE __attribute__((amdgpu_waves_per_eu(5)))
#define WTP_FB_INV_WPE __attribute__((amdgpu_waves_per_eu(5)))
#define WTP_FB_INT_WPE __attribute__((amdgpu_waves_per_eu(EDGE ? 5 : 6))) /* EDGE: room for the edge forms */

/* the forward input tile's first column and row pitch in LDS (fb_plan.h), as the kernels name them */
template <int FT> constexpr int FWD_S0 = fwd_s0(FT);
template <int FT> constexpr int FWD_TP = fwd_tp(FT);
/* the general kernels take any filter (Taps); the specialised ones only as many taps as they use */
template <int FT> using TapsT = typename std::conditional<FT == 0, Taps, SmallTaps>::type;

__device__ __forceinline__ int ext_idx(int t, int N) { /* wt_ext_index in 32 bits */
    const int Ne = N + (N & 1);
    int r = t % Ne;
    r = r < 0 ? r + Ne : r;
    return r < N ? r : N - 1;
}
__device__ __forceinline__ int pmod32(int a, int m) {
    const int r = a % m;
    return r < 0 ? r + m : r;
}

/* analysis of one output (both bands) at site i = F/2 + 2o of a line of N samples;
 * get(g) returns the sample at unwrapped position g (the tile already holds the extension) */
template <int FT, class Get>
__device__ __forceinline__ f2 ana2(int i, int N, int Frt, const float* lo, const float* hi, const Get& get) {
    f2 acc = {0.0f, 0.0f};
    if constexpr (FT > 0) {
        /* every sample the output needs (positions i-j, j < F) is read into registers first,
         * so the LDS reads issue back to back; then the sum runs in pywt's order */
        float v[FT];
#pragma unroll
        for (int j = 0; j < FT; ++j) v[j] = get(i - j);
        if (i < N) {
#pragma unroll
            for (int j = 0; j < FT; ++j) { const f2 t = {lo[j], hi[j]}; acc = acc + t * v[j]; }
        } else {
#pragma unroll
            for (int j = FT - 1; j >= 0; --j)
                if (i - j >= N) { const f2 t = {lo[j], hi[j]}; acc = acc + t * v[j]; }
#pragma unroll
            for (int j = 0; j < FT; ++j)
                if (i - j < N) { const f2 t = {lo[j], hi[j]}; acc = acc + t * v[j]; }
        }
    } else {
        const int F = Frt;
        if (i < N) {
            for (int j = 0; j < F; ++j) { const f2 t = {lo[j], hi[j]}; acc = acc + t * get(i - j); }
        } else {
            for (int j = F - 1; j >= 0; --j)
                if (i - j >= N) { const f2 t = {lo[j], hi[j]}; acc = acc + t * get(i - j); }
            for (int j = 0; j < F; ++j)
                if (i - j < N) { const f2 t = {lo[j], hi[j]}; acc = acc + t * get(i - j); }
        }
    }
    return acc;
}

/* ana2 for specialised filters with the samples already in registers: samp(j) is the sample
 * at position i - j (a compile-time register index after unrolling) */
template <int FT, class Samp>
__device__ __forceinline__ f2 ana2_j(int i, int N, const float* lo, const float* hi, const Samp& samp) {
    f2 acc = {0.0f, 0.0f};
    if (__all(i < N)) { /* wave-uniform: the interior form, no predication */
#pragma unroll
        for (int j = 0; j < FT; ++j) { const f2 t = {lo[j], hi[j]}; acc = acc + t * samp(j); }
    } else if (i < N) {
#pragma unroll
        for (int j = 0; j < FT; ++j) { const f2 t = {lo[j], hi[j]}; acc = acc + t * samp(j); }
    } else {
#pragma unroll
        for (int j = FT - 1; j >= 0; --j)
            if (i - j >= N) { const f2 t = {lo[j], hi[j]}; acc = acc + t * samp(j); }
#pragma unroll
        for (int j = 0; j < FT; ++j)
            if (i - j < N) { const f2 t = {lo[j], hi[j]}; acc = acc + t * samp(j); }
    }
    return acc;
}

/* two analysis outputs at the same site sharing taps (e.g. the L and H rows): returns
 * (lo.x, hi.x) in r0 and (lo.y, hi.y) in r1, each band carried packed over the two rows */
template <int FT, class Get>
__device__ __forceinline__ void ana2x2(int i, int N, int Frt, const float* lo, const float* hi, const Get& get,
                                       f2& low, f2& high) {
    f2 a = {0.0f, 0.0f}, d = {0.0f, 0.0f};
    if constexpr (FT > 0) {
        f2 v[FT];
#pragma unroll
        for (int j = 0; j < FT; ++j) v[j] = get(i - j);
        auto term = [&](int j) { a = a + lo[j] * v[j]; d = d + hi[j] * v[j]; };
        if (__all(i < N)) { /* wave-uniform: the interior form, no predication */
#pragma unroll
            for (int j = 0; j < FT; ++j) term(j);
        } else if (i < N) {
#pragma unroll
            for (int j = 0; j < FT; ++j) term(j);
        } else {
#pragma unroll
            for (int j = FT - 1; j >= 0; --j)
                if (i - j >= N) term(j);
#pragma unroll
            for (int j = 0; j < FT; ++j)
                if (i - j < N) term(j);
        }
    } else {
        const int F = Frt;
        auto term = [&](int j) { const f2 v = get(i - j); a = a + lo[j] * v; d = d + hi[j] * v; };
        if (i < N) {
            for (int j = 0; j < F; ++j) term(j);
        } else {
            for (int j = F - 1; j >= 0; --j)
                if (i - j >= N) term(j);
            for (int j = 0; j < F; ++j)
                if (i - j < N) term(j);
        }
    }
    low = a;
    high = d;
}

/* synthesis site with an unwrapped source position: the H-even special last output n = 2N-1
 * reads positions i - j + N (== i - j mod N), so a tile's sites increase monotonically */
struct SiteU {
    int i, iu, par, special;
};
__device__ __forceinline__ SiteU site_u(int n, int N, int F) {
    const wt_syn_site s = wt_syn_locate(n, N, F);
    SiteU u;
    u.i = (int)s.i;
    u.par = s.par;
    u.special = s.special;
    u.iu = u.i + ((s.special && n == 2 * N - 1) ? N : 0);
    return u;
}

/* one synthesis pass (H terms) in wt_syn_pass's exact order; get(g) at unwrapped g = iu - j;
 * tap(j) = rec[2j + par] for this output's parity */
template <int FT, class T, class Tap, class Get>
__device__ __forceinline__ T syn_pass_u(const SiteU& s, int N, int Frt, const Tap& tap, const Get& get, T acc) {
    const int i = s.i;
    if constexpr (FT > 0) {
        constexpr int H = FT / 2;
        T v[H];
#pragma unroll
        for (int j = 0; j < H; ++j) v[j] = get(s.iu - j);
        if (s.special) {
#pragma unroll
            for (int j = H - 1; j >= 0; --j)
                if (i - j >= 0) acc = acc + tap(j) * v[j];
#pragma unroll
            for (int j = 0; j < H; ++j)
                if (i - j < 0) acc = acc + tap(j) * v[j];
        } else if (i < N) {
#pragma unroll
            for (int j = 0; j < H; ++j) acc = acc + tap(j) * v[j];
        } else {
#pragma unroll
            for (int j = H - 1; j >= 0; --j)
                if (i - j >= N) acc = acc + tap(j) * v[j];
#pragma unroll
            for (int j = 0; j < H; ++j)
                if (i - j < N) acc = acc + tap(j) * v[j];
        }
    } else {
        const int H = Frt / 2;
        if (s.special) {
            for (int j = H - 1; j >= 0; --j)
                if (i - j >= 0) acc = acc + tap(j) * get(s.iu - j);
            for (int j = 0; j < H; ++j)
                if (i - j < 0) acc = acc + tap(j) * get(s.iu - j);
        } else if (i < N) {
            for (int j = 0; j < H; ++j) acc = acc + tap(j) * get(s.iu - j);
        } else {
            for (int j = H - 1; j >= 0; --j)
                if (i - j >= N) acc = acc + tap(j) * get(s.iu - j);
            for (int j = 0; j < H; ++j)
                if (i - j < N) acc = acc + tap(j) * get(s.iu - j);
        }
    }
    return acc;
}

/* the interior form of syn_pass_u (not special, i < N): ascending taps */
template <int FT, class T, class Tap, class Get>
__device__ __forceinline__ T syn_pass_inner(const SiteU& s, int Frt, const Tap& tap, const Get& get, T acc) {
    if constexpr (FT > 0) {
        constexpr int H = FT / 2;
        T v[H];
#pragma unroll
        for (int j = 0; j < H; ++j) v[j] = get(s.iu - j);
#pragma unroll
        for (int j = 0; j < H; ++j) acc = acc + tap(j) * v[j];
    } else {
        for (int j = 0; j < Frt / 2; ++j) acc = acc + tap(j) * get(s.iu - j);
    }
    return acc;
}

}  // namespace wtp

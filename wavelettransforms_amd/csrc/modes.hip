/*
 * modes.hip -- the filter bank under PyWavelets' signal-extension modes zero, constant,
 * symmetric, reflect and periodic (wtp_prune_mode_f32 and the mode component entries; the
 * arithmetic and the geometry are csrc/wt_modes_core.h, shared with the host-side check).
 *
 *   k_mtiny_fwd / k_mtiny_inv   tensors whose images are at most 8 x 8 (conv kernels): a wave per
 *                tensor slice, one image per lane in a sample-major LDS arena (wt_tiny_arena.h;
 *                the level loops are wtm_tiny_fwd / wtm_tiny_inv of wt_modes_core.h).  k_mtiny_fwd
 *                reads an image once, runs every analysis level on chip and stores the packed
 *                coefficient image, padding zeros included (the percentile's population);
 *                after the selection k_mtiny_inv reads the packed image once,
 *                thresholds it on load, runs every synthesis level and waverec2's crops on chip
 *                and stores the weights, counting their zeros.
 *   k_mdwt_cols / k_mdwt_rows / k_midwt_rows / k_midwt_cols   every other tensor, a level at a
 *                time over the packed array in the workspace: one output per thread, gathered
 *                with wtm_ana_point / wtm_syn_point.  A point whose taps all lie on the line takes
 *                only the middle run of wtm_ana_point: interior points never see the extension.
 *
 * A level's output is floor((N + F - 1) / 2) a side, sampled at the odd sites of the full
 * convolution: the periodized kernels of levels.inc / filterbank.hip (ceil(N / 2), sites
 * F/2 + 2o, circular indexing) do not compute these values anywhere, so nothing of them is reused.
 */
#include "wtp_device.h"
#include "wt_modes_core.h"

#pragma clang fp contract(off)

namespace wtp {

constexpr int MDWT_THREADS = 256;

/* axis -2 analysis: in (B, R, C) -> L, H (B, Ro, C), Ro = wtm_dec_len(R) */
__global__ __launch_bounds__(MDWT_THREADS) void k_mdwt_cols(const float* __restrict__ in, int64_t B, int64_t R,
                                                            int64_t C, int64_t Ro, Taps tp, int mode,
                                                            float* __restrict__ L, float* __restrict__ H) {
    const int64_t total = B * Ro * C;
    for (int64_t idx = (int64_t)blockIdx.x * MDWT_THREADS + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * MDWT_THREADS) {
        const int64_t c = idx % C, t = idx / C, o = t % Ro, b = t / Ro;
        const float* x = in + b * R * C + c;
        float a, d;
        wtm_ana_point(o, R, tp.F, tp.f[0], tp.f[1], mode, [&](int64_t k) { return x[k * C]; }, a, d);
        L[idx] = a;
        H[idx] = d;
    }
}

/* axis -1 analysis of L and H (B, Ro, C) -> aa (the next level's input (B, Ro, Co), or the packed
 * cA when last), ad, da, dd into the packed array */
__global__ __launch_bounds__(MDWT_THREADS) void k_mdwt_rows(const float* __restrict__ L, const float* __restrict__ H,
                                                            int64_t B, int64_t Ro, int64_t C, int64_t Co, Taps tp,
                                                            int mode, float* __restrict__ anext,
                                                            float* __restrict__ P, int64_t PR, int64_t PC,
                                                            int64_t offR, int64_t offC, int last) {
    const int64_t total = B * Ro * Co;
    for (int64_t idx = (int64_t)blockIdx.x * MDWT_THREADS + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * MDWT_THREADS) {
        const int64_t o = idx % Co, t = idx / Co, r = t % Ro, b = t / Ro;
        const float* lrow = L + (b * Ro + r) * C;
        const float* hrow = H + (b * Ro + r) * C;
        float aa, ad, da, dd;
        wtm_ana_point(o, C, tp.F, tp.f[0], tp.f[1], mode, [&](int64_t k) { return lrow[k]; }, aa, ad);
        wtm_ana_point(o, C, tp.F, tp.f[0], tp.f[1], mode, [&](int64_t k) { return hrow[k]; }, da, dd);
        float* Pb = P + b * PR * PC;
        if (last) Pb[r * PC + o] = aa;
        else anext[idx] = aa;
        Pb[r * PC + offC + o] = ad;
        Pb[(offR + r) * PC + o] = da;
        Pb[(offR + r) * PC + offC + o] = dd;
    }
}

/* axis -1 synthesis: (aa, ad) -> lo, (da, dd) -> hi, each (B, R, oW) with oW <= 2C - F + 2 (the
 * crop).  a: the packed cA (a_from_P) or the level above's output (B, R, C), dense.  Every
 * coefficient read from the packed array is thresholded on load. */
__global__ __launch_bounds__(MDWT_THREADS) void k_midwt_rows(const float* __restrict__ a, int a_from_P,
                                                             const float* __restrict__ P, int64_t PR, int64_t PC,
                                                             int64_t offR, int64_t offC, int64_t B, int64_t R,
                                                             int64_t C, int64_t oW, Taps tp, const float* thrp,
                                                             float* __restrict__ lo, float* __restrict__ hi) {
    const float thr = thrp ? *thrp : 0.0f; /* |c| < 0 never holds: no threshold */
    const int64_t total = B * R * oW;
    for (int64_t idx = (int64_t)blockIdx.x * MDWT_THREADS + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * MDWT_THREADS) {
        const int64_t n = idx % oW, t = idx / oW, r = t % R, b = t / R;
        const float* Pb = P + b * PR * PC;
        const float* arow = a_from_P ? Pb + r * PC : a + (b * R + r) * C;
        const float* adr = Pb + r * PC + offC;
        const float* dar = Pb + (offR + r) * PC;
        const float* ddr = Pb + (offR + r) * PC + offC;
        float vlo;
        if (a_from_P)
            vlo = wtm_syn_point(n, tp.F, tp.f[2], tp.f[3], [&](int64_t k) { return wt_thr_mask(arow[k], thr); },
                                [&](int64_t k) { return wt_thr_mask(adr[k], thr); });
        else
            vlo = wtm_syn_point(n, tp.F, tp.f[2], tp.f[3], [&](int64_t k) { return arow[k]; },
                                [&](int64_t k) { return wt_thr_mask(adr[k], thr); });
        const float vhi = wtm_syn_point(n, tp.F, tp.f[2], tp.f[3], [&](int64_t k) { return wt_thr_mask(dar[k], thr); },
                                        [&](int64_t k) { return wt_thr_mask(ddr[k], thr); });
        lo[idx] = vlo;
        hi[idx] = vhi;
    }
}

/* axis -2 synthesis: lo, hi (B, R, oW) -> y (B, oH, oW), oH <= 2R - F + 2 (the crop); optionally
 * counts the exact zeros of y (the last level writes the pruned weights) */
__global__ __launch_bounds__(MDWT_THREADS) void k_midwt_cols(const float* __restrict__ lo, const float* __restrict__ hi,
                                                             int64_t B, int64_t R, int64_t oW, Taps tp,
                                                             float* __restrict__ y, int64_t oH,
                                                             unsigned long long* zero_count) {
    const int64_t total = B * oH * oW;
    unsigned long long z = 0;
    for (int64_t idx = (int64_t)blockIdx.x * MDWT_THREADS + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * MDWT_THREADS) {
        const int64_t n = idx % oW, t = idx / oW, m = t % oH, b = t / oH;
        const float* lc = lo + b * R * oW + n;
        const float* hc = hi + b * R * oW + n;
        const float v = wtm_syn_point(m, tp.F, tp.f[2], tp.f[3], [&](int64_t k) { return lc[k * oW]; },
                                      [&](int64_t k) { return hc[k * oW]; });
        y[idx] = v;
        z += (v == 0.0f);
    }
    if (zero_count) {
        const unsigned long long tot = block_sum_u64<MDWT_THREADS>(z);
        if (threadIdx.x == 0 && tot) atomicAdd(zero_count, tot);
    }
}

/* ------------------------------------------------------------- tiny images --- */
/* A wave's arena (wt_tiny_arena.h) holds the areas A, T and D of its images (wt_modes_core.h,
 * where the per-image routines wtm_tiny_fwd / wtm_tiny_inv are).  The geometry is wave-uniform:
 * thread 0 puts it into LDS (the level loops index it; private arrays would go to scratch). */
__global__ __launch_bounds__(TINY_THREADS) void k_mtiny_fwd(MTinyTable t) {
    __shared__ float lds[WTM_WAVE_WORDS];
    __shared__ float ltap[4 * WTM_TINY_F_MAX];
    const TinyWave v = tiny_wave(t);
    tiny_stage_taps(ltap, WTM_TINY_F_MAX, WTM_TINY_F_MAX, [&](int k, int j) { return t.f[k][j]; });
    const MTinySeg& S = t.s[v.sg];
    const int H = S.H, W = S.W, L = S.L, NL = 1 << S.nl_log2, F = t.F, HW = H * W, mode = t.mode;
    __shared__ wtm_tiny_geom g;
    if (threadIdx.x == 0) wtm_tiny_geometry(H, W, L, F, g);
    __syncthreads();
    const int PP = g.PR * g.PC, lane = threadIdx.x;
    float* A = lds;
    float* T = A + wtm_tiny_area_a(H, W, L, F) * NL;
    float* D = T + wtm_tiny_area_t(H, W, L, F) * NL;
    tiny_load(A, NL, S.in + v.b0 * HW, v.nimg, HW, [](float x) { return x; });
    if (lane < NL)
        for (int s = 0; s < PP; ++s) D[s * NL + lane] = 0.0f;
    __syncthreads();
    if (lane < v.nimg) wtm_tiny_fwd(A + lane, T + lane, D + lane, NL, g, L, F, mode, ltap, ltap + WTM_TINY_F_MAX);
    __syncthreads();
    tiny_store(S.P + v.b0 * PP, D, NL, v.nimg, PP, [](float) {});
}

__global__ __launch_bounds__(TINY_THREADS) void k_mtiny_inv(MTinyTable t) {
    __shared__ float lds[WTM_WAVE_WORDS];
    __shared__ float ltap[4 * WTM_TINY_F_MAX];
    const TinyWave v = tiny_wave(t);
    tiny_stage_taps(ltap, WTM_TINY_F_MAX, WTM_TINY_F_MAX, [&](int k, int j) { return t.f[k][j]; });
    const MTinySeg& S = t.s[v.sg];
    const int H = S.H, W = S.W, L = S.L, NL = 1 << S.nl_log2, F = t.F, HW = H * W;
    __shared__ wtm_tiny_geom g;
    if (threadIdx.x == 0) wtm_tiny_geometry(H, W, L, F, g);
    __syncthreads();
    const int PP = g.PR * g.PC, lane = threadIdx.x;
    const float thr = S.thr ? *S.thr : 0.0f; /* |c| < 0 never holds: no threshold */
    float* A = lds;
    float* T = A + wtm_tiny_area_a(H, W, L, F) * NL;
    float* D = T + wtm_tiny_area_t(H, W, L, F) * NL;
    tiny_load(D, NL, S.P + v.b0 * PP, v.nimg, PP, [&](float c) { return wt_thr_mask(c, thr); });
    __syncthreads();
    if (lane < v.nimg)
        wtm_tiny_inv(A + lane, T + lane, D + lane, NL, g, L, F, ltap + 2 * WTM_TINY_F_MAX, ltap + 3 * WTM_TINY_F_MAX);
    __syncthreads();
    unsigned z = 0;
    tiny_store(S.out + v.b0 * HW, A, NL, v.nimg, HW, [&](float y) { z += (y == 0.0f); });
    z = wave_sum_u32(z);
    if (lane == 0 && z && S.zc) atomicAdd(S.zc, (unsigned long long)z);
}

/* ---------------------------------------------------------------- launchers --- */
static inline unsigned mgrid_for(int64_t total) {
    int64_t g = (total + MDWT_THREADS - 1) / MDWT_THREADS;
    if (g > 65536) g = 65536;
    if (g < 1) g = 1;
    return (unsigned)g;
}

void launch_mdwt_level(const float* in, int64_t B, int64_t R, int64_t C, int64_t Ro, int64_t Co, const Taps& tp,
                       int mode, float* tL, float* tH, float* anext, float* P, int64_t PR, int64_t PC, int64_t offR,
                       int64_t offC, int last, hipStream_t s) {
    hipLaunchKernelGGL(k_mdwt_cols, dim3(mgrid_for(B * Ro * C)), dim3(MDWT_THREADS), 0, s, in, B, R, C, Ro, tp, mode,
                       tL, tH);
    hipLaunchKernelGGL(k_mdwt_rows, dim3(mgrid_for(B * Ro * Co)), dim3(MDWT_THREADS), 0, s, tL, tH, B, Ro, C, Co, tp,
                       mode, anext, P, PR, PC, offR, offC, last);
}

void launch_midwt_level(const float* a, int a_from_P, const float* P, int64_t PR, int64_t PC, int64_t offR,
                        int64_t offC, int64_t B, int64_t R, int64_t C, const Taps& tp, const float* thr, float* tL,
                        float* tH, float* y, int64_t oH, int64_t oW, unsigned long long* zc, hipStream_t s) {
    hipLaunchKernelGGL(k_midwt_rows, dim3(mgrid_for(B * R * oW)), dim3(MDWT_THREADS), 0, s, a, a_from_P, P, PR, PC,
                       offR, offC, B, R, C, oW, tp, thr, tL, tH);
    hipLaunchKernelGGL(k_midwt_cols, dim3(mgrid_for(B * oH * oW)), dim3(MDWT_THREADS), 0, s, tL, tH, B, R, oW, tp, y,
                       oH, zc);
}

void launch_mtiny_fwd(const MTinyTable& t, hipStream_t s) {
    hipLaunchKernelGGL(k_mtiny_fwd, dim3((unsigned)t.nwave), dim3(TINY_THREADS), 0, s, t);
}
void launch_mtiny_inv(const MTinyTable& t, hipStream_t s) {
    hipLaunchKernelGGL(k_mtiny_inv, dim3((unsigned)t.nwave), dim3(TINY_THREADS), 0, s, t);
}

}  // namespace wtp

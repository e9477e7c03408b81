/*
 * modes.hip -- the filter bank under PyWavelets' signal-extension modes zero, constant,
 * symmetric, reflect and periodic (wtp_prune_mode_f32 and the mode component entries; the
 * arithmetic and the geometry are csrc/wt_modes_core.h, shared with the host-side check).
 *
 *   k_mtiny_fwd / k_mtiny_inv   tensors whose images are at most 8 x 8 (conv kernels): a wave per
 *                tensor slice, one image per lane in a sample-major LDS arena (k_abs_tiny's
 *                layout).  k_mtiny_fwd reads an image once, runs every analysis level on chip and
 *                stores the packed coefficient image, padding zeros included (the percentile's
 *                population); after the selection k_mtiny_inv reads the packed image once,
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

__device__ __forceinline__ float mthr_load(float c, float thr) { return (fabsf(c) < thr) ? 0.0f : c; }

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
            vlo = wtm_syn_point(n, tp.F, tp.f[2], tp.f[3], [&](int64_t k) { return mthr_load(arow[k], thr); },
                                [&](int64_t k) { return mthr_load(adr[k], thr); });
        else
            vlo = wtm_syn_point(n, tp.F, tp.f[2], tp.f[3], [&](int64_t k) { return arow[k]; },
                                [&](int64_t k) { return mthr_load(adr[k], thr); });
        const float vhi = wtm_syn_point(n, tp.F, tp.f[2], tp.f[3], [&](int64_t k) { return mthr_load(dar[k], thr); },
                                        [&](int64_t k) { return mthr_load(ddr[k], thr); });
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
/* The areas of a lane's image in the arena (wtm_tiny_areas): A the image / a level's
 * approximation / a level's synthesis output, T a level's two half transforms, D the packed
 * coefficient image (PR x PC, row pitch PC).  The geometry is wave-uniform, so every index below
 * is scalar arithmetic and every LDS access a uniform offset plus the lane. */
struct MTinyGeom {
    int R[MT_LMAX + 1], C[MT_LMAX + 1], offR[MT_LMAX + 1], offC[MT_LMAX + 1], PR, PC;
};
__device__ __forceinline__ void mtiny_geom(int H, int W, int L, int F, MTinyGeom& g) {
    g.R[0] = H;
    g.C[0] = W;
    for (int k = 1; k <= L; ++k) { g.R[k] = (g.R[k - 1] + F - 1) >> 1; g.C[k] = (g.C[k - 1] + F - 1) >> 1; }
    int aR = g.R[L], aC = g.C[L];
    for (int k = L; k >= 1; --k) { g.offR[k] = aR; g.offC[k] = aC; aR += g.R[k]; aC += g.C[k]; }
    g.PR = aR;
    g.PC = aC;
}

__device__ __forceinline__ void mtiny_setup(const MTinyTable& t, float* ltap, int& sg, int& w) {
    const int gw = blockIdx.x;
    sg = 0;
    for (int i = 1; i < t.nseg; ++i) sg += gw >= t.wave_begin[i];
    w = gw - t.wave_begin[sg];
    if (threadIdx.x < 4 * MT_F_MAX) ltap[threadIdx.x] = t.f[threadIdx.x / MT_F_MAX][threadIdx.x % MT_F_MAX];
}

__global__ __launch_bounds__(MT_THREADS) void k_mtiny_fwd(MTinyTable t) {
    __shared__ float lds[MT_WAVE_WORDS];
    __shared__ float ltap[4 * MT_F_MAX];
    int sg, w;
    mtiny_setup(t, ltap, sg, w);
    const MTinySeg& S = t.s[sg];
    const int H = S.H, W = S.W, L = S.L, NL = 1 << S.nl_log2, F = t.F, HW = H * W, mode = t.mode;
    __shared__ MTinyGeom g; /* LDS, not registers: the level loops index it (private arrays would go to scratch) */
    if (threadIdx.x == 0) mtiny_geom(H, W, L, F, g);
    __syncthreads();
    const int PP = g.PR * g.PC;
    const int64_t b0 = (int64_t)w * NL;
    const int nimg = (int)(S.B - b0 < NL ? S.B - b0 : NL);
    const int lane = threadIdx.x;
    float* A = lds;
    float* T = A + wtm_tiny_area_a(H, W, L, F) * NL;
    float* D = T + wtm_tiny_area_t(H, W, L, F) * NL;
    const float* in = S.in + b0 * HW;
    for (int e = lane; e < nimg * HW; e += MT_THREADS) {
        const int img = e / HW, s = e - img * HW;
        A[s * NL + img] = in[e];
    }
    if (lane < NL)
        for (int s = 0; s < PP; ++s) D[s * NL + lane] = 0.0f;
    __syncthreads();
    if (lane < nimg) {
        float* a = A + lane;
        float* tt = T + lane;
        float* dd = D + lane;
        const float *dlo = ltap, *dhi = ltap + MT_F_MAX;
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
                    if (last) dd[(r * g.PC + o) * NL] = aa;
                    else a[(r * C + o) * NL] = aa;
                    dd[(r * g.PC + g.offC[k] + o) * NL] = ad;
                    dd[((g.offR[k] + r) * g.PC + o) * NL] = da;
                    dd[((g.offR[k] + r) * g.PC + g.offC[k] + o) * NL] = d2;
                }
        }
    }
    __syncthreads();
    float* P = S.P + b0 * PP;
    for (int e = lane; e < nimg * PP; e += MT_THREADS) {
        const int img = e / PP, s = e - img * PP;
        P[e] = D[s * NL + img];
    }
}

__global__ __launch_bounds__(MT_THREADS) void k_mtiny_inv(MTinyTable t) {
    __shared__ float lds[MT_WAVE_WORDS];
    __shared__ float ltap[4 * MT_F_MAX];
    int sg, w;
    mtiny_setup(t, ltap, sg, w);
    const MTinySeg& S = t.s[sg];
    const int H = S.H, W = S.W, L = S.L, NL = 1 << S.nl_log2, F = t.F, HW = H * W;
    __shared__ MTinyGeom g; /* LDS, not registers: the level loops index it (private arrays would go to scratch) */
    if (threadIdx.x == 0) mtiny_geom(H, W, L, F, g);
    __syncthreads();
    const int PP = g.PR * g.PC;
    const int64_t b0 = (int64_t)w * NL;
    const int nimg = (int)(S.B - b0 < NL ? S.B - b0 : NL);
    const int lane = threadIdx.x;
    const float thr = S.thr ? *S.thr : 0.0f; /* |c| < 0 never holds: no threshold */
    float* A = lds;
    float* T = A + wtm_tiny_area_a(H, W, L, F) * NL;
    float* D = T + wtm_tiny_area_t(H, W, L, F) * NL;
    const float* P = S.P + b0 * PP;
    for (int e = lane; e < nimg * PP; e += MT_THREADS) {
        const int img = e / PP, s = e - img * PP;
        D[s * NL + img] = mthr_load(P[e], thr);
    }
    __syncthreads();
    if (lane < nimg) {
        float* a = A + lane;
        float* tt = T + lane;
        const float* dd = D + lane;
        const float *rlo = ltap + 2 * MT_F_MAX, *rhi = ltap + 3 * MT_F_MAX;
        for (int k = L; k >= 1; --k) {
            const int R = g.R[k], C = g.C[k], oH = g.R[k - 1], oW = g.C[k - 1];
            const float* ca = (k == L) ? dd : a;
            const int lda = (k == L) ? g.PC : C;
            const float* pad = dd + g.offC[k] * NL;
            const float* pda = dd + g.offR[k] * g.PC * NL;
            const float* pdd = dd + (g.offR[k] * g.PC + g.offC[k]) * NL;
            for (int r = 0; r < R; ++r)
                for (int n = 0; n < oW; ++n) {
                    tt[(r * oW + n) * NL] =
                        wtm_syn_point(n, F, rlo, rhi, [&](int64_t q) { return ca[(r * lda + (int)q) * NL]; },
                                      [&](int64_t q) { return pad[(r * g.PC + (int)q) * NL]; });
                    tt[((R + r) * oW + n) * NL] =
                        wtm_syn_point(n, F, rlo, rhi, [&](int64_t q) { return pda[(r * g.PC + (int)q) * NL]; },
                                      [&](int64_t q) { return pdd[(r * g.PC + (int)q) * NL]; });
                }
            for (int m = 0; m < oH; ++m)
                for (int n = 0; n < oW; ++n)
                    a[(m * oW + n) * NL] =
                        wtm_syn_point(m, F, rlo, rhi, [&](int64_t q) { return tt[((int)q * oW + n) * NL]; },
                                      [&](int64_t q) { return tt[((R + (int)q) * oW + n) * NL]; });
        }
    }
    __syncthreads();
    float* out = S.out + b0 * HW;
    unsigned z = 0;
    for (int e = lane; e < nimg * HW; e += MT_THREADS) {
        const int img = e / HW, s = e - img * HW;
        const float v = A[s * NL + img];
        out[e] = v;
        z += (v == 0.0f);
    }
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
    hipLaunchKernelGGL(k_mtiny_fwd, dim3((unsigned)t.nwave), dim3(MT_THREADS), 0, s, t);
}
void launch_mtiny_inv(const MTinyTable& t, hipStream_t s) {
    hipLaunchKernelGGL(k_mtiny_inv, dim3((unsigned)t.nwave), dim3(MT_THREADS), 0, s, t);
}

}  // namespace wtp

/*
 * abs.hip -- device side of the absolute-threshold method (ResNet/dwt_pruning_NoEntropy.py:29-60,
 * wtp_prune_abs_f32): the threshold is a given number, so nothing is selected and a tensor is one
 * streaming pass.
 *
 *   k_abs_tiny   every tensor of the call whose images are at most 8 x 8 (conv kernels), in one
 *                launch: an image is read once, all levels forward, the mask, all levels inverse
 *                and the crop run in LDS, and it is written once (8 B of HBM per weight).
 *   k_abs_tiny_sweep  k_abs_tiny for up to eight thresholds (wtp_prune_abs_sweep_f32): an image is
 *                read once and taken forward once, its raw coefficients stay in LDS, and every
 *                threshold's masked inverse runs over them and writes that threshold's output.
 *   k_abs_init, k_abs_count_in, k_abs_count, k_abs_zero  the cold kernels both entries share
 *                (the ordinary call is a sweep of one threshold to them): the records' zero fill
 *                and the threshold words, count_nonzero of an input with its records' fixed
 *                fields, count_nonzero of an output, a packed array's zero padding.
 *
 * k_abs_tiny gives a whole wave to one tensor, one image per lane, in a sample-major LDS layout
 * (word s of an image at lds[s * NL + lane]): (H, W, level, F) are wave-uniform, so the wrapped
 * sample index of every (output, tap) is scalar arithmetic and every LDS access is a uniform
 * offset plus the lane.  Lines here are shorter than the filter (a 3 x 3 kernel under an 8-tap
 * bior3.3 at level 5 ends in four 1 -> 1 levels): every tap is still multiplied and added on its
 * own, in wt_dwt_core.h's order (wt_abs_core.h: abs_image, shared with the host-side check).
 */
#include "wtp_internal.h"
#include "wt_abs_sweep_core.h"

#pragma clang fp contract(off)

namespace wtp {

/* torch.count_nonzero's test on the bit pattern (a denormal is non-zero whatever the FP mode) */
__device__ __forceinline__ unsigned abs_nonzero(float v) { return (__float_as_uint(v) << 1) != 0u; }

__device__ __forceinline__ unsigned abs_wave_sum(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(TINY_THREADS) void k_abs_tiny(AbsTable t, wtp_abs_result* __restrict__ res) {
    __shared__ float lds[ABS_WAVE_WORDS];
    /* the four filters beside the arena: a tap is a broadcast LDS read that returns in order with
     * the sample reads, so an unrolled tap loop keeps several reads in flight (a scalar load per
     * tap from the kernel argument returns out of order: every tap then waits for all of them) */
    __shared__ float ltap[ABS_TAP_WORDS];
    const int gw = blockIdx.x;
    int sg = 0;
    for (int i = 1; i < t.nseg; ++i) sg += gw >= t.wave_begin[i];
    const AbsSeg& S = t.s[sg];
    const int H = S.H, W = S.W, L = S.L, NL = 1 << S.nl_log2, F = t.tp.F, HW = H * W;
    const int w = gw - t.wave_begin[sg];
    const int64_t b0 = (int64_t)w * NL;
    const int nimg = (int)(S.B - b0 < NL ? S.B - b0 : NL);
    const float thr = __uint_as_float(t.thr_bits);
    const float* in = S.in + b0 * HW; /* may alias out: the wave reads all of its range before it writes */
    float* out = S.out + b0 * HW;
    const int lane = threadIdx.x;
    const int total = nimg * HW;

    /* areas (wt_abs_core.h): A the image / a level's approximation, T a level's two half
     * transforms, D the masked coefficients */
    float* A = lds;
    float* T = A + abs_area_a(H, W, L) * NL;
    float* D = T + abs_area_t(H, W, L) * NL;

    const int FP = ABS_TAP_WORDS / 4;
    for (int e = threadIdx.x; e < 4 * F; e += TINY_THREADS) {
        const int k = e / F, j = e - k * F;
        ltap[k * FP + j] = t.tp.f[k][j];
    }
    /* coalesced read of the wave's images into the sample-major layout */
    unsigned z_in = 0, z_out = 0;
    for (int e = lane; e < total; e += TINY_THREADS) {
        const float v = in[e];
        const int img = e / HW, s = e - img * HW;
        A[s * NL + img] = v;
        z_in += !abs_nonzero(v);
    }
    __syncthreads();

    if (lane < nimg)
        abs_image(A + lane, T + lane, D + lane, NL, H, W, L, F, ltap, ltap + FP, ltap + 2 * FP, ltap + 3 * FP, thr);
    __syncthreads();

    for (int e = lane; e < total; e += TINY_THREADS) {
        const int img = e / HW, s = e - img * HW;
        const float v = A[s * NL + img];
        out[e] = v;
        z_out += !abs_nonzero(v);
    }
    /* the counts as numel minus the zeros: the tensor's first wave adds numel, every wave takes
     * off the zeros it saw -- usually none, so a tensor costs two atomics, not two per wave (the
     * ResNet-18 list: 39 000 adds on 40 addresses, 28 us of a 583 us launch) */
    z_in = abs_wave_sum(z_in);
    z_out = abs_wave_sum(z_out);
    if (lane == 0) {
        wtp_abs_result* r = res + S.res;
        if (z_in) atomicAdd((unsigned long long*)&r->nonzero_in, 0ull - (unsigned long long)z_in);
        if (z_out) atomicAdd((unsigned long long*)&r->nonzero_out, 0ull - (unsigned long long)z_out);
        if (w == 0) { /* ... and the record's fixed fields (the record starts from the call's zero fill) */
            atomicAdd((unsigned long long*)&r->nonzero_in, (unsigned long long)S.B * HW);
            atomicAdd((unsigned long long*)&r->nonzero_out, (unsigned long long)S.B * HW);
            int PR = H, PC = W; /* wt_geom's packed size */
            if (L) {
                int R = H, C = W;
                PR = PC = 0;
                for (int k = 1; k <= L; ++k) {
                    R = (R + 1) >> 1;
                    C = (C + 1) >> 1;
                    PR += R;
                    PC += C;
                }
                PR += R;
                PC += C;
            }
            r->numel = (int64_t)S.B * HW;
            r->coeff_numel = (int64_t)S.B * PR * PC;
            r->thr32_bits = t.thr_bits;
            r->level = L;
            r->path = WTP_ABS_PATH_TINY;
            r->reserved = 0;
        }
    }
}

/* a thread's share of count_nonzero(x) (-0.0 is zero, NaN is non-zero), summed over its wave */
__device__ __forceinline__ unsigned abs_count_wave(const float* __restrict__ x, int64_t n) {
    unsigned c = 0;
    for (int64_t i = (int64_t)blockIdx.x * ABS_COUNT_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * ABS_COUNT_THREADS)
        c += abs_nonzero(x[i]);
    return abs_wave_sum(c);
}

/* count_nonzero(x) added to *dst: one atomic per wave (an output's count) */
__global__ __launch_bounds__(ABS_COUNT_THREADS) void k_abs_count(const float* __restrict__ x, int64_t n,
                                                                 unsigned long long* __restrict__ dst) {
    const unsigned c = abs_count_wave(x, n);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(dst, (unsigned long long)c);
}

/* count_nonzero of a chain or mask tensor's input: counted once, added to nonzero_in of the
 * tensor's thr.n records (rec, rec + stride, ...), each of which also gets its fixed fields
 * (init's, with its own threshold) */
__global__ __launch_bounds__(ABS_COUNT_THREADS) void k_abs_count_in(const float* __restrict__ x, int64_t n,
                                                                    wtp_abs_result* __restrict__ rec, int64_t stride,
                                                                    AbsThr thr, wtp_abs_result init) {
    const unsigned c = abs_count_wave(x, n);
    if ((threadIdx.x & 63) == 0 && c)
        for (int k = 0; k < thr.n; ++k)
            atomicAdd((unsigned long long*)&rec[k * stride].nonzero_in, (unsigned long long)c);
    if (blockIdx.x == 0 && threadIdx.x < thr.n) {
        wtp_abs_result* r = rec + threadIdx.x * stride;
        r->numel = init.numel;
        r->coeff_numel = init.coeff_numel;
        r->thr32_bits = thr.bits[threadIdx.x];
        r->level = init.level;
        r->path = init.path;
        r->reserved = 0;
    }
}

/* The call's first launch: every record zero (the counts are accumulated; an empty tensor's
 * record stays zero) and the float32 thresholds in their workspace words for the kernels that
 * read them from memory.  A kernel, not hipMemsetAsync: with a memset node in its place the
 * records were not zero when a captured graph of the call replayed (eager calls were right); the
 * cause was not established. */
__global__ __launch_bounds__(ABS_COUNT_THREADS) void k_abs_init(uint32_t* __restrict__ rec_words, int64_t nwords,
                                                                uint32_t* __restrict__ thr_words, AbsThr thr) {
    for (int64_t i = (int64_t)blockIdx.x * ABS_COUNT_THREADS + threadIdx.x; i < nwords;
         i += (int64_t)gridDim.x * ABS_COUNT_THREADS)
        rec_words[i] = 0u;
    if (thr_words && blockIdx.x == 0 && threadIdx.x < thr.n) thr_words[threadIdx.x] = thr.bits[threadIdx.x];
}

/* zero padding of a packed array that is not tight (pywt.coeffs_to_array) */
__global__ __launch_bounds__(ABS_COUNT_THREADS) void k_abs_zero(float* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * ABS_COUNT_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * ABS_COUNT_THREADS)
        p[i] = 0.0f;
}

/* k_abs_tiny's scheme (one wave per workgroup, one image per lane, sample-major LDS, the filters
 * in LDS, abs_lanes_log2's lanes) with the per-image routine cut at its mask (wt_abs_sweep_core.h):
 * the forward leaves the raw coefficients in D, which no inverse writes, so the wave reads its
 * images and runs the forward once for all thresholds.  Level 0 has no D: the image stays in A
 * and each store pass masks it. */
/* the fixed fields of a tiny tensor's record and numel on both counts (the record starts from the
 * call's zero fill; every wave takes off the zeros it saw): its first wave's lane 0 */
__device__ __forceinline__ void abs_tiny_record(wtp_abs_result* r, int64_t B, int H, int W, int L, uint32_t thr_bits) {
    int PR, PC;
    tiny_packed_size(H, W, L, 2, PR, PC); /* wt_geom's */
    atomicAdd((unsigned long long*)&r->nonzero_in, (unsigned long long)B * (H * W));
    atomicAdd((unsigned long long*)&r->nonzero_out, (unsigned long long)B * (H * W));
    r->numel = B * (H * W);
    r->coeff_numel = B * PR * PC;
    r->thr32_bits = thr_bits;
    r->level = L;
    r->path = WTP_ABS_PATH_TINY;
    r->reserved = 0;
}

__global__ __launch_bounds__(TINY_THREADS) void k_abs_tiny_sweep(AbsSweepTable t, wtp_abs_result* __restrict__ res) {
    __shared__ float lds[ABS_WAVE_WORDS];
    __shared__ float ltap[ABS_TAP_WORDS];
    const TinyWave v = tiny_wave(t);
    const AbsSweepSeg& S = t.s[v.sg];
    const int H = S.H, W = S.W, L = S.L, NL = 1 << S.nl_log2, F = t.tp.F, HW = H * W;
    const int lane = threadIdx.x;

    float* A = lds;
    float* T = A + abs_area_a(H, W, L) * NL;
    float* D = T + abs_area_t(H, W, L) * NL;

    const int FP = ABS_TAP_WORDS / 4;
    tiny_stage_taps(ltap, FP, F, [&](int k, int j) { return t.tp.f[k][j]; });
    /* the input may alias ONE of the outputs: the wave reads all of its range before it writes */
    unsigned z_in = 0;
    tiny_load(A, NL, S.in + v.b0 * HW, v.nimg, HW, [&](float x) {
        z_in += !abs_nonzero(x);
        return x;
    });
    __syncthreads();
    if (lane < v.nimg) abs_forward_raw(A + lane, T + lane, D + lane, NL, H, W, L, F, ltap, ltap + FP);
    z_in = abs_wave_sum(z_in);

    wtp_abs_result* r = res + S.res;
    for (int k = 0; k < t.thr.n; ++k, r += t.ntensors) {
        const float thr = __uint_as_float(t.thr.bits[k]);
        if (lane < v.nimg)
            abs_inverse_masked(A + lane, T + lane, D + lane, NL, H, W, L, F, ltap + 2 * FP, ltap + 3 * FP, thr);
        __syncthreads(); /* the store reads other lanes' words */
        float* out = S.out[k] + v.b0 * HW;
        unsigned z_out = 0;
        /* tiny_store with level 0's mask on the way out */
        for (int e = lane; e < v.nimg * HW; e += TINY_THREADS) {
            const int img = e / HW, s = e - img * HW;
            float y = A[s * NL + img];
            if (L == 0) y = wt_thr_mask(y, thr);
            out[e] = y;
            z_out += !abs_nonzero(y);
        }
        __syncthreads(); /* the next inverse overwrites A and T */
        /* k_abs_tiny's counts, numel minus the zeros seen, into this threshold's record */
        z_out = abs_wave_sum(z_out);
        if (lane == 0) {
            if (z_in) atomicAdd((unsigned long long*)&r->nonzero_in, 0ull - (unsigned long long)z_in);
            if (z_out) atomicAdd((unsigned long long*)&r->nonzero_out, 0ull - (unsigned long long)z_out);
            if (v.w == 0) abs_tiny_record(r, S.B, H, W, L, t.thr.bits[k]);
        }
    }
}

static unsigned abs_grid(int64_t n, int per_thread) {
    int64_t blocks = (n + (int64_t)ABS_COUNT_THREADS * per_thread - 1) / ((int64_t)ABS_COUNT_THREADS * per_thread);
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    return (unsigned)blocks;
}

void launch_abs_init(wtp_abs_result* res, int n, float* thr_words, const AbsThr& thr, hipStream_t s) {
    const int64_t nwords = (int64_t)n * (int64_t)(sizeof(wtp_abs_result) / 4);
    hipLaunchKernelGGL(k_abs_init, dim3(abs_grid(nwords, 4)), dim3(ABS_COUNT_THREADS), 0, s,
                       reinterpret_cast<uint32_t*>(res), nwords, reinterpret_cast<uint32_t*>(thr_words), thr);
}

void launch_abs_zero(float* p, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_abs_zero, dim3(abs_grid(n, 16)), dim3(ABS_COUNT_THREADS), 0, s, p, n);
}

void launch_abs_tiny(const AbsTable& t, wtp_abs_result* res, hipStream_t s) {
    hipLaunchKernelGGL(k_abs_tiny, dim3((unsigned)t.nwave), dim3(TINY_THREADS), 0, s, t, res);
}

void launch_abs_tiny(const AbsSweepTable& t, wtp_abs_result* res, hipStream_t s) {
    hipLaunchKernelGGL(k_abs_tiny_sweep, dim3((unsigned)t.nwave), dim3(TINY_THREADS), 0, s, t, res);
}

/* a thread takes at most 2^31 elements: the per-thread count stays in 32 bits */
void launch_abs_count(const float* x, int64_t n, unsigned long long* dst, hipStream_t s) {
    hipLaunchKernelGGL(k_abs_count, dim3(abs_grid(n, 16)), dim3(ABS_COUNT_THREADS), 0, s, x, n, dst);
}

void launch_abs_count_in(const float* x, int64_t n, wtp_abs_result* rec, int64_t stride, const AbsThr& thr,
                         const wtp_abs_result& init, hipStream_t s) {
    hipLaunchKernelGGL(k_abs_count_in, dim3(abs_grid(n, 16)), dim3(ABS_COUNT_THREADS), 0, s, x, n, rec, stride, thr, init);
}

}  // namespace wtp

/*
 * half.hip -- the kernels of the float16 path (wtp_prune_f16; the arithmetic is wt_half_core.h,
 * shared with tests/native/halfcore.cpp).  A translation unit of its own: nothing here is shared
 * with prune_unit.hip, whose k_resident moves with what it is compiled beside.
 *
 * Kind B (no transform: ndim < 2, or level 0 after the clamp) stays in float16 as NumPy keeps it.
 * |w| has 2^15 possible keys, so the percentile's order statistics come from histograms alone --
 * no sample, no window, no fallback:
 *   k_h16_hist1   the top 11 bits of every key, an LDS histogram per block added to the tensor's
 *   k_h16_scan1   per tensor: the top digits of rank lo, rank hi and rank n - 1 (the maximum)
 *   k_h16_hist2   the low 4 bits of the keys under each of those three top digits
 *   k_h16_scan2   per tensor: the three keys, the threshold by NumPy's float16 rule, the record
 *   k_h16_mask    out = key(w) < key(half(thr64)) ? +0 : w, and the zero count
 * Kind A (transformed) runs the float32 path between k_h16_widen and k_h16_narrow.
 *
 * Every kernel takes a table of up to H16_PER_LAUNCH tensors as its argument and maps blocks to
 * tensors by blk_begin.  A tensor is walked as h16_split cuts it: 16-byte vectors of 8 words
 * between a scalar head and tail (a tensor may start on any 2-byte boundary and numel may be odd);
 * block 0 of a tensor takes the head and the tail.  Where the other buffer of a kernel does not
 * share the input's phase the vectors' words go one by one.
 */
#include "wtp_half.h"

namespace wtp {

namespace {

__device__ __forceinline__ int seg_of_block(const H16Table& t, int b) {
    int i = 0;
    while (i + 1 < t.nseg && t.blk_begin[i + 1] <= b) ++i;
    return i;
}

/* The words of segment block `lb`: fv(v) for each of its vectors when `vec`, else fs(i) for their
 * words; fs(i) for the head and tail words in block 0. */
template <class FV, class FS>
__device__ __forceinline__ void walk(const h16_span& sp, int64_t n, int lb, bool vec, FV fv, FS fs) {
    const int64_t v0 = (int64_t)lb * H16_VPB, v1 = v0 + H16_VPB < sp.nvec ? v0 + H16_VPB : sp.nvec;
    if (vec) {
        for (int64_t v = v0 + threadIdx.x; v < v1; v += H16_THREADS) fv(v);
    } else {
        for (int64_t i = sp.head + 8 * v0 + threadIdx.x; i < sp.head + 8 * v1; i += H16_THREADS) fs(i);
    }
    if (lb == 0) {
        if ((int64_t)threadIdx.x < sp.head) fs((int64_t)threadIdx.x);
        const int64_t i = sp.tail + threadIdx.x;
        if (threadIdx.x < 8 && i < n) fs(i);
    }
}

__device__ __forceinline__ void words_of(const uint4& q, uint16_t w[8]) {
    w[0] = (uint16_t)q.x; w[1] = (uint16_t)(q.x >> 16);
    w[2] = (uint16_t)q.y; w[3] = (uint16_t)(q.y >> 16);
    w[4] = (uint16_t)q.z; w[5] = (uint16_t)(q.z >> 16);
    w[6] = (uint16_t)q.w; w[7] = (uint16_t)(q.w >> 16);
}
__device__ __forceinline__ uint4 vec_of(const uint16_t w[8]) {
    return make_uint4((uint32_t)w[0] | ((uint32_t)w[1] << 16), (uint32_t)w[2] | ((uint32_t)w[3] << 16),
                      (uint32_t)w[4] | ((uint32_t)w[5] << 16), (uint32_t)w[6] | ((uint32_t)w[7] << 16));
}

/* the block's sum of `c`, in thread 0 */
__device__ __forceinline__ unsigned block_sum(unsigned c, unsigned* red) {
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    unsigned tot = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < H16_THREADS / 64; ++k) tot += red[k];
    return tot;
}

__global__ void k_h16_init(uint32_t* a, int64_t words, uint32_t* res, int64_t res_words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) a[i] = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < res_words; i += stride) res[i] = 0u;
}

__global__ __launch_bounds__(H16_THREADS) void k_h16_hist1(const H16Table t, H16Ws w) {
    __shared__ uint32_t h[H16_BINS1];
    const int si = seg_of_block(t, blockIdx.x);
    const H16Seg& sg = t.s[si];
    const int lb = blockIdx.x - t.blk_begin[si];
    for (int i = threadIdx.x; i < H16_BINS1; i += H16_THREADS) h[i] = 0u;
    __syncthreads();
    const h16_span sp = h16_split((uint64_t)(uintptr_t)sg.in, sg.n);
    const uint4* vin = reinterpret_cast<const uint4*>(sg.in + sp.head);
    walk(sp, sg.n, lb, true,
         [&](int64_t v) {
             uint16_t x[8];
             words_of(vin[v], x);
#pragma unroll
             for (int k = 0; k < 8; ++k) atomicAdd(&h[h16_digit1(h16_key(x[k]))], 1u);
         },
         [&](int64_t i) { atomicAdd(&h[h16_digit1(h16_key(sg.in[i]))], 1u); });
    __syncthreads();
    uint32_t* g = w.hist1 + (size_t)sg.sub * H16_BINS1;
    for (int i = threadIdx.x; i < H16_BINS1; i += H16_THREADS)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

/* one block per tensor */
__global__ __launch_bounds__(H16_THREADS) void k_h16_scan1(const H16Table t, H16Ws w) {
    constexpr int PER = H16_BINS1 / H16_THREADS;
    static_assert(PER >= 1 && PER * H16_THREADS == H16_BINS1, "a whole number of top-digit bins per thread");
    __shared__ uint32_t h[H16_BINS1];
    __shared__ uint32_t part[2][H16_THREADS];
    const H16Seg& sg = t.s[blockIdx.x];
    const uint32_t* g = w.hist1 + (size_t)sg.sub * H16_BINS1;
    uint32_t sum = 0;
    for (int k = 0; k < PER; ++k) {
        const uint32_t c = g[threadIdx.x * PER + k];
        h[threadIdx.x * PER + k] = c;
        sum += c;
    }
    part[0][threadIdx.x] = sum;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < H16_THREADS; off <<= 1) {
        uint32_t v = part[cur][threadIdx.x];
        if ((int)threadIdx.x >= off) v += part[cur][threadIdx.x - off];
        part[cur ^ 1][threadIdx.x] = v;
        cur ^= 1;
        __syncthreads();
    }
    if (threadIdx.x < H16_NRANK) {
        const int j = threadIdx.x;
        const int64_t r = j == 0 ? sg.r0 : (j == 1 ? (sg.above ? sg.r0 : sg.r0 + 1) : sg.n - 1);
        uint32_t resid;
        const int d = h16_locate_grouped(h, part[cur], H16_BINS1, PER, (uint32_t)r, &resid);
        H16State& st = w.st[sg.sub];
        st.d1[j] = (uint32_t)d;
        st.resid[j] = resid;
    }
}

__global__ __launch_bounds__(H16_THREADS) void k_h16_hist2(const H16Table t, H16Ws w) {
    __shared__ uint32_t h[H16_NRANK * H16_BINS2];
    const int si = seg_of_block(t, blockIdx.x);
    const H16Seg& sg = t.s[si];
    const int lb = blockIdx.x - t.blk_begin[si];
    for (int i = threadIdx.x; i < H16_NRANK * H16_BINS2; i += H16_THREADS) h[i] = 0u;
    __syncthreads();
    const H16State& st = w.st[sg.sub];
    const uint32_t p0 = st.d1[0], p1 = st.d1[1], p2 = st.d1[2];
    auto add = [&](uint16_t x) {
        const uint32_t key = h16_key(x), d1 = h16_digit1(key), d2 = h16_digit2(key);
        if (d1 == p0) atomicAdd(&h[d2], 1u);
        if (d1 == p1) atomicAdd(&h[H16_BINS2 + d2], 1u);
        if (d1 == p2) atomicAdd(&h[2 * H16_BINS2 + d2], 1u);
    };
    const h16_span sp = h16_split((uint64_t)(uintptr_t)sg.in, sg.n);
    const uint4* vin = reinterpret_cast<const uint4*>(sg.in + sp.head);
    walk(sp, sg.n, lb, true,
         [&](int64_t v) {
             uint16_t x[8];
             words_of(vin[v], x);
#pragma unroll
             for (int k = 0; k < 8; ++k) add(x[k]);
         },
         [&](int64_t i) { add(sg.in[i]); });
    __syncthreads();
    uint32_t* g = w.hist2 + (size_t)sg.sub * (H16_NRANK * H16_BINS2);
    for (int i = threadIdx.x; i < H16_NRANK * H16_BINS2; i += H16_THREADS)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

/* one thread per tensor */
__global__ void k_h16_scan2(const H16Table t, H16Ws w, wtp_result* res) {
    const int si = threadIdx.x;
    if (si >= t.nseg) return;
    const H16Seg& sg = t.s[si];
    H16State& st = w.st[sg.sub];
    const uint32_t* g = w.hist2 + (size_t)sg.sub * (H16_NRANK * H16_BINS2);
    uint32_t key[H16_NRANK];
    for (int j = 0; j < H16_NRANK; ++j) {
        uint32_t resid;
        const int d2 = h16_locate(g + j * H16_BINS2, H16_BINS2, st.resid[j], &resid);
        key[j] = h16_join(st.d1[j], (uint32_t)d2);
    }
    double thr64;
    const uint32_t ckey = h16_threshold(key[0], key[1], key[2], sg.gamma, sg.above, &thr64);
    st.ckey = ckey;
    wtp_result& r = res[sg.res]; /* zero_count: zeroed by k_h16_init, counted by k_h16_mask */
    r.numel = sg.n;
    r.coeff_numel = sg.n;
    r.thr64 = thr64;
    r.thr32_bits = h16_to_float_bits(h16_from_double(thr64));
    r.max_abs_bits = h16_to_float_bits((uint16_t)key[2]);
    r.eff_level = sg.eff_level;
    r.path = WTP_PATH_HALF;
}

__global__ __launch_bounds__(H16_THREADS) void k_h16_mask(const H16Table t, H16Ws w, wtp_result* res) {
    __shared__ unsigned red[H16_THREADS / 64];
    const int si = seg_of_block(t, blockIdx.x);
    const H16Seg& sg = t.s[si];
    const int lb = blockIdx.x - t.blk_begin[si];
    const uint32_t ckey = w.st[sg.sub].ckey;
    const h16_span sp = h16_split((uint64_t)(uintptr_t)sg.in, sg.n);
    const bool vec = (((uintptr_t)sg.in ^ (uintptr_t)sg.out) & 15) == 0;
    const uint4* vin = reinterpret_cast<const uint4*>(sg.in + sp.head);
    uint4* vout = reinterpret_cast<uint4*>(sg.out + sp.head);
    unsigned zeros = 0;
    walk(sp, sg.n, lb, vec,
         [&](int64_t v) {
             uint16_t x[8];
             words_of(vin[v], x);
#pragma unroll
             for (int k = 0; k < 8; ++k) {
                 x[k] = h16_mask(x[k], ckey);
                 zeros += h16_is_zero(x[k]);
             }
             vout[v] = vec_of(x);
         },
         [&](int64_t i) {
             const uint16_t y = h16_mask(sg.in[i], ckey);
             zeros += h16_is_zero(y);
             sg.out[i] = y;
         });
    const unsigned tot = block_sum(zeros, red);
    if (threadIdx.x == 0 && tot)
        atomicAdd(reinterpret_cast<unsigned long long*>(&res[sg.res].zero_count), (unsigned long long)tot);
}

__global__ __launch_bounds__(H16_THREADS) void k_h16_widen(const H16Table t) {
    const int si = seg_of_block(t, blockIdx.x);
    const H16Seg& sg = t.s[si];
    const int lb = blockIdx.x - t.blk_begin[si];
    const h16_span sp = h16_split((uint64_t)(uintptr_t)sg.in, sg.n);
    /* the staging is 16-byte aligned at word 0: its float4 line up with the vectors when head is 0 or 4 */
    const bool vec = (sp.head & 3) == 0;
    const uint4* vin = reinterpret_cast<const uint4*>(sg.in + sp.head);
    float4* vst = reinterpret_cast<float4*>(sg.stage + sp.head);
    walk(sp, sg.n, lb, vec,
         [&](int64_t v) {
             uint16_t x[8];
             words_of(vin[v], x);
             vst[2 * v] = make_float4(h16_to_float(x[0]), h16_to_float(x[1]), h16_to_float(x[2]), h16_to_float(x[3]));
             vst[2 * v + 1] = make_float4(h16_to_float(x[4]), h16_to_float(x[5]), h16_to_float(x[6]), h16_to_float(x[7]));
         },
         [&](int64_t i) { sg.stage[i] = h16_to_float(sg.in[i]); });
}

__global__ __launch_bounds__(H16_THREADS) void k_h16_narrow(const H16Table t, const wtp_result* sub, wtp_result* res) {
    __shared__ unsigned red[H16_THREADS / 64];
    const int si = seg_of_block(t, blockIdx.x);
    const H16Seg& sg = t.s[si];
    const int lb = blockIdx.x - t.blk_begin[si];
    const h16_span sp = h16_split((uint64_t)(uintptr_t)sg.out, sg.n);
    const bool vec = (sp.head & 3) == 0;
    const float4* vst = reinterpret_cast<const float4*>(sg.stage + sp.head);
    uint4* vout = reinterpret_cast<uint4*>(sg.out + sp.head);
    unsigned zeros = 0;
    walk(sp, sg.n, lb, vec,
         [&](int64_t v) {
             const float4 a = vst[2 * v], b = vst[2 * v + 1];
             const uint16_t x[8] = {h16_from_float(a.x), h16_from_float(a.y), h16_from_float(a.z), h16_from_float(a.w),
                                    h16_from_float(b.x), h16_from_float(b.y), h16_from_float(b.z), h16_from_float(b.w)};
#pragma unroll
             for (int k = 0; k < 8; ++k) zeros += h16_is_zero(x[k]);
             vout[v] = vec_of(x);
         },
         [&](int64_t i) {
             const uint16_t y = h16_from_float(sg.stage[i]);
             zeros += h16_is_zero(y);
             sg.out[i] = y;
         });
    const unsigned tot = block_sum(zeros, red);
    if (threadIdx.x == 0) {
        wtp_result& r = res[sg.res];
        if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(&r.zero_count), (unsigned long long)tot);
        if (lb == 0) { /* the inner call's record; zero_count is the count after the narrowing */
            const wtp_result& q = sub[sg.sub];
            r.numel = q.numel;
            r.coeff_numel = q.coeff_numel;
            r.thr64 = q.thr64;
            r.thr32_bits = q.thr32_bits;
            r.max_abs_bits = q.max_abs_bits;
            r.eff_level = q.eff_level;
            r.path = q.path;
        }
    }
}

}  // namespace

void launch_h16_init(uint32_t* a, int64_t words, wtp_result* res, int nres, hipStream_t s) {
    const int64_t rw = (int64_t)nres * (int64_t)(sizeof(wtp_result) / 4);
    const int64_t most = words > rw ? words : rw;
    const int blocks = (int)((most + 4095) / 4096 < 1024 ? (most + 4095) / 4096 : 1024);
    hipLaunchKernelGGL(k_h16_init, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, s, a, words,
                       reinterpret_cast<uint32_t*>(res), rw);
}
void launch_h16_hist1(const H16Table& t, H16Ws w, hipStream_t s) {
    hipLaunchKernelGGL(k_h16_hist1, dim3(t.nblk), dim3(H16_THREADS), 0, s, t, w);
}
void launch_h16_scan1(const H16Table& t, H16Ws w, hipStream_t s) {
    hipLaunchKernelGGL(k_h16_scan1, dim3(t.nseg), dim3(H16_THREADS), 0, s, t, w);
}
void launch_h16_hist2(const H16Table& t, H16Ws w, hipStream_t s) {
    hipLaunchKernelGGL(k_h16_hist2, dim3(t.nblk), dim3(H16_THREADS), 0, s, t, w);
}
void launch_h16_scan2(const H16Table& t, H16Ws w, wtp_result* res, hipStream_t s) {
    hipLaunchKernelGGL(k_h16_scan2, dim3(1), dim3(64), 0, s, t, w, res);
}
void launch_h16_mask(const H16Table& t, H16Ws w, wtp_result* res, hipStream_t s) {
    hipLaunchKernelGGL(k_h16_mask, dim3(t.nblk), dim3(H16_THREADS), 0, s, t, w, res);
}
void launch_h16_widen(const H16Table& t, hipStream_t s) {
    hipLaunchKernelGGL(k_h16_widen, dim3(t.nblk), dim3(H16_THREADS), 0, s, t);
}
void launch_h16_narrow(const H16Table& t, const wtp_result* sub, wtp_result* res, hipStream_t s) {
    hipLaunchKernelGGL(k_h16_narrow, dim3(t.nblk), dim3(H16_THREADS), 0, s, t, sub, res);
}

}  // namespace wtp

/*
 * randprune.inc -- the random-pruning kernels (k_rand_copy, k_rand_zero) and their launcher.
 */
#include "wtp_device.h"
#include "wt_perm.h"

#pragma clang fp contract(off)

namespace wtp {

/* ------------------------------------------------------ random pruning --- */
/* random_pruning (ResNet/random_pruning.py:49-56): out = in with k distinct flat positions
 * zeroed -- perm(0..k-1) of the keyed permutation in wt_perm.h; zero_count = zeros(in) + the
 * chosen positions that held a non-zero (count_nonzero counts NaN as non-zero).
 *   k_rand_copy  out = in (unless in place), zeros(in) per block, the record's numel
 *   k_rand_zero  one thread per chosen position; block sums of the non-zeros it removed */
__device__ __forceinline__ int rand_seg(const int32_t* begin, int nseg, int b) {
    int s = 0;
    for (int i = 1; i < nseg; ++i) s += b >= begin[i];
    return s;
}

__global__ __launch_bounds__(STREAM_THREADS) void k_rand_copy(RandTable t, wtp_result* __restrict__ res) {
    const int si = rand_seg(t.copy_begin, t.nseg, blockIdx.x);
    const RandSeg& sg = t.s[si];
    const int64_t base = (int64_t)(blockIdx.x - t.copy_begin[si]) * CHUNK;
    const int64_t end = min(sg.numel, base + CHUNK);
    uint32_t z = 0;
    for (int64_t i = base + threadIdx.x; i < end; i += STREAM_THREADS) {
        const float v = sg.in[i];
        z += v == 0.0f;
        if (sg.out != sg.in) sg.out[i] = v;
    }
    const unsigned long long tot = block_sum_u64<STREAM_THREADS>(z);
    if (threadIdx.x == 0) {
        if (tot) atomicAdd((unsigned long long*)&res[sg.res].zero_count, tot);
        if (base == 0) res[sg.res].numel = sg.numel;
    }
}

__global__ __launch_bounds__(STREAM_THREADS) void k_rand_zero(RandTable t, wtp_result* __restrict__ res) {
    const int si = rand_seg(t.zero_begin, t.nseg, blockIdx.x);
    const RandSeg& sg = t.s[si];
    const int64_t j = (int64_t)(blockIdx.x - t.zero_begin[si]) * STREAM_THREADS + threadIdx.x;
    uint32_t hit = 0;
    if (j < sg.k) {
        const int64_t idx = (int64_t)wt_perm((uint64_t)j, (uint64_t)sg.numel, sg.h, sg.key);
        hit = sg.in[idx] != 0.0f; /* distinct positions: in place, nobody else has written idx */
        sg.out[idx] = 0.0f;
    }
    const unsigned long long tot = block_sum_u64<STREAM_THREADS>(hit);
    if (threadIdx.x == 0 && tot) atomicAdd((unsigned long long*)&res[sg.res].zero_count, tot);
}

/* ---------------------------------------------------------------- launchers --- */
void launch_random_prune(const RandTable& t, wtp_result* res, hipStream_t s) {
    if (t.copy_begin[t.nseg] > 0)
        hipLaunchKernelGGL(k_rand_copy, dim3(t.copy_begin[t.nseg]), dim3(STREAM_THREADS), 0, s, t, res);
    if (t.zero_begin[t.nseg] > 0)
        hipLaunchKernelGGL(k_rand_zero, dim3(t.zero_begin[t.nseg]), dim3(STREAM_THREADS), 0, s, t, res);
}

}  // namespace wtp

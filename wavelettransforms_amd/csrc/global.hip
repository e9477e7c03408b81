/*
 * global.hip -- the global percentile (wtp_prune_global_f32): the sweep's exact selection of up to
 * SW_MAX_PCT percentiles' order statistics, over the pool of every tensor's keys.
 *
 *   k_global_pass    sweep.hip's k_sweep_pass with the pool's state: a workgroup histograms the
 *                    pass's digit of its chunks' keys in LDS (pass 1 every key, passes 2 and 3 the
 *                    keys whose prefix owns a slot: gl_hist_index) and flushes the bins it filled
 *                    into the pool's ONE histogram with global atomic adds -- the workgroups of
 *                    every tensor and of every launch group add into the same words.  Pass 1
 *                    raises the pool's maximum key, one atomic per workgroup (an LDS maximum
 *                    first: every workgroup of the call meets on that one word).
 *   k_global_scan    one workgroup for the call, one wave per slot: every rank's bin and residual
 *                    in its slot's histogram, the next pass's slots; <3> ends with each
 *                    percentile's lerp and writes the pool's npct thresholds (float32 word, float64)
 *   k_global_records one small launch per launch group after the third scan: record (k, t) from
 *                    tensor t's own fields (the group's table) and the pool's values at
 *                    percentile k (gl_fill_record), and thr[k] into word (k, t) of the table that
 *                    sweep.hip's k_sweep_mask indexes, which masks the untransformed tensors
 *                    unchanged.
 *
 * Plain launches in stream order; the state and histograms are zeroed by the call's first launch
 * (sweep.hip's k_sweep_init).  The digits, the rank search, the slots and the lerp are
 * wt_sweep_core.h's; the pool's part is wt_global_core.h's, which tests/native/globalcore.cpp runs
 * on the host.
 */
#include "wtp_device.h"

#pragma clang fp contract(off)

namespace wtp {

static __device__ __forceinline__ int gl_find_seg(const int32_t (&blk_begin)[SEG_PER_LAUNCH], int b) {
    int s = 0; /* blk_begin[0] == 0; entries past nseg hold INT32_MAX */
#pragma unroll
    for (int i = 1; i < SEG_PER_LAUNCH; ++i) s += b >= blk_begin[i];
    return s;
}

template <int PASS>
__global__ __launch_bounds__(SW_THREADS) void k_global_pass(GlTable t, GlWs w) {
    constexpr int NH = PASS == 1 ? SW_BINS1 : SW_SLOT_WORDS;
    __shared__ uint32_t h[NH];
    __shared__ __attribute__((aligned(4))) uint8_t tab1[PASS >= 2 ? SW_BINS1 : 16];
    __shared__ __attribute__((aligned(4))) uint8_t tab2[PASS == 3 ? SW_SLOT_WORDS : 16];
    __shared__ uint32_t wg_max;
    const int tid = threadIdx.x;
    const int si = gl_find_seg(t.blk_begin, blockIdx.x);
    const GlSeg& sg = t.s[si];
    SwState& S = *w.st;
    const int ns2 = PASS >= 2 ? min((int)S.nslots[0], SW_MAX_RANKS) : 0;
    const int ns3 = PASS == 3 ? min((int)S.nslots[1], SW_MAX_RANKS) : 0;
    const int nh = PASS == 1 ? SW_BINS1 : (PASS == 2 ? ns2 : ns3) * SW_BINS;
    for (int i = tid; i < nh; i += SW_THREADS) h[i] = 0u;
    if (tid == 0) wg_max = 0u;
    if constexpr (PASS >= 2) {
        for (int i = tid; i < SW_BINS1 / 4; i += SW_THREADS) reinterpret_cast<uint32_t*>(tab1)[i] = 0xFFFFFFFFu;
    }
    if constexpr (PASS == 3) {
        for (int i = tid; i < ns2 * SW_BINS / 4; i += SW_THREADS) reinterpret_cast<uint32_t*>(tab2)[i] = 0xFFFFFFFFu;
    }
    __syncthreads();
    if constexpr (PASS >= 2) {
        if (tid < ns2) tab1[S.slot_prefix[0][tid] & (SW_BINS1 - 1)] = (uint8_t)tid;
        __syncthreads();
    }
    if constexpr (PASS == 3) {
        if (tid < ns3) {
            const uint32_t p = S.slot_prefix[1][tid];
            const uint32_t s2 = tab1[(p >> 10) & (SW_BINS1 - 1)];
            if (s2 != SW_NO_SLOT) tab2[s2 * SW_BINS + (p & (SW_BINS - 1))] = (uint8_t)tid;
        }
        __syncthreads();
    }
    uint32_t mk = 0;
    auto add = [&](uint32_t key) {
        if constexpr (PASS == 1) mk = max(mk, key);
        const int i = gl_hist_index(key, PASS, tab1, tab2);
        if (PASS == 1 || i >= 0) atomicAdd(&h[i], 1u);
    };
    const int64_t nchunks = (sg.n + SW_CHUNK - 1) / SW_CHUNK;
    const int64_t c0 = (int64_t)(blockIdx.x - t.blk_begin[si]) * t.cpb;
    const int64_t c1 = min(nchunks, c0 + t.cpb);
    const bool aligned = (reinterpret_cast<uintptr_t>(sg.data) & 15) == 0;
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t base = c * SW_CHUNK;
        const int len = (int)min<int64_t>(SW_CHUNK, sg.n - base);
        float4 v[16];
        if (aligned && len == SW_CHUNK) {
            load_chunk<16, SW_THREADS>(sg.data + base, v);
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                add(abs_key(v[it].x)); add(abs_key(v[it].y)); add(abs_key(v[it].z)); add(abs_key(v[it].w));
            }
        } else {
            load_chunk_ragged<16, SW_THREADS>(sg.data + base, len, v);
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int e = 4 * (it * SW_THREADS + tid);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (e + q < len) add(abs_key(f4_get(v[it], q)));
            }
        }
    }
    if constexpr (PASS == 1) {
        mk = wave_max_u32(mk); /* every lane is active here */
        if ((tid & 63) == 0 && mk) atomicMax(&wg_max, mk);
    }
    __syncthreads();
    uint32_t* gh = PASS == 1 ? w.h1 : (PASS == 2 ? w.h2 : w.h3);
    for (int i = tid; i < nh; i += SW_THREADS) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&gh[i], c);
    }
    if constexpr (PASS == 1) {
        if (tid == 0 && wg_max) atomicMax(&S.maxkey, wg_max);
    }
}

/* One wave per slot: lane l sums PER consecutive bins of its slot's histogram, a wave scan makes
 * them inclusive prefix sums in LDS, and every rank then searches its slot's (sw_locate).  The
 * sums are at most the pool's count, which fits 32 bits (gl_pool_count). */
template <int PASS>
__global__ __launch_bounds__(SW_SCAN_THREADS) void k_global_scan(GlRanks r, GlWs w) {
    constexpr int NBINS = PASS == 1 ? SW_BINS1 : SW_BINS;
    constexpr int PER = NBINS / 64;
    __shared__ uint32_t incl[PASS == 1 ? SW_BINS1 : SW_SLOT_WORDS];
    __shared__ uint32_t npre[SW_MAX_RANKS], nres[SW_MAX_RANKS], sp[SW_MAX_RANKS];
    __shared__ uint8_t rs[SW_MAX_RANKS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    SwState& S = *w.st;
    const int npct = min(r.npct, SW_MAX_PCT), nranks = 2 * npct;
    const int nsl = PASS == 1 ? 1 : min((int)S.nslots[PASS == 1 ? 0 : PASS - 2], SW_MAX_RANKS);
    /* this thread's rank: where it is looked up, and what is known of its key */
    uint32_t my_r = 0, my_pre = 0;
    int my_slot = -1;
    if (tid < nranks) {
        if constexpr (PASS == 1) {
            const int k = tid >> 1;
            my_r = gl_rank(r.r0[k], (r.above >> k) & 1u, tid & 1);
            my_slot = 0;
        } else {
            my_r = S.rank_res[tid];
            my_pre = S.rank_prefix[tid];
            my_slot = min((int)S.rank_slot[tid], nsl - 1);
        }
    }
    if (wave < nsl) { /* wave-uniform: every lane of a scanning wave is active */
        const uint32_t* hg = PASS == 1 ? w.h1 : (PASS == 2 ? w.h2 : w.h3) + (size_t)wave * SW_BINS;
        uint32_t loc[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) loc[j] = hg[lane * PER + j];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            sum += loc[j];
            loc[j] = sum;
        }
        const uint32_t off = wave_scan_u32(sum) - sum;
#pragma unroll
        for (int j = 0; j < PER; ++j) incl[wave * NBINS + lane * PER + j] = off + loc[j];
    }
    __syncthreads();
    if (my_slot >= 0) {
        uint32_t resid;
        const int d = sw_locate(incl + my_slot * NBINS, NBINS, my_r, &resid);
        npre[tid] = sw_extend(my_pre, (uint32_t)d, PASS);
        nres[tid] = resid;
    }
    __syncthreads();
    if constexpr (PASS < 3) {
        if (tid == 0) S.nslots[PASS - 1] = (uint32_t)sw_assign_slots(npre, nranks, sp, rs);
        __syncthreads();
        if (tid < nranks) {
            S.slot_prefix[PASS - 1][tid] = sp[tid]; /* past the slot count: unused */
            S.rank_prefix[tid] = npre[tid];
            S.rank_res[tid] = nres[tid];
            S.rank_slot[tid] = rs[tid];
        }
    } else {
        /* every rank's prefix is its key: np.percentile's lerp per percentile, once for the call */
        if (tid < npct) {
            double thr64;
            w.thr[tid] = sw_lerp(npre[2 * tid], npre[2 * tid + 1], r.gamma[tid], S.maxkey, &thr64);
            w.thr64[tid] = thr64;
        }
    }
}

__global__ __launch_bounds__(SW_THREADS) void k_global_records(GlRecTable t, GlWs w, wtp_result* __restrict__ res) {
    const int nseg = min(t.nseg, SEG_PER_LAUNCH), npct = min(t.npct, SW_MAX_PCT);
    const int i = threadIdx.x;
    if (i >= nseg * npct) return;
    const int k = i / nseg, j = i - k * nseg;
    const GlRecSeg& sg = t.s[j];
    const size_t ri = gl_record_index(k, t.ntensors, t.t0 + j);
    const float thr32 = w.thr[k];
    gl_fill_record(&res[ri], sg.numel, sg.coeff_numel, sg.eff_level, w.thr64[k], __float_as_uint(thr32), w.st->maxkey);
    w.thr_tab[ri] = thr32;
}
static_assert(SEG_PER_LAUNCH * SW_MAX_PCT <= SW_THREADS, "k_global_records: a thread per record of the group");

void launch_global_pass(const GlTable& t, int pass, const GlWs& w, hipStream_t s) {
    const dim3 g((unsigned)t.nblk), b(SW_THREADS);
    if (pass == 1) hipLaunchKernelGGL(k_global_pass<1>, g, b, 0, s, t, w);
    else if (pass == 2) hipLaunchKernelGGL(k_global_pass<2>, g, b, 0, s, t, w);
    else hipLaunchKernelGGL(k_global_pass<3>, g, b, 0, s, t, w);
}

void launch_global_scan(const GlRanks& r, int pass, const GlWs& w, hipStream_t s) {
    const dim3 g(1), b(SW_SCAN_THREADS);
    if (pass == 1) hipLaunchKernelGGL(k_global_scan<1>, g, b, 0, s, r, w);
    else if (pass == 2) hipLaunchKernelGGL(k_global_scan<2>, g, b, 0, s, r, w);
    else hipLaunchKernelGGL(k_global_scan<3>, g, b, 0, s, r, w);
}

void launch_global_records(const GlRecTable& t, const GlWs& w, wtp_result* res, hipStream_t s) {
    hipLaunchKernelGGL(k_global_records, dim3(1), dim3(SW_THREADS), 0, s, t, w, res);
}

}  // namespace wtp

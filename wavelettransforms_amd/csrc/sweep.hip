/*
 * sweep.hip -- the percentile sweep (wtp_prune_sweep_f32): one exact selection of the order
 * statistics of up to SW_MAX_PCT percentiles at once, and the level-0 mask that writes all their
 * outputs from one read.
 *
 *   k_sweep_init   the call's first launch: zeroes the states and histograms the passes add into
 *   k_sweep_pass   <1>: every workgroup histograms the top digit of its chunks' keys in LDS,
 *                  flushes the bins it filled with global atomic adds and raises the maximum key;
 *                  <2>, <3>: a key whose prefix owns a slot (two small LDS tables: top digit ->
 *                  pass-2 slot, (pass-2 slot, second digit) -> pass-3 slot) adds to that slot's LDS
 *                  histogram of the pass's digit; one flush per workgroup
 *   k_sweep_scan   one workgroup per tensor, one wave per slot: every rank's bin and residual in
 *                  its slot's histogram, the next pass's slots; <3> ends with each percentile's lerp, its
 *                  record and its float32 threshold word
 *   k_sweep_mask   level-0 and ndim < 2 tensors: a chunk is read once, every percentile's masked
 *                  copy is stored and its exact zeros are counted into its record
 *
 * Plain launches in stream order: no waits between workgroups, no co-resident grid.  The digit
 * split, the rank search, the slot assignment and the lerp are wt_sweep_core.h's, which
 * tests/native/sweepcore.cpp runs on the host.
 */
#include "wtp_device.h"

#pragma clang fp contract(off)

namespace wtp {

static __device__ __forceinline__ int sw_find_seg(const int32_t (&blk_begin)[SEG_PER_LAUNCH], int b) {
    int s = 0; /* blk_begin[0] == 0; entries past nseg hold INT32_MAX */
#pragma unroll
    for (int i = 1; i < SEG_PER_LAUNCH; ++i) s += b >= blk_begin[i];
    return s;
}

__global__ __launch_bounds__(SW_THREADS) void k_sweep_init(uint32_t* __restrict__ words, int64_t nwords) {
    for (int64_t i = (int64_t)blockIdx.x * SW_THREADS + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * SW_THREADS)
        words[i] = 0u;
}

template <int PASS>
__global__ __launch_bounds__(SW_THREADS) void k_sweep_pass(SwTable t, SwWs w) {
    constexpr int NH = PASS == 1 ? SW_BINS1 : SW_SLOT_WORDS;
    __shared__ uint32_t h[NH];
    __shared__ __attribute__((aligned(4))) uint8_t tab1[PASS >= 2 ? SW_BINS1 : 16];
    __shared__ __attribute__((aligned(4))) uint8_t tab2[PASS == 3 ? SW_SLOT_WORDS : 16];
    const int tid = threadIdx.x;
    const int si = sw_find_seg(t.blk_begin, blockIdx.x);
    const SwSeg& sg = t.s[si];
    SwState& S = w.st[sg.t];
    const int ns2 = PASS >= 2 ? min((int)S.nslots[0], SW_MAX_RANKS) : 0;
    const int ns3 = PASS == 3 ? min((int)S.nslots[1], SW_MAX_RANKS) : 0;
    const int nh = PASS == 1 ? SW_BINS1 : (PASS == 2 ? ns2 : ns3) * SW_BINS;
    for (int i = tid; i < nh; i += SW_THREADS) h[i] = 0u;
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
        if constexpr (PASS == 1) {
            mk = max(mk, key);
            atomicAdd(&h[sw_digit(key, 1)], 1u);
        } else {
            const uint32_t s2 = tab1[sw_digit(key, 1)];
            if (s2 != SW_NO_SLOT) {
                if constexpr (PASS == 2) {
                    atomicAdd(&h[s2 * SW_BINS + sw_digit(key, 2)], 1u);
                } else {
                    const uint32_t s3 = tab2[s2 * SW_BINS + sw_digit(key, 2)];
                    if (s3 != SW_NO_SLOT) atomicAdd(&h[s3 * SW_BINS + sw_digit(key, 3)], 1u);
                }
            }
        }
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
    __syncthreads();
    uint32_t* gh = PASS == 1 ? w.h1 + (size_t)sg.t * SW_BINS1 : (PASS == 2 ? w.h2 : w.h3) + (size_t)sg.t * SW_SLOT_WORDS;
    for (int i = tid; i < nh; i += SW_THREADS) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&gh[i], c);
    }
    if constexpr (PASS == 1) {
        mk = wave_max_u32(mk);
        if ((tid & 63) == 0 && mk) atomicMax(&S.maxkey, mk);
    }
}

/* One wave per slot: lane l sums PER consecutive bins of its slot's histogram, a wave scan makes
 * them inclusive prefix sums in LDS, and every rank then searches its slot's (sw_locate). */
template <int PASS>
__global__ __launch_bounds__(SW_SCAN_THREADS) void k_sweep_scan(SwTable t, SwWs w, wtp_result* __restrict__ res) {
    constexpr int NBINS = PASS == 1 ? SW_BINS1 : SW_BINS;
    constexpr int PER = NBINS / 64;
    __shared__ uint32_t incl[PASS == 1 ? SW_BINS1 : SW_SLOT_WORDS];
    __shared__ uint32_t npre[SW_MAX_RANKS], nres[SW_MAX_RANKS], sp[SW_MAX_RANKS];
    __shared__ uint8_t rs[SW_MAX_RANKS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const SwSeg& sg = t.s[blockIdx.x];
    SwState& S = w.st[sg.t];
    const int npct = min(t.npct, SW_MAX_PCT), nranks = 2 * npct;
    const int nsl = PASS == 1 ? 1 : min((int)S.nslots[PASS == 1 ? 0 : PASS - 2], SW_MAX_RANKS);
    /* this thread's rank: where it is looked up, and what is known of its key */
    uint32_t my_r = 0, my_pre = 0;
    int my_slot = -1;
    if (tid < nranks) {
        if constexpr (PASS == 1) {
            const int k = tid >> 1;
            my_r = sg.r0[k] + (((tid & 1) && !((sg.above >> k) & 1u)) ? 1u : 0u);
            my_slot = 0;
        } else {
            my_r = S.rank_res[tid];
            my_pre = S.rank_prefix[tid];
            my_slot = min((int)S.rank_slot[tid], nsl - 1);
        }
    }
    if (wave < nsl) { /* wave-uniform: every lane of a scanning wave is active */
        const uint32_t* hg = PASS == 1 ? w.h1 + (size_t)sg.t * SW_BINS1
                                       : (PASS == 2 ? w.h2 : w.h3) + (size_t)sg.t * SW_SLOT_WORDS + (size_t)wave * SW_BINS;
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
        /* every rank's prefix is its key: np.percentile's lerp per percentile, the record's fields
         * (the zero count is accumulated by the kernels that write the outputs) */
        if (tid < npct) {
            const int k = tid;
            const uint32_t mkey = S.maxkey;
            double thr64;
            const float thr32 = sw_lerp(npre[2 * k], npre[2 * k + 1], sg.gamma[k], mkey, &thr64);
            const size_t ri = (size_t)k * t.ntensors + sg.t;
            w.thr[ri] = thr32;
            wtp_result& r = res[ri];
            r.numel = sg.numel;
            r.zero_count = 0;
            r.coeff_numel = sg.n;
            r.thr64 = thr64;
            r.thr32_bits = __float_as_uint(thr32);
            r.max_abs_bits = mkey;
            r.eff_level = sg.eff_level;
            r.path = WTP_PATH_SWEEP;
        }
    }
}

/* out_k = where(|x| < thr_k, +0, x) for every percentile k from one read of the chunk: every
 * element is in registers before any copy of it is stored, so one output may be the input */
__global__ __launch_bounds__(SW_THREADS) void k_sweep_mask(SwMaskTable t, const float* __restrict__ thr,
                                                          wtp_result* __restrict__ res) {
    __shared__ unsigned long long zc[SW_MAX_PCT];
    const int tid = threadIdx.x;
    const int si = sw_find_seg(t.blk_begin, blockIdx.x);
    const SwMaskSeg& sg = t.s[si];
    const int npct = min(t.npct, SW_MAX_PCT);
    const int64_t base = (int64_t)(blockIdx.x - t.blk_begin[si]) * SW_CHUNK;
    const int len = (int)min<int64_t>(SW_CHUNK, sg.n - base);
    if (len <= 0) return; /* block-uniform */
    const bool full = sg.aligned && len == SW_CHUNK;
    if (tid < SW_MAX_PCT) zc[tid] = 0;
    float4 v[16];
    if (full) load_chunk<16, SW_THREADS>(sg.data + base, v);
    else load_chunk_ragged<16, SW_THREADS>(sg.data + base, len, v);
    __syncthreads();
    for (int k = 0; k < npct; ++k) {
        const float th = thr[(size_t)k * t.ntensors + sg.t];
        float* q = sg.out[k] + base;
        uint32_t z = 0;
        auto f = [&](float xv) { return wt_thr_mask(xv, th); };
        if (full) {
            float4* q4 = reinterpret_cast<float4*>(q);
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                float4 y;
                y.x = f(v[it].x); y.y = f(v[it].y); y.z = f(v[it].z); y.w = f(v[it].w);
                z += (y.x == 0.0f) + (y.y == 0.0f) + (y.z == 0.0f) + (y.w == 0.0f);
                q4[it * SW_THREADS + tid] = y;
            }
        } else {
            /* range-checked stores: writes past len are dropped */
            const __amdgpu_buffer_rsrc_t r = ragged_rsrc(q, len);
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int e = 4 * (it * SW_THREADS + tid);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float y = f(f4_get(v[it], c));
                    z += (e + c < len) && (y == 0.0f);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), r, 4 * (e + c), 0, 0);
                }
            }
        }
        z = wave_sum_u32(z);
        if ((tid & 63) == 0 && z) atomicAdd(&zc[k], (unsigned long long)z);
    }
    __syncthreads();
    if (tid < npct && zc[tid])
        atomicAdd(reinterpret_cast<unsigned long long*>(&res[(size_t)tid * t.ntensors + sg.t].zero_count), zc[tid]);
}

void launch_sweep_init(uint32_t* words, int64_t nwords, hipStream_t s) {
    int64_t blocks = (nwords + (int64_t)SW_THREADS * 16 - 1) / ((int64_t)SW_THREADS * 16);
    blocks = std::min<int64_t>(std::max<int64_t>(blocks, 1), 2048);
    hipLaunchKernelGGL(k_sweep_init, dim3((unsigned)blocks), dim3(SW_THREADS), 0, s, words, nwords);
}

void launch_sweep_pass(const SwTable& t, int pass, const SwWs& w, wtp_result* res, hipStream_t s) {
    const dim3 g((unsigned)t.nblk), gs((unsigned)t.nseg), b(SW_THREADS), bs(SW_SCAN_THREADS);
    if (pass == 1) {
        hipLaunchKernelGGL(k_sweep_pass<1>, g, b, 0, s, t, w);
        hipLaunchKernelGGL(k_sweep_scan<1>, gs, bs, 0, s, t, w, res);
    } else if (pass == 2) {
        hipLaunchKernelGGL(k_sweep_pass<2>, g, b, 0, s, t, w);
        hipLaunchKernelGGL(k_sweep_scan<2>, gs, bs, 0, s, t, w, res);
    } else {
        hipLaunchKernelGGL(k_sweep_pass<3>, g, b, 0, s, t, w);
        hipLaunchKernelGGL(k_sweep_scan<3>, gs, bs, 0, s, t, w, res);
    }
}

void launch_sweep_mask(const SwMaskTable& t, const float* thr, wtp_result* res, hipStream_t s) {
    hipLaunchKernelGGL(k_sweep_mask, dim3((unsigned)t.nblk), dim3(SW_THREADS), 0, s, t, thr, res);
}

}  // namespace wtp

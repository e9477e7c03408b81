/*
 * resident.inc -- k_resident, the level-0 prune of a whole launch group in one persistent launch
 * (DESIGN.md), with its host-side knobs: the wait bound, the span stamps and the early stores.
 * Built with -ffp-contract=off: the float32 operation order IS the parity contract.
 */
#include "wtp_select.h"

#include <atomic>
#include <cstdlib>

#pragma clang fp contract(off)

namespace wtp {

/* ------------------------------------------------------------- k_resident --- */
/* The level-0 prune of a whole launch group in ONE launch.  Every workgroup is resident (one per
 * CU; the host checks the grid against resident_capacity()) and holds its chunk in VGPRs from
 * the first read to the masked write, so HBM sees 4 B read + 4 B written per weight -- the
 * algorithmic minimum -- and the selection's two dependent steps run between them:
 *   P0  the sample loads, then the chunk's loads (RES_IT float4 per thread); the segment's
 *       window is built from the sample while the chunk is in flight (every workgroup of a
 *       segment draws the same sample and derives the same window)
 *   P1  from registers: count keys < kl and == kl, max key; histogram the keys inside (kl, kh]
 *       over the buckets in LDS, reserve one run per non-empty bucket (returning atomic), re-scan
 *       the registers and scatter the inside keys with write-through (sc1) stores
 *   --  grid barrier: each workgroup's waves drain their stores (vmcnt(0)), lane 0 adds to its
 *       shard's arrival counter (blockIdx % 8), wave 0 polls all shards with sc1 loads
 *   P2  every workgroup resolves its segment's threshold (select_body over sc1 loads); the
 *       segment's first workgroup publishes the record and the exact zero count
 *   P3  out = where(|x| < thr, 0, x) from registers; a shared segment's workgroups (out of
 *       place) store every wave-wide float4 already decided by the ranks' bucket as soon as their
 *       selector publishes it, ahead of the threshold (the early stores, above res_body)
 * A segment whose window missed is re-scanned from memory (full radix select); when its input is
 * also its output (in place) its workgroups meet at a segment-wide barrier before any writes.
 * Every wait is bounded (RES_TIMEOUT of the 100 MHz wall clock): a grid that is not co-resident
 * after all drains instead of hanging, and its records read MODE_FAULT. */
/* The window search of k_resident for ONE wave over the flat NB-bin histogram h of the m sampled
 * keys: lane l owns the RES_BPL consecutive bins from l * RES_BPL (odd stride: no bank
 * conflicts); one scan of the lane sums finds the lane holding a sample rank, a second scan over
 * that lane's bins (RES_BPL - 1 by the lanes, the last one by elimination) finds the bin. */
constexpr int RES_BPL = 65;
constexpr int RES_HBINS = 64 * RES_BPL; /* >= NB; the bins past NB stay 0 */
static_assert(RES_HBINS >= NB, "flat window histogram");
__device__ __forceinline__ void wave_find_bins_flat(const uint32_t* h, int ra, int rb, int* fa, int* fb) {
    const int lane = threadIdx.x & 63;
    uint32_t s = 0;
#pragma unroll
    for (int q = 0; q < RES_BPL; ++q) s += h[lane * RES_BPL + q];
    const int incl = (int)wave_scan_u32(s), excl = incl - (int)s;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = i == 0 ? ra : rb;
        int f = -1;
        const uint64_t msk = __ballot(r >= 0 && excl <= r && r < incl);
        if (msk) {
            const int L = __ffsll((unsigned long long)msk) - 1;
            const int before = __builtin_amdgcn_readlane(excl, L);
            const uint32_t c = h[L * RES_BPL + lane];
            const int i2 = before + (int)wave_scan_u32(lane < RES_BPL - 1 ? c : 0u);
            const int e2 = i2 - (int)(lane < RES_BPL - 1 ? c : 0u);
            const uint64_t m2 = __ballot(lane < RES_BPL - 1 && e2 <= r && r < i2);
            f = L * RES_BPL + (m2 ? __ffsll((unsigned long long)m2) - 1 : RES_BPL - 1);
        }
        if (i == 0) *fa = f; else *fb = f;
    }
}
__device__ __forceinline__ void window_search_flat(const SegDesc& sd, const uint32_t* h, int m, bool exact,
                                                   uint32_t* kl_out, uint32_t* kh_out, uint32_t* sh_out, double sig,
                                                   double add) {
    const int64_t n = sd.n;
    const int64_t r0 = sd.r0, r1 = sd.above ? sd.r0 : sd.r0 + 1;
    int sa, sb;
    if (exact) {
        sa = (int)r0;
        sb = (int)r1;
    } else {
        const double p = (double)r0 / (double)(n - 1);
        const double s0 = p * (double)(m - 1), s1 = (double)r1 / (double)(n - 1) * (double)(m - 1);
        const double d = sig * sqrt((double)m * p * (1.0 - p)) + add;
        sa = (int)floor(s0 - d);
        sb = (int)ceil(s1 + d);
    }
    int f0, f1;
    wave_find_bins_flat(h, sa, sb < m ? sb : -1, &f0, &f1);
    const uint32_t kl = (sa < 0 || f0 < 0) ? 0u : bin_lo_key(f0);
    const uint32_t kh = (sb >= m || f1 < 0) ? 0xFFFFFFFFu : bin_hi_key(f1);
    uint32_t sh = 0;
    if (kh > kl + 1) {
        const uint32_t R = kh - kl - 1;
        const int bits = 32 - __clz(R);
        sh = bits > sd.nsub_log2 ? bits - sd.nsub_log2 : 0;
    }
    *kl_out = kl;
    *kh_out = kh;
    *sh_out = sh;
}

/* One lane's wait until the segment barrier counter reaches `want` arrivals (sc1 loads, s_sleep
 * between polls).  A wait that outlasts `timeout` ticks poisons the counter -- only while it is
 * still short of `want` (compare-and-swap) -- so every workgroup of the segment either passes the
 * barrier or sees the poison: all of them store, or none does.  Returns 1 when the barrier passed. */
__device__ __forceinline__ uint32_t res_poll_counter(uint32_t* ctr, uint32_t want, uint64_t timeout) {
    const uint64_t t0 = wall_ticks();
    uint32_t ok = 0;
    while (true) {
        const uint32_t v = ldc<true>(ctr);
        if (v & RES_POISON) break;
        if (v >= want) { ok = 1; break; }
        if (wall_ticks() - t0 >= timeout) { /* >=: a zero bound poisons at the first incomplete look */
            if (atomicCAS(ctr, v, v | RES_POISON) == v) break;
            continue; /* it moved: look again */
        }
        __builtin_amdgcn_s_sleep(2);
    }
    return ok;
}

/* res_poll_counter by thread 0; the other waves wait at the workgroup barrier, then load.
 * Block-uniform result. */
__device__ __forceinline__ bool res_wait(uint32_t* ctr, uint32_t want, uint64_t timeout) {
    __shared__ int s_ok;
    if (threadIdx.x == 0) s_ok = (int)res_poll_counter(ctr, want, timeout);
    __syncthreads();
    return s_ok != 0;
}

/* every wave drains its stores (vmcnt(0)), then lane 0 arrives: the sc1 hand-off form of
 * MI355X_MICROARCH.md (one arrival per workgroup for all its stores) */
__device__ __forceinline__ void res_arrive(uint32_t* ctr) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(ctr, 1u);
}

/* the workspace parity, loaded at the kernel's start by a VECTOR load (qv) and made uniform only
 * where it is first needed, behind the chunk's loads: a scalar load of it is waited by the first
 * s_waitcnt lgkmcnt(0) -- every LDS barrier -- and put its device round trip (~1 us) ahead of
 * the sample's and the chunk's loads.  The asm keeps the read from being hoisted above the loads
 * (the wait the compiler inserts for it then counts only the older parity load). */
__device__ __forceinline__ uint32_t parity_late(uint32_t qv) {
    uint32_t q;
    asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(q) : "v"(qv) : "memory");
    return q;
}

/* k_resident's last pass: out = where(|x| < thr, 0, x) from registers; a NaN threshold prunes
 * nothing and the copy's zeros are counted (the pad slots read as +0.0 excluded) */
template <bool FULL>
__device__ __forceinline__ void res_final(const float4 (&v)[RES_IT], float thr, const SegDesc& sd,
                                          wtp_result* __restrict__ res, int64_t base, int len, bool al) {
    constexpr int CT = RES_THREADS, IT = RES_IT;
    const int tid = threadIdx.x;
    float* qo = sd.out + base;
    auto fin = [&](float xv) { return wt_thr_mask(xv, thr); };
    if (FULL) {
        float4* q4 = reinterpret_cast<float4*>(qo);
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            typedef float f4v __attribute__((ext_vector_type(4)));
            const f4v yv = {fin(v[it].x), fin(v[it].y), fin(v[it].z), fin(v[it].w)};
            __builtin_nontemporal_store(yv, reinterpret_cast<f4v*>(q4 + it * CT + tid));
        }
    } else {
        const __amdgpu_buffer_rsrc_t rr = ragged_rsrc(qo, len);
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const float4 y = make_float4(fin(v[it].x), fin(v[it].y), fin(v[it].z), fin(v[it].w));
            store4_tail(y, qo, rr, it * CT + tid, len, al);
        }
    }
    if (thr != thr) { /* uniform */
        uint32_t z = 0;
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int c = 0; c < 4; ++c) z += f4_get(v[it], c) == 0.0f;
        const unsigned long long tot = block_sum_u64<CT>(z) - (unsigned long long)(RES_CHUNK - len);
        if (tid == 0 && tot) atomicAdd((unsigned long long*)&res[sd.res].zero_count, tot);
    }
    WTP_RPROBE(7);
}

/* ---- early stores (a remote segment's data workgroups, out of place) ----
 * The selector publishes the bound granule {lo, hi} -- the key range of the ranks' buckets, which
 * holds both order statistics and so the threshold -- three hops (barrier 2, offsets, keys + LDS
 * select) before the threshold granule.  Every key outside [lo, hi] is decided by it exactly:
 * key < lo <= ka gives |x| < thr (0), key > hi >= kb gives |x| > thr (kept).  A wave-wide float4
 * store (64 lanes x 16 B) none of whose 256 keys lies in [lo, hi] goes out whole on the bound;
 * the others (a few per cent: [lo, hi] is 1/1024 of the window) are held back for the threshold,
 * one bit each in a wave-uniform mask.  Nothing is written twice, except after RES_GR_ALL. */

/* one poll of a slot's granule pair {thr_gr, bnd_gr}: ONE aligned 16-byte sc1 load (each 8-byte
 * half is written whole by one store or compare-and-swap) */
__device__ __forceinline__ void res_poll_pair(const SelState* st, unsigned long long* thr, unsigned long long* bnd) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    u4v x;
    const unsigned long long* p = &st->thr_gr;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(x) : "v"(p) : "memory");
    *thr = ((unsigned long long)x.y << 32) | x.x;
    *bnd = ((unsigned long long)x.w << 32) | x.z;
}

/* float4 slot `it` of the thread, in res_final's store forms */
template <bool FULL>
__device__ __forceinline__ void res_store_slot(const float4& y, float* qo, __amdgpu_buffer_rsrc_t rr, int it, int len,
                                               bool al) {
    const int j = it * RES_THREADS + (int)threadIdx.x;
    if (FULL) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v yv = {y.x, y.y, y.z, y.w};
        __builtin_nontemporal_store(yv, reinterpret_cast<f4v*>(qo) + j);
    } else {
        store4_tail(y, qo, rr, j, len, al);
    }
}

/* the wave's decided float4 stores on the bound [lo, hi]; returns the wave-uniform mask of the
 * slots held back (bit it: some lane of the wave has a key of slot it inside [lo, hi]).
 * STORE = false: classification only (the polling wave when RES_EARLY_POLL_STORES is off). */
template <bool FULL, bool STORE>
__device__ __forceinline__ uint32_t res_early_stores(const float4 (&v)[RES_IT], uint32_t lo, uint32_t hi,
                                                     const SegDesc& sd, int64_t base, int len, bool al) {
    float* qo = sd.out + base;
    const __amdgpu_buffer_rsrc_t rr = ragged_rsrc(qo, FULL ? 0 : len);
    const uint32_t w = hi - lo;
    uint32_t pend = 0; /* wave-uniform: a scalar register */
#pragma unroll
    for (int it = 0; it < RES_IT; ++it) {
        uint32_t k4[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) k4[c] = abs_key(f4_get(v[it], c));
        const bool in = (k4[0] - lo <= w) | (k4[1] - lo <= w) | (k4[2] - lo <= w) | (k4[3] - lo <= w);
        if (__ballot(in) != 0ull) { /* uniform */
            pend |= 1u << it;
        } else if (STORE) {
            const float4 y = make_float4(k4[0] < lo ? 0.0f : v[it].x, k4[1] < lo ? 0.0f : v[it].y,
                                         k4[2] < lo ? 0.0f : v[it].z, k4[3] < lo ? 0.0f : v[it].w);
            res_store_slot<FULL>(y, qo, rr, it, len, al);
        }
    }
    return pend;
}

/* after the threshold granule: the slots of `pend` with the threshold itself (finite: the bound
 * is published only for a segment without NaN and with finite rank buckets) */
template <bool FULL>
__device__ __forceinline__ void res_pending_stores(const float4 (&v)[RES_IT], uint32_t pend, float thr,
                                                   const SegDesc& sd, int64_t base, int len, bool al) {
    float* qo = sd.out + base;
    const __amdgpu_buffer_rsrc_t rr = ragged_rsrc(qo, FULL ? 0 : len);
    auto fin = [&](float xv) { return wt_thr_mask(xv, thr); };
    pend = __builtin_amdgcn_readfirstlane(pend); /* wave-uniform: scalar branches below */
#pragma unroll
    for (int it = 0; it < RES_IT; ++it)
        if (pend & (1u << it)) { /* uniform */
            const float4 y = make_float4(fin(v[it].x), fin(v[it].y), fin(v[it].z), fin(v[it].w));
            res_store_slot<FULL>(y, qo, rr, it, len, al);
        }
    WTP_RPROBE(7);
}

/* the parity flip's second level: the last reader of a shard (blockIdx % 8) adds to the top
 * counter, whose last arrival flips the parity (every workgroup of the grid has read it); arr is
 * the result of the workgroup's first-level arrival */
__device__ __forceinline__ void res_parity_arrive(SelHeader* head, BarState* bar, uint32_t q, uint32_t arr) {
    const uint32_t sh8 = blockIdx.x & (NSHARD - 1);
    const uint32_t nsh = (gridDim.x - sh8 + NSHARD - 1) / NSHARD;
    const uint32_t nact = min((uint32_t)NSHARD, gridDim.x);
    if (arr == nsh - 1u && atomicAdd(&bar->arrive[0][16], 1u) == nact - 1u) stc(&head->parity, q + 1u);
}

/* a wait timed out or met a poisoned barrier: the record reads MODE_FAULT, and a selector also
 * claims the threshold granule gr for FAULT (its data workgroups then store nothing more) */
__device__ __forceinline__ void res_fault(wtp_result* res, const SegDesc& sd, uint64_t* gr, bool sel) {
    if (threadIdx.x == 0) {
        atomicMax(&res[sd.res].path, (int32_t)MODE_FAULT);
        if (sel) atomicCAS(reinterpret_cast<unsigned long long*>(gr), 0ull, (unsigned long long)RES_GR_FAULT << 32);
    }
}

/* the key range [res_bucket_lo(ba), res_bucket_hi(bb)] of the buckets ba..bb of the window [kl, kh]
 * (bucket of a key: (k - kl) >> sh) */
__device__ __forceinline__ uint32_t res_bucket_lo(uint32_t kl, uint32_t sh, int ba) {
    return (uint32_t)((uint64_t)kl + ((uint64_t)ba << sh));
}
__device__ __forceinline__ uint32_t res_bucket_hi(uint32_t kl, uint32_t kh, uint32_t sh, int bb) {
    return (uint32_t)min((uint64_t)kh, (uint64_t)kl + ((uint64_t)(bb + 1) << sh) - 1);
}

template <bool FULL>
__device__ __forceinline__ void res_body(const SegTable& t, const SegDesc& sd, SelHeader* __restrict__ head, uint32_t qv,
                                         uint32_t* __restrict__ cand, wtp_result* __restrict__ res,
                                         float* __restrict__ thr_out, int64_t base, int len, uint32_t* raw,
                                         uint32_t* lsub, uint32_t (*wred)[8], uint32_t* wstage, bool sel) {
    constexpr int CT = RES_THREADS, IT = RES_IT, NW = CT / 64;
    uint32_t q = 0;
    /* sel: this workgroup is its segment's selector (no chunk: len 0, its loads read nothing) */
    const bool first = base == 0 && !sel;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const uint64_t tmo = t.res_timeout;
    WTP_RPROBE(0);
    WTP_RTAG(sd.flags);
    __shared__ uint32_t s_win[3];
    __shared__ uint32_t s_sync; /* the sampling waves' LDS meeting counter */
    __shared__ uint32_t s_pubn; /* the storing waves drained (publication) */
    __shared__ uint32_t s_arr;  /* wave 7's first-level parity arrival */
    float4 v[IT];
    uint32_t arr1 = 0; /* wave 7 lane 0: the first-level parity arrival's result */
    /* ---- P0: the sample waves' loads go out before any chunk load of the workgroup (the barrier
     * below orders them), then every wave issues its chunk; the sample arrives first (a wave's
     * loads return in order) and is histogrammed while the chunk streams in; wave 0 searches the
     * histogram for the window [kl, kh] bracketing the segment's two ranks */
    {
        uint32_t ks[RES_SPL];
        const int64_t n = sd.n;
        const bool exact = n <= RES_MS;
        const int m = exact ? (int)n : RES_MS;
        if (wv < RES_SW) {
            /* group g = i / SAMPLE_GROUP starts at floor(g * (n - SAMPLE_GROUP) / (RES_MS / SAMPLE_GROUP - 1)),
             * in 32.32 fixed point from the host (res_step_fx): two 32-bit multiplies a load */
            const uint32_t sl = (uint32_t)sd.res_step_fx, shi = (uint32_t)(sd.res_step_fx >> 32);
#pragma unroll
            for (int j = 0; j < RES_SPL; ++j) {
                const int i = j * (64 * RES_SW) + tid;
                const uint32_t g = (uint32_t)i / SAMPLE_GROUP;
                const int pos = exact ? min(i, (int)n - 1)
                                      : (int)(__umulhi(g, sl) + g * shi) + (i % SAMPLE_GROUP);
                ks[j] = __float_as_uint(sd.data[pos]); /* raw bits: |x| at the histogram */
            }
        }
        for (int j = tid; j < RES_HBINS; j += CT) raw[j] = 0u;
        for (int j = tid; j < RES_NSUB; j += CT) lsub[j] = 0u;
        if (tid == 0) { s_sync = 0u; s_pubn = 0u; }
        if (first && tid == 0) { /* memory-side words: later adds come from other workgroups */
            stc(reinterpret_cast<unsigned long long*>(&res[sd.res].zero_count), 0ull);
            stc(&res[sd.res].path, 0);
        }
        __syncthreads(); /* the sample's loads are out before any chunk load of the workgroup */
        WTP_RPROBE(8);
        /* the sampling waves histogram their sample (it comes back ahead of the flood) and wave 0
         * searches the window; the other waves go straight to the loads.  The chunk is loaded at
         * ONE program point by every wave: a single definition of v[], so the compiler keeps the
         * loads' destination registers and nothing waits for the data before it is counted; the
         * sample's |x| is taken here, behind the barrier, by an AND the compiler cannot fold back
         * into the loads' block (it would make the sampling waves wait for the sample before the
         * barrier) */
        if (wv < RES_SW) {
#pragma unroll
            for (int j = 0; j < RES_SPL; ++j)
                if (j * (64 * RES_SW) + tid < m) {
                    uint32_t k;
                    asm volatile("v_and_b32 %0, 0x7fffffff, %1" : "=v"(k) : "v"(ks[j]));
                    atomicAdd(&raw[key_bin(k)], 1u);
                }
            /* the sampling waves meet on an LDS counter (the others do not wait for them) */
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) atomicAdd(&s_sync, 1u);
            if (wv == 0) {
                while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&s_sync, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_WORKGROUP)) < (uint32_t)RES_SW)
                    __builtin_amdgcn_s_sleep(1);
                asm volatile("" ::: "memory");
                uint32_t wkl, wkh, wsh;
                window_search_flat(sd, raw, m, exact, &wkl, &wkh, &wsh, RES_SIGMA_X100 * 0.01, 8.0);
                if (lane == 0) { s_win[0] = wkl; s_win[1] = wkh; s_win[2] = wsh; }
                WTP_RPROBE(1);
            }
        }
        /* a late workgroup (SEG_LATE: the group's small segments) issues its chunk only once
         * the window is known: the early group's chunks come off HBM first, and their counts,
         * barriers and selects run while the late group's chunks stream */
        if (sd.flags & SEG_LATE) __syncthreads(); /* block-uniform */
        if (FULL) load_chunk<IT, CT, true>(sd.data + base, v);
        else load_chunk_ragged<IT, CT, true>(sd.data + base, len, v);
        q = parity_late(qv);
        {   /* clear this workgroup's slice of the idle region (the previous launch's; the next
             * launch works in it): stores behind the chunk's loads */
            uint4* idle = reinterpret_cast<uint4*>(sel_region(head, q ^ 1u));
            constexpr int NV4 = (int)(SEL_REGION / 16);
            const int per = (NV4 + (int)gridDim.x - 1) / (int)gridDim.x;
            for (int i = tid; i < per; i += CT) {
                const int j = (int)blockIdx.x * per + i;
                if (j < NV4) idle[j] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        /* the parity flip's first-level arrival (the last reader of the parity in the grid flips
         * it): a returning add issued behind wave 7's chunk loads, its result used only at the
         * publication, so its queueing on the shard's counter costs no wave a wait */
        if (wv == NW - 1 && lane == 0) arr1 = atomicAdd(&bar_region(head, q)->arrive[blockIdx.x & (NSHARD - 1)][0], 1u);
        WTP_RPROBE(10);
    }
    __syncthreads();
    SelState* st = sel_region(head, q) + sd.slot;
    const uint32_t kl = s_win[0], kh = s_win[1];
    /* ---- P1: one branch-free pass over the registers, two classes per key from one difference
     * d = k - kl (keys and kl < 2^31): "below" (k < kl: bit 31 of d) and "inside" [kl, kh]
     * (d <= span; keys == kl belong to bucket 0), the max key, and the inside keys appended to the
     * thread's own LDS column (slot j of thread t at col[j * CT]; every key is written to the next
     * free slot and kept only if inside -- no branch, no atomic).  In a ragged chunk the slots
     * past len were loaded as +0.0: never inside, counted below (kl > 0) and dropped once. */
    const uint32_t span = kh - kl; /* >= 1 */
    uint32_t sh = 0; /* bucket of an inside key: (k - kl) >> sh, RES_NSUB buckets */
    if (span > 0) {
        const int bits = 32 - __clz(span);
        sh = bits > RES_NSUB_LOG2 ? bits - RES_NSUB_LOG2 : 0;
    }
    uint32_t wbelow = 0, mx = 0, cnt = 0;
    uint32_t* col = wstage + tid;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        uint32_t k4[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) k4[c] = abs_key(opaque(f4_get(v[it], c)));
        mx = max(mx, max(max(k4[0], k4[1]), max(k4[2], k4[3])));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t k = k4[c];
            const uint32_t d = k - kl;
            wbelow += d >> 31;
            col[min(cnt, (uint32_t)RES_STG) * CT] = k;
            const bool valid = FULL || 4 * (it * CT + tid) + c < len;
            cnt += (d <= span) & valid;
        }
    }
    {
        wbelow = wave_sum_u32(wbelow);
        const uint32_t r2 = wave_max_u32(mx), r4 = wave_max_u32(cnt);
        if (lane == 0) { wred[wv][0] = wbelow; wred[wv][2] = r2; wred[wv][5] = r4; }
    }
    __syncthreads();
    WTP_RPROBE(2);
    if (wv == NW - 1 && lane == 0) s_arr = arr1;
    uint32_t wmax = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) wmax = max(wmax, wred[w][5]);
    /* block-uniform: a thread's column overflowed -> the segment takes the full scan */
    const bool ovf = wmax > (uint32_t)RES_STG;
    /* a segment of ONE workgroup (solo) selects from its own LDS: no counter, bucket total,
     * publication or barrier touches memory -- under the launch's traffic every round trip costs
     * 1-3 us, and the solo segments were the launch's tail */
    const uint32_t nwg = (uint32_t)((sd.n + RES_CHUNK - 1) / RES_CHUNK);
    const bool solo = nwg == 1u; /* block-uniform */
    /* remote: a shared segment whose select runs on its selector workgroup (a CU that holds no
     * chunk: the select's dependent round trips start from an idle memory queue); its workgroups
     * only wait for the threshold granule */
    const bool remote = t.nsel > 0 && !solo; /* block-uniform */
    const bool al = (sd.flags & SEG_ALIGNED) != 0;
    __shared__ unsigned long long s_cnt[1];
    __shared__ uint32_t s_mk, s_ovf;
    if (tid == 0) {
        unsigned long long a0 = 0;
        uint32_t m2 = 0;
        for (int w = 0; w < NW; ++w) { a0 += wred[w][0]; m2 = max(m2, wred[w][2]); }
        if (kl > 0) a0 -= (unsigned long long)(RES_CHUNK - len);
        if (solo) {
            s_cnt[0] = a0;
            s_mk = m2;
            s_ovf = ovf;
        } else if (!sel) {
            const int sh8 = blockIdx.x & (NSHARD - 1);
            if (a0) atomicAdd(&st->below[sh8], a0);
            atomicMax(&st->maxkey[sh8], m2);
            if (ovf) atomicOr(&st->overflow, 1u);
        }
    }
    /* the inside keys' bucket histogram in LDS (eight column reads in flight per step), then the
     * segment's bucket totals as no-return atomic adds */
    constexpr int BPT = RES_NSUB / CT; /* buckets per thread */
    static_assert(BPT * CT == RES_NSUB, "buckets per thread");
    if (!ovf) { /* block-uniform */
        for (uint32_t j0 = 0; j0 < cnt; j0 += 8) {
            uint32_t kk[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) kk[u] = col[min(j0 + u, (uint32_t)RES_STG) * CT];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < cnt) atomicAdd(&lsub[(kk[u] - kl) >> sh], 1u);
        }
        __syncthreads();
        if (!solo && !sel) {
#pragma unroll
            for (int j = 0; j < BPT; ++j) { /* bucket j * CT + tid: 256 contiguous bytes per wave instruction */
                const uint32_t c = lsub[j * CT + tid];
                if (c) atomicAdd(&st->sub[j * CT + tid], c);
            }
        }
    }
    WTP_RPROBE(3);
    /* ---- segment barrier 1: every workgroup's counters and bucket totals are in */
    BarState* bar = bar_region(head, q);
    uint32_t* b0 = reinterpret_cast<uint32_t*>(&st->seg_bar[0]);
    uint32_t* b1 = reinterpret_cast<uint32_t*>(&st->seg_bar[1]);
    uint32_t* b2 = reinterpret_cast<uint32_t*>(&st->seg_bar[2]);
    if (!solo) {
        if (sel) __syncthreads(); /* orders s_arr for wave 6 (the selector has no publication) */
        else res_arrive(b1);
    }
    WTP_RPROBE(4);
    /* ---- publication, while the segment gathers at barrier 1: this workgroup's inside keys,
     * bucket-sorted in LDS, and the bucket offsets (exclusive prefix of its bucket histogram),
     * write-through (16-byte sc1 stores) to its region of the candidate area, then barrier 2's
     * arrival.  It depends on nothing global: waves 0-6 store and drain it while wave 7 polls
     * barrier 1, and after barrier 1 the select reads only the keys of the ranks' buckets from
     * the regions (offsets, then keys: two round trips) -- no slot round after the locate. */
    uint32_t* pub = cand + (int64_t)blockIdx.x * RES_PUB_WORDS;
    uint32_t* pos = raw;     /* bucket offsets (the window histogram is done with) */
    uint32_t* srt = wstage;  /* the sorted keys, over the columns */
    __shared__ uint32_t s_ok1;
    if (!ovf && !sel) { /* block-uniform */
        uint32_t kk[RES_STG];
#pragma unroll
        for (int j = 0; j < RES_STG; ++j) kk[j] = col[j * CT]; /* entries past cnt are not used */
        /* exclusive scan of the bucket counts, BPT buckets per thread */
        __shared__ uint32_t s_pw[NW];
        uint32_t c[BPT], cs = 0;
#pragma unroll
        for (int j = 0; j < BPT; ++j) { c[j] = lsub[BPT * tid + j]; cs += c[j]; }
        const uint32_t inc = wave_scan_u32(cs);
        if (lane == 63) s_pw[wv] = inc;
        __syncthreads(); /* also: every column is read into kk */
        uint32_t ex = inc - cs;
#pragma unroll
        for (int w = 0; w < NW; ++w) ex += w < wv ? s_pw[w] : 0u;
#pragma unroll
        for (int j = 0; j < BPT; ++j) { pos[BPT * tid + j] = ex; ex += c[j]; }
        __syncthreads();
        /* scatter, four keys at a time with no branch (a key past cnt counts into its lane's
         * spare counter pos[RES_NSUB + lane] -- one per lane: a shared one serialised every
         * atomic 64 ways -- and lands in the spare words past the sorted array): the four
         * returning atomics issue back to back; the trip count is the wave's largest cnt */
        const uint32_t wc = wred[wv][5];
#pragma unroll
        for (int j0 = 0; j0 < RES_STG; j0 += 4) {
            if ((uint32_t)j0 < wc) {
                uint32_t pp[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = (uint32_t)(j0 + u) < cnt;
                    pp[u] = atomicAdd(&pos[ok ? (kk[j0 + u] - kl) >> sh : (uint32_t)(RES_NSUB + lane)], 1u);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = (uint32_t)(j0 + u) < cnt;
                    srt[ok ? pp[u] : (uint32_t)(RES_STG * CT + lane)] = kk[j0 + u];
                }
            }
        }
        __syncthreads();
    }
    WTP_RPROBE(9);
    if (solo) {
        /* s_arr (wave 7's store after its returning add) must be visible to wave 6: on the
         * non-overflow path the publication's barriers order it; an overflowing solo segment has
         * none of them (block-uniform branch) */
        if (ovf) __syncthreads();
        /* the parity flip's second level (as the storing waves do it below) */
        if (tid == 64 * (NW - 2)) res_parity_arrive(head, bar, q, s_arr);
        if (tid == 0) s_ok1 = 1;
    } else if (wv == NW - 1 && remote && !sel) {
        if (lane == 0) s_ok1 = 1; /* a remote segment's workgroup does not wait at barrier 1 */
    } else if (wv == NW - 1) {
        /* ---- barrier 1, polled by wave 7 while the others store (the selector: by wave 7) */
        if (lane == 0) s_ok1 = res_poll_counter(b1, nwg, tmo);
    } else {
        constexpr int ST = CT - 64; /* the storing threads */
        if (!ovf && !sel) {
            /* offsets: pub[b] = start of bucket b (pos[b - 1] now), pub[RES_NSUB] = the total */
            const __amdgpu_buffer_rsrc_t prs = region_rsrc(pub, RES_PUB_WORDS);
            if (tid < RES_NSUB / 4) {
                const int b = 4 * tid;
                st16_sc1(prs, b, make_uint4(b ? pos[b - 1] : 0u, pos[b], pos[b + 1], pos[b + 2]));
            } else if (tid == RES_NSUB / 4) {
                stc(pub + RES_NSUB, pos[RES_NSUB - 1]);
            }
            const uint32_t nin = pos[RES_NSUB - 1];
            for (uint32_t i4 = tid; 4 * i4 < nin; i4 += ST)
                st16_sc1(prs, RES_PUB_KEYS + 4 * i4, *reinterpret_cast<const uint4*>(srt + 4 * i4));
        }
        /* every storing wave drains; the last one to do so arrives at barrier 2 for the
         * workgroup (its LDS add follows every other storing wave's drain) */
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (!sel && lane == 0 && atomicAdd(&s_pubn, 1u) == (uint32_t)(NW - 2)) atomicAdd(b2, 1u);
        /* the parity flip's second level -- wave 6, after its drain, off the barrier-1 poll */
        if (wv == NW - 2 && lane == 0) res_parity_arrive(head, bar, q, s_arr);
    }
    __syncthreads();
    WTP_RPROBE(11);
    uint64_t* gr = reinterpret_cast<uint64_t*>(&st->thr_gr);
    if (!s_ok1) {
        res_fault(res, sd, gr, sel);
        return; /* nothing stored to the output: the caller's input and output are untouched */
    }
    WTP_RPROBE(5);
    if (remote && !sel) {
        /* ---- the threshold granule {thr bits, tag} from the segment's selector (one 8-byte sc1
         * word; the region is zero at the launch's start).  A wait that times out claims the
         * granule for FAULT by compare-and-swap, so every workgroup of the segment and the
         * selector agree: all store, or none does */
        __shared__ unsigned long long s_gr, s_bnd;
        const bool early = t.res_early != 0; /* uniform over the grid (kernel argument) */
        if (wv == NW - 1 && lane == 0) {
            const uint64_t t0 = wall_ticks();
            unsigned long long x, b = 0ull;
            while (true) {
                if (early) res_poll_pair(st, &x, &b);
                else x = ldc<true>(reinterpret_cast<const unsigned long long*>(gr));
                if (x) break;
                if (b) break; /* the bound first: the decided stores go out now */
                if (wall_ticks() - t0 >= tmo) {
                    const unsigned long long f = (unsigned long long)RES_GR_FAULT << 32;
                    const unsigned long long o = atomicCAS(reinterpret_cast<unsigned long long*>(gr), 0ull, f);
                    x = o ? o : f;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            s_gr = x;
            s_bnd = b;
        }
        __syncthreads();
        unsigned long long g = s_gr;
        if (g == 0ull) {
            /* ---- the bound granule came first: every wave stores its decided float4 now (the
             * polling wave too: RES_EARLY_POLL_STORES) and keeps the rest for the threshold */
            const unsigned long long bw = s_bnd;
            const uint32_t lo = (uint32_t)bw, hi = (uint32_t)(bw >> 32) & ~RES_BND_VALID;
            WTP_RPROBE(20); /* bound seen */
            uint32_t pend;
            if (wv == NW - 1 && !RES_EARLY_POLL_STORES) pend = res_early_stores<FULL, false>(v, lo, hi, sd, base, len, al);
            else pend = res_early_stores<FULL, true>(v, lo, hi, sd, base, len, al);
            WTP_RPROBE(21); /* early stores issued */
            if (t.res_early == 2 && lane == 0) { /* measurement only */
                const uint32_t nd = (uint32_t)__builtin_popcount(pend);
                atomicAdd(&head->early_ws, (uint32_t)IT - nd);
                if (nd) atomicAdd(&head->defer_ws, nd);
            }
            __syncthreads(); /* s_gr is read by every wave before it is rewritten */
            if (wv == NW - 1 && lane == 0) {
                const uint64_t t0 = wall_ticks();
                unsigned long long x;
                while (true) {
                    x = ldc<true>(reinterpret_cast<const unsigned long long*>(gr));
                    if (x) break;
                    if (wall_ticks() - t0 >= tmo) {
                        const unsigned long long f = (unsigned long long)RES_GR_FAULT << 32;
                        const unsigned long long o = atomicCAS(reinterpret_cast<unsigned long long*>(gr), 0ull, f);
                        x = o ? o : f;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                s_gr = x;
            }
            __syncthreads();
            g = s_gr;
            const uint32_t tag2 = (uint32_t)(g >> 32);
            if (tag2 & RES_GR_FAULT) { /* out of place: the output stays partly written, the record says FAULT */
                res_fault(res, sd, gr, false);
                return;
            }
            const float thr2 = __uint_as_float((uint32_t)g);
            WTP_RPROBE(6);
            if ((tag2 & RES_GR_ALL) || thr2 != thr2) {
                res_final<FULL>(v, thr2, sd, res, base, len, al); /* the selector left [lo, hi]: every float4 again */
            } else {
                if (wv == NW - 1 && !RES_EARLY_POLL_STORES) pend = (1u << IT) - 1u; /* the polling wave: all of its float4 */
                res_pending_stores<FULL>(v, pend, thr2, sd, base, len, al);
            }
            return;
        }
        const uint32_t tag = (uint32_t)(g >> 32);
        if (tag & RES_GR_FAULT) {
            res_fault(res, sd, gr, false);
            return;
        }
        const float thr = __uint_as_float((uint32_t)g);
        WTP_RPROBE(6);
        res_final<FULL>(v, thr, sd, res, base, len, al);
        return;
    }
    /* ---- P2: the segment's counters and bucket totals in one round trip (every load in
     * flight before any is used); a block scan of the totals names the bucket of each rank */
    __shared__ uint32_t s_wtot[NW], s_b2;
    __shared__ int s_bk[2];
    __shared__ uint32_t s_bef[2], s_bn[2];
    if (!solo) {
        if (tid == 0) {
            unsigned long long x[NSHARD];
#pragma unroll
            for (int i = 0; i < NSHARD; ++i) x[i] = ldc<true>(st->below + i);
            unsigned long long sum = 0;
#pragma unroll
            for (int i = 0; i < NSHARD; ++i) sum += x[i];
            s_cnt[0] = sum;
        } else if (tid == 2) {
            uint32_t x[NSHARD];
#pragma unroll
            for (int i = 0; i < NSHARD; ++i) x[i] = ldc<true>(st->maxkey + i);
            uint32_t mm = 0;
#pragma unroll
            for (int i = 0; i < NSHARD; ++i) mm = max(mm, x[i]);
            s_mk = mm;
        } else if (tid == 3) {
            s_ovf = ldc<true>(&st->overflow);
        } else if (tid == 4) {
            /* barrier 2's counter in the same round trip: its arrivals were made before barrier
             * 1's wait, so it is usually complete already and its poll round trip is skipped */
            s_b2 = ldc<true>(b2);
        }
    }
    if (tid < 2) { s_bk[tid] = -1; s_bef[tid] = 0; s_bn[tid] = 0; }
    uint32_t cb8[BPT]; /* buckets BPT * tid .. + BPT - 1, every load in flight before any is used */
#pragma unroll
    for (int j = 0; j < BPT; ++j) cb8[j] = solo ? lsub[BPT * tid + j] : ldc<true>(st->sub + BPT * tid + j);
    uint32_t cs = 0;
#pragma unroll
    for (int j = 0; j < BPT; ++j) cs += cb8[j];
    const uint32_t incl = wave_scan_u32(cs);
    if (lane == 63) s_wtot[wv] = incl;
    __syncthreads();
    WTP_PROBE(1);
    const int64_t sbelow = (int64_t)s_cnt[0];
    const uint32_t mk = s_mk;
    uint32_t excl = incl - cs, ninside = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const uint32_t x = s_wtot[w]; ninside += x; excl += w < wv ? x : 0u; }
    const int64_t r0 = sd.r0, r1 = sd.above ? sd.r0 : sd.r0 + 1;
    /* class of a rank: 0 outside the window, 2 inside [kl, kh] at inside-rank j */
    auto classify = [&](int64_t r, int64_t* j) {
        if (r < sbelow) return 0;
        r -= sbelow;
        if (r < (int64_t)ninside) { *j = r; return 2; }
        return 0;
    };
    int64_t ja = 0, jb = 0;
    const int ca = classify(r0, &ja), cb = classify(r1, &jb);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t j = i == 0 ? ja : jb;
        if ((i == 0 ? ca : cb) == 2 && j >= (int64_t)excl && j < (int64_t)(excl + cs)) {
            uint32_t e = excl;
            int b = BPT * tid;
#pragma unroll
            for (int u = 0; u < BPT - 1; ++u) {
                const bool past = j >= (int64_t)(e + cb8[u]) && b == BPT * tid + u;
                e += past ? cb8[u] : 0u;
                b += past ? 1 : 0;
            }
            s_bk[i] = b;
            s_bef[i] = e;
            s_bn[i] = cb8[b - BPT * tid];
        }
    }
    __syncthreads();
    WTP_PROBE(2);
    bool full = ca == 0 || cb == 0 || s_ovf != 0;
    int path = MODE_WINDOW;
    uint32_t ka = kl, kb = kl;
    uint32_t before = 0;
    int m = 0;
    uint32_t* stage = raw; /* the window histogram is done with */
    const uint32_t* sel_keys = stage; /* the staged keys of the ranks' buckets */
    bool bnd_pub = false;      /* the selector published the bound granule [blo, bhi] */
    uint32_t blo = 0, bhi = 0;
    if (!full && (ca == 2 || cb == 2)) {
        const int ba = ca == 2 ? s_bk[0] : s_bk[1], bb = cb == 2 ? s_bk[1] : s_bk[0];
        before = ca == 2 ? s_bef[0] : s_bef[1];
        const uint32_t nlo = ca == 2 ? s_bn[0] : s_bn[1], nhi = (bb != ba) ? s_bn[1] : 0u;
        m = (int)(nlo + nhi);
        if (solo) {
            /* the ranks' buckets ba..bb are one run of this workgroup's sorted keys in LDS (the
             * buckets between are empty); pos[b] is the end of bucket b after the scatter */
            sel_keys = srt + (ba ? pos[ba - 1] : 0u);
            const uint32_t lo = res_bucket_lo(kl, sh, ba), hi = res_bucket_hi(kl, kh, sh, bb);
            uint32_t xa = kl, xb = kl;
            select_in_range<CT>([&](int64_t i) { return sel_keys[i]; }, [](uint32_t) { return true; }, (int64_t)m, lo,
                                hi, ja - (int64_t)before, jb - (int64_t)before, ca == 2, cb == 2, &xa, &xb);
            ka = ca == 2 ? xa : kl;
            kb = cb == 2 ? xb : kl;
            path = MODE_CAND;
        } else if (m > RES_SEL_MAX) {
            full = true; /* uniform over the segment: the same totals everywhere */
        } else {
            /* ---- the bound granule: the ranks' buckets are named, so the threshold lies in
             * [blo, bhi] -- published before barrier 2's wait, for the data workgroups' early
             * stores.  Only where that range is certain to hold the threshold and a rewrite would
             * be harmless: both ranks inside the window, no overflow, no NaN (mk), no inf in the
             * rank buckets (the lerp stays finite), out of place; and only for a window closed on
             * both sides (pct 0 and 100 open it below / above: no bound there). */
            if (sel && t.res_early != 0 && ca == 2 && cb == 2 && mk <= 0x7F800000u && sd.out != sd.data && kl > 0u &&
                kh != 0xFFFFFFFFu) {
                blo = res_bucket_lo(kl, sh, ba);
                bhi = res_bucket_hi(kl, kh, sh, bb);
                bnd_pub = bhi < 0x7F800000u; /* block-uniform */
                if (bnd_pub && tid == 0)
                    stc(&st->bnd_gr, ((unsigned long long)(bhi | RES_BND_VALID) << 32) | blo);
            }
            /* ---- barrier 2: every region of the segment is published (its arrivals were made
             * before barrier 1's wait, so this wait is short) */
            WTP_PROBE(3);
            const uint32_t b2v = s_b2; /* block-uniform */
            if (!(b2v >= nwg && !(b2v & RES_POISON)) && !res_wait(b2, nwg, tmo)) {
                res_fault(res, sd, gr, sel);
                return;
            }
            WTP_PROBE(4);
            /* ---- the segment's workgroups' offsets of buckets ba and bb + 1 (wave 0, every load
             * in flight at once), their key counts scanned; then the keys themselves, at most two
             * a thread (m <= RES_SEL_MAX), staged in LDS.  The buckets between ba and bb are
             * empty, so a workgroup's keys of ba..bb are one run of its sorted array. */
            const int wb = sd.blk_begin;
            __shared__ uint32_t s_so[RES_MAX_WG], s_ob[RES_MAX_WG];
            __shared__ uint32_t s_tot;
            if (wv == 0) {
                constexpr int WPL = RES_MAX_WG / 64;
                uint32_t ob[WPL], oe[WPL];
#pragma unroll
                for (int u = 0; u < WPL; ++u) {
                    const int w = lane + 64 * u;
                    const uint32_t* pw = cand + (int64_t)(wb + min(w, (int)nwg - 1)) * RES_PUB_WORDS;
                    ob[u] = ldc<true>(pw + ba);
                    oe[u] = ldc<true>(pw + bb + 1);
                }
                uint32_t base = 0;
#pragma unroll
                for (int u = 0; u < WPL; ++u) {
                    const int w = lane + 64 * u;
                    const uint32_t cw = w < (int)nwg ? oe[u] - ob[u] : 0u;
                    const uint32_t inc = wave_scan_u32(cw);
                    if (w < (int)nwg) { s_so[w] = base + inc - cw; s_ob[w] = ob[u]; }
                    base += __builtin_amdgcn_readlane(inc, 63);
                }
                if (lane == 0) s_tot = base;
            }
            __syncthreads();
            if ((int)s_tot != m) {
                full = true; /* uniform over the segment (the same regions everywhere) */
            } else {
                uint32_t kv[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int i = min(tid + u * CT, m - 1);
                    int lo_w = 0, hi_w = (int)nwg - 1; /* the last workgroup whose run starts <= i */
                    while (lo_w < hi_w) {
                        const int mid = (lo_w + hi_w + 1) >> 1;
                        if (s_so[mid] <= (uint32_t)i) lo_w = mid; else hi_w = mid - 1;
                    }
                    kv[u] = ldc<true>(cand + (int64_t)(wb + lo_w) * RES_PUB_WORDS + RES_PUB_KEYS + s_ob[lo_w] +
                                      ((uint32_t)i - s_so[lo_w]));
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (tid + u * CT < m) stage[tid + u * CT] = kv[u];
                __syncthreads();
                WTP_PROBE(5);
                /* ---- the ranks among the staged keys (buckets ba..bb; buckets between are empty:
                 * the two ranks are adjacent): an LDS radix select of both at once */
                const uint32_t lo = res_bucket_lo(kl, sh, ba), hi = res_bucket_hi(kl, kh, sh, bb);
                uint32_t xa = kl, xb = kl;
                select_in_range<CT>([&](int64_t i) { return stage[i]; }, [](uint32_t) { return true; }, (int64_t)m,
                                    lo, hi, ja - (int64_t)before, jb - (int64_t)before, ca == 2, cb == 2, &xa, &xb);
                ka = ca == 2 ? xa : kl;
                kb = cb == 2 ? xb : kl;
                path = MODE_CAND;
            }
        }
    }
    WTP_PROBE(6);
    if (full) {
        /* the window missed (or a column or slot overflowed): exact radix select over the
         * segment's input in memory -- every workgroup of the segment takes this branch */
        const float* x = sd.data;
        select_in_range<CT>([&](int64_t i) { return abs_key(x[i]); }, [](uint32_t) { return true; }, sd.n, 0u,
                            0xFFFFFFFFu, r0, r1, true, true, &ka, &kb);
        path = MODE_FULL;
    }
    /* threshold: numpy/lib/function_base.py _lerp -- diff in float32, the blend in float64 */
    const float fa = __uint_as_float(ka), fb = __uint_as_float(kb);
    const float diff = fb - fa;
    const double g = sd.gamma;
    double thr64 = (g >= 0.5) ? (double)fb - (double)diff * (1.0 - g) : (double)fa + (double)diff * g;
    if (mk > 0x7F800000u) thr64 = __longlong_as_double(0x7FF8000000000000ll); /* NaN present: np.percentile is NaN */
    const float thr = (float)thr64;
    const bool nan = thr != thr; /* also inf - inf inside the lerp */
    if (sel && tid == 0) {
        /* the threshold granule for the segment's workgroups, ahead of the record: {thr bits, tag},
         * claimed by compare-and-swap (a workgroup whose wait timed out may have claimed it for
         * FAULT) */
        /* RES_GR_ALL also where the ranks resolved outside a published bound (cannot happen with
         * consistent totals; the rewrite keeps the output exact if it ever does) */
        const uint32_t tag = RES_GR_OK | ((path == MODE_FULL || (bnd_pub && (ka < blo || kb > bhi))) ? RES_GR_ALL : 0u);
        const unsigned long long gv = ((unsigned long long)tag << 32) | __float_as_uint(thr);
        if (atomicCAS(reinterpret_cast<unsigned long long*>(gr), 0ull, gv) != 0ull)
            atomicMax(&res[sd.res].path, (int32_t)MODE_FAULT);
    }
    WTP_RPROBE(6);
    if (first || sel) {
        /* zeros of where(|x| < thr, 0, x) = #(key < tk), tk = bits(thr) when thr > 0, else 1 (only
         * the zeros themselves); ka <= thr <= kb and the ranks are adjacent, so #(key < tk) =
         * below + before + #(staged < tk).  A NaN threshold prunes nothing: every
         * workgroup counts the zeros of its copy below. */
        unsigned long long zc = 0;
        if (!nan) {
            const uint32_t tk = thr > 0.0f ? __float_as_uint(thr) : 1u;
            if (path == MODE_FULL) {
                /* a selector counts AFTER publishing the granule: in place, the segment's data
                 * workgroups may already be overwriting sd.data.  The count is unchanged by them:
                 * where(|x| < thr, 0, x) turns every key < tk into +0 (key 0 < tk) and leaves every
                 * other key as it was (tests/test_gpu_resident.py::
                 * test_cfg2_in_place_full_scan_with_selectors) */
                zc = (unsigned long long)block_count_below<CT>([&](int64_t i) { return abs_key(sd.data[i]); }, sd.n, tk);
            } else {
                uint32_t c = 0;
                if (path == MODE_CAND)
                    for (int i = tid; i < m; i += CT) c += sel_keys[i] < tk;
                const unsigned long long sc = block_sum_u64<CT>(c);
                zc = (unsigned long long)sbelow +
                     (path == MODE_CAND ? (unsigned long long)before : 0ull) + sc;
            }
        }
        if (tid == 0) {
            thr_out[sd.res] = thr; /* per tensor */
            wtp_result& r = res[sd.res];
            r.numel = sd.numel;
            r.coeff_numel = sd.n;
            if (zc) atomicAdd((unsigned long long*)&r.zero_count, zc);
            r.thr64 = thr64;
            r.thr32_bits = __float_as_uint(thr);
            r.max_abs_bits = mk;
            r.eff_level = sd.eff_level;
            atomicMax(&r.path, path);
        }
    }
    if (sel) return;
    if (path == MODE_FULL && sd.out == sd.data) { /* in place: nobody writes before the segment's scans end */
        res_arrive(b0);
        if (!res_wait(b0, nwg, tmo)) {
            res_fault(res, sd, gr, false);
            return;
        }
    }
    WTP_RPROBE(6);
    /* ---- P3: out = where(|x| < thr, 0, x) from registers (a NaN threshold prunes nothing) */
    res_final<FULL>(v, thr, sd, res, base, len, al);
    WTP_RPROBE(7);
}

__global__ __launch_bounds__(RES_THREADS) void k_resident(SegTable t, SelHeader* __restrict__ head,
                                                          uint32_t* __restrict__ cand, wtp_result* __restrict__ res,
                                                          float* __restrict__ thr_out) {
    __shared__ __attribute__((aligned(16))) uint32_t raw[RES_HBINS > RES_SEL_MAX ? RES_HBINS : RES_SEL_MAX];
    __shared__ uint32_t lsub[RES_NSUB];
    __shared__ uint32_t wred[RES_THREADS / 64][8];
    __shared__ __attribute__((aligned(16))) uint32_t wstage[(RES_STG + 1) * RES_THREADS]; /* 66 KB: RES_STG slots + the discard slot per thread */
    const uint32_t qv = ldc<true>(&head->parity); /* a vector load: see parity_late */
    if (t.stamps && threadIdx.x == 0) atomicMin(t.stamps, wall_ticks()); /* measurement only */
    /* workgroups past the chunks are selectors, one per shared segment (t.sel_seg) */
    const bool sel = (int)blockIdx.x >= t.nblk;
    const int si = sel ? t.sel_seg[blockIdx.x - t.nblk] : find_seg(t, blockIdx.x);
    const SegDesc& sd = t.s[si];
    const int64_t base = sel ? 0 : (int64_t)(blockIdx.x - sd.blk_begin) * RES_CHUNK;
    const int len = sel ? 0 : (int)min((int64_t)RES_CHUNK, sd.n - base);
    if ((sd.flags & SEG_ALIGNED) && len == RES_CHUNK)
        res_body<true>(t, sd, head, qv, cand, res, thr_out, base, len, raw, lsub, wred, wstage, false);
    else
        res_body<false>(t, sd, head, qv, cand, res, thr_out, base, len, raw, lsub, wred, wstage, sel);
    if (t.stamps) { /* measurement only: the workgroup's end, once its stores have completed */
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(t.stamps + 1, wall_ticks());
    }
}

/* ---------------------------------------------------------------- launchers --- */
int resident_capacity() {
    static std::atomic<int> cache[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
    if (dev < 16) {
        const int c = cache[dev].load(std::memory_order_relaxed);
        if (c) return c > 0 ? c : 0;
    }
    int per = 0, cus = 0;
    int cap = -1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_resident, RES_THREADS, 0) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && per >= 1 && cus > 0)
        cap = cus; /* one workgroup per CU: the form the inter-workgroup hand-off is specified for */
    (void)hipGetLastError();
    if (dev < 16) cache[dev].store(cap, std::memory_order_relaxed);
    return cap > 0 ? cap : 0;
}
static std::atomic<uint32_t> g_res_timeout_us{RES_TIMEOUT_DEFAULT_US};
uint32_t set_resident_timeout_us(uint32_t us) { return g_res_timeout_us.exchange(std::min(us, RES_TIMEOUT_MAX_US)); }
static std::atomic<unsigned long long*> g_stamps{nullptr};
void set_kernel_stamps(unsigned long long* dev) { g_stamps.store(dev); }
/* early stores: on unless the environment says otherwise (WTP_RESIDENT_EARLY = 0 / 1 / 2, read
 * once; wtp_set_resident_early overrides it) */
static int env_resident_early() {
    const char* e = getenv("WTP_RESIDENT_EARLY");
    return (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ? e[0] - '0' : 1;
}
static std::atomic<int> g_res_early{-1};
int resident_early() {
    int m = g_res_early.load(std::memory_order_relaxed);
    if (m < 0) {
        int want = env_resident_early();
        if (g_res_early.compare_exchange_strong(m, want)) m = want;
    }
    return m;
}
int set_resident_early(int mode) {
    const int prev = resident_early();
    g_res_early.store(mode);
    return prev;
}
uint32_t resident_timeout_us() { return g_res_timeout_us.load(std::memory_order_relaxed); }
unsigned long long* kernel_stamps() { return g_stamps.load(std::memory_order_relaxed); }
void launch_resident(const SegTable& t0, SelHeader* head, uint32_t* cand, wtp_result* res, float* thr_out,
                     hipStream_t s) {
    SegTable t = t0;
    t.res_timeout = g_res_timeout_us.load(std::memory_order_relaxed) * 100u; /* 100 MHz wall clock */
    t.stamps = g_stamps.load(std::memory_order_relaxed);
    t.res_early = resident_early();
    /* one selector workgroup per shared segment when they fit beside the chunks (one per CU):
     * the segment's select runs on a CU that holds no chunk */
    int nshared = 0;
    for (int i = 0; i < t.nseg; ++i) nshared += t.s[i].n > RES_CHUNK;
    t.nsel = 0;
    if (nshared > 0 && t.nblk + nshared <= RES_MAX_WG && t.nblk + nshared <= resident_capacity())
        for (int i = 0; i < t.nseg; ++i)
            if (t.s[i].n > RES_CHUNK) t.sel_seg[t.nsel++] = i;
    hipLaunchKernelGGL(k_resident, dim3(t.nblk + t.nsel), dim3(RES_THREADS), 0, s, t, head, cand, res, thr_out);
}

}  // namespace wtp

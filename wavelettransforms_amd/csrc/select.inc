/*
 * select.inc -- gfx950 kernels of the selection of the DWT -> percentile-threshold -> IDWT path.
 *
 * Selection (np.percentile(np.abs(coeff_arr), pct) + np.where(|c| < thr, 0, c),
 * ResNet/dwt_pruning.py:25-32) over grouped segments, one segment per tensor, on the float32
 * bit pattern of |x| (a key monotone in |x|; NaN sorts last as in np.partition):
 *   k_collect  every block first derives its segment's window [kl, kh] (bracketing the order
 *              statistics r0, r0+1) from the same deterministic sample of M_SAMPLE keys
 *              histogrammed into 1/128-octave bins; then it streams its chunk once: count
 *              keys < kl and == kl; scatter the keys inside (kl, kh] into key-range buckets
 *              (one run per bucket per block); max key
 *   k_mask_select  stream again: every block first resolves its segment's threshold (exact
 *              radix select of both ranks from the one or two buckets that hold them, or the
 *              whole segment if the window missed; NumPy 1.x _lerp in f64), then writes
 *              out = |x| < thr ? 0 : x (level-0 segments); the first
 *              block of a segment publishes the result and the exact zero count
 * Built with -ffp-contract=off: the float32 operation order IS the parity contract.
 */
#include "wtp_select.h"

#pragma clang fp contract(off)

namespace wtp {

/* -------------------------------------------------------------- k_collect --- */
/* IT float4 per thread: a sub-chunk of IT * CT * 4
 * elements per block.  FULL: a whole 16-byte-aligned sub-chunk (unpredicated loads);
 * otherwise a ragged or unaligned one (range-checked buffer loads).
 *
 * One pass over the chunk: per key one unsigned compare each for "below" (k < kl), "equal to
 * kl" and "inside" (kl < k <= kh, as (k - kl - 1) < (kh - kl)), and the inside keys are staged
 * in the thread's own LDS column (stage[i * CT + tid], conflict-free, no scan).  A thread may
 * stage up to STG of its 4*IT keys; more sends the segment to the full-scan select. */
constexpr int STG = 24;

/* the counting pass over a thread's IT float4 (element e of slot (it, c) is 4 (it CT + tid) + c;
 * past len -- a ragged chunk -- nothing counts): below / equal-to-kl counts, the max key, and the
 * inside keys staged in the thread's LDS column; clears the block's bucket histogram */
template <int CT, int IT>
__device__ __forceinline__ void collect_count(const float4 (&v)[IT], bool full, int len, int nsub, uint32_t kl,
                                              uint32_t kh, uint32_t* lsub, uint32_t* stage, uint32_t& below,
                                              uint32_t& eql, uint32_t& mx, uint32_t& cnt) {
    for (int i = threadIdx.x; i < nsub; i += CT) lsub[i] = 0;
    const uint32_t span = kh - kl; /* >= 1 */
    below = 0; eql = 0; mx = 0; cnt = 0;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int e = 4 * (it * CT + (int)threadIdx.x);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t k = abs_key(f4_get(v[it], c));
            const bool valid = full || e + c < len;
            mx = max(mx, k); /* 0 past len: no effect */
            below += valid && k < kl;
            eql += valid && k == kl;
            if (valid && k - kl - 1u < span) {
                if (cnt < STG) stage[cnt * CT + threadIdx.x] = k;
                ++cnt;
            }
        }
    }
}

/* the rest of a chunk: the block's counters into the segment's (8-way sharded agent atomics), the
 * inside keys bucketed by key range (LDS histogram, the block's returning reservation atomics all
 * in flight at once) and scattered into the candidate buckets */
template <int CT, int STGN = STG>
__device__ __forceinline__ void collect_finish(const SegDesc& sd, SelState* __restrict__ st, uint32_t* __restrict__ cand,
                                               uint32_t kl, uint32_t sh, uint32_t below, uint32_t eql, uint32_t mx,
                                               uint32_t cnt, uint32_t* lsub, uint32_t* lbase, uint32_t* stage,
                                               uint32_t (*wred)[4], int* wtot) {
    const int nsub = 1 << sd.nsub_log2;
    /* one block reduction for the counters */
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    {
        const uint32_t r0 = wave_sum_u32(below), r1 = wave_sum_u32(eql), r2 = wave_max_u32(mx),
                       r3 = wave_max_u32(cnt);
        if (lane == 0) { wred[wv][0] = r0; wred[wv][1] = r1; wred[wv][2] = r2; wred[wv][3] = r3; }
    }
    const uint32_t tot_w = wave_sum_u32(cnt);
    if (lane == 0) wtot[wv] = (int)tot_w;
    __syncthreads();
    WTP_CPROBE(2);
    int total = 0;
    uint32_t cmax = 0;
    for (int w = 0; w < CT / 64; ++w) { total += wtot[w]; cmax = max(cmax, wred[w][3]); }
    const bool ovf = cmax > (uint32_t)STGN;
    if (threadIdx.x == 0) {
        unsigned long long a0 = 0, a1 = 0;
        uint32_t m2 = 0;
        for (int w = 0; w < CT / 64; ++w) {
            a0 += wred[w][0];
            a1 += wred[w][1];
            m2 = max(m2, wred[w][2]);
        }
        const int sh8 = blockIdx.x & (NSHARD - 1);
        if (a0) atomicAdd(&st->below[sh8], a0);
        if (a1) atomicAdd(&st->eq_lo[sh8], a1);
        atomicMax(&st->maxkey[sh8], m2);
        if (ovf) atomicOr(&st->overflow, 1u);
    }
    /* uniform: nothing inside the window here, or a thread overflowed (full-scan select) */
    if (total == 0 || ovf) return;
    WTP_CPROBE(3);
    for (uint32_t i = 0; i < cnt; ++i) atomicAdd(&lsub[(stage[i * CT + threadIdx.x] - kl - 1) >> sh], 1u);
    __syncthreads();
    /* reserve one contiguous run per non-empty bucket (one returning atomic per bucket, all of a
     * thread's in flight at once) */
    {
        constexpr int PER = NSUB_MAX / CT;
        uint32_t cj[PER], rj[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) cj[j] = (j * CT + (int)threadIdx.x < nsub) ? lsub[j * CT + threadIdx.x] : 0u;
#pragma unroll
        for (int j = 0; j < PER; ++j) rj[j] = cj[j] ? atomicAdd(&st->sub[j * CT + threadIdx.x], cj[j]) : 0u;
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if (j * CT + (int)threadIdx.x < nsub) { lbase[j * CT + threadIdx.x] = rj[j]; lsub[j * CT + threadIdx.x] = 0; }
    }
    __syncthreads();
    WTP_CPROBE(4);
    const int64_t bcap = sd.bucket_cap;
    uint32_t* out = cand + sd.cand_off;
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t k = stage[i * CT + threadIdx.x];
        const uint32_t b = (k - kl - 1) >> sh;
        const uint32_t at = lbase[b] + atomicAdd(&lsub[b], 1u);
        if (at < bcap) out[(int64_t)b * bcap + at] = k; /* counted beyond capacity: the select sees it */
    }
    WTP_CPROBE(5);
}

/* One chunk of a k_collect_t block: its loads (and with WIN the window from the block's own
 * sample), the counting pass, the rest.  FULL: a whole 16-byte-aligned chunk (unpredicated
 * loads); otherwise a ragged or unaligned one (range-checked buffer loads). */
template <int CT, int IT, bool FULL, bool WIN>
__device__ __forceinline__ void collect_body(const SegDesc& sd, SelState* __restrict__ st,
                                             uint32_t* __restrict__ cand, int64_t base, int len, bool first,
                                             uint32_t* lsub, uint32_t* lbase, uint32_t* stage,
                                             WindowLds<CT>* wl, uint32_t (*wred)[4], int* wtot) {
    const float* p = sd.data + base;
    WTP_CPROBE(0);
    uint32_t kl, kh, sh;
    float4 v[IT];
    if constexpr (WIN) {
        /* sample loads first, then the stream loads: the window is built while the chunk arrives */
        uint32_t ks[M_SAMPLE / CT];
        sample_keys<CT, M_SAMPLE>(sd, ks);
        if (FULL) load_chunk<IT, CT>(p, v);
        else load_chunk_ragged<IT, CT>(p, len, v);
        window_from_keys<CT, M_SAMPLE>(sd, ks, *wl, &kl, &kh, &sh);
        if (first && threadIdx.x == 0) { st->kl = kl; st->kh = kh; st->shift = sh; } /* for the select */
    } else {
        /* the window came from k_window; the stream loads go out first (the window words are
         * scalar loads, counted separately from the vector loads) */
        if (FULL) load_chunk<IT, CT>(p, v);
        else load_chunk_ragged<IT, CT>(p, len, v);
        kl = st->kl;
        kh = st->kh;
        sh = st->shift;
    }
    WTP_CPROBE(1);
    uint32_t below, eql, mx, cnt;
    collect_count<CT, IT>(v, FULL, len, 1 << sd.nsub_log2, kl, kh, lsub, stage, below, eql, mx, cnt);
    collect_finish<CT>(sd, st, cand, kl, sh, below, eql, mx, cnt, lsub, lbase, stage, wred, wtot);
}

/* k_window: one 1024-thread block per segment derives the window of the region k_collect is
 * about to fill (used when the window is not computed inline by every k_collect block) */
constexpr int WIN_THREADS = 1024;
__global__ __launch_bounds__(WIN_THREADS) void k_window(SegTable t, SelHeader* __restrict__ head,
                                                         const wtp_result* __restrict__ res) {
    __shared__ WindowLds<WIN_THREADS> wl;
    const SegDesc& sd = t.s[blockIdx.x];
    if (t.retry && res[sd.res].path != MODE_RETRY) return; /* block-uniform */
    /* the sample in passes of 16 keys a thread (groups of SAMPLE_GROUP contiguous keys spread
     * evenly over the segment, as sample_keys), histogrammed as they arrive */
    constexpr int PASS = 16 * WIN_THREADS, NPASS = M_SAMPLE_WIN / PASS;
    static_assert(M_SAMPLE_WIN % PASS == 0, "sample passes");
    for (int i = threadIdx.x; i < WindowLds<WIN_THREADS>::FBP * WIN_THREADS; i += WIN_THREADS) wl.h[i] = 0;
    if (threadIdx.x < 2) wl.found[threadIdx.x] = -1;
    __syncthreads();
    {
        const int64_t n = sd.n;
        const bool exact = n <= M_SAMPLE_WIN;
        const double step = exact ? 0.0 : (double)(n - SAMPLE_GROUP) / (double)(M_SAMPLE_WIN / SAMPLE_GROUP - 1);
        for (int ps = 0; ps < NPASS; ++ps) {
            uint32_t k[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int i = ps * PASS + j * WIN_THREADS + (int)threadIdx.x;
                const int64_t pos = exact ? min((int64_t)i, n - 1)
                                          : (int64_t)((double)(i / SAMPLE_GROUP) * step) + (i % SAMPLE_GROUP);
                k[j] = abs_key(sd.data[pos]);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (!exact || ps * PASS + j * WIN_THREADS + (int)threadIdx.x < n) atomicAdd(&wl.h[key_bin(k[j])], 1u);
        }
    }
    __syncthreads();
    uint32_t kl, kh, sh;
    window_search<WIN_THREADS, M_SAMPLE_WIN>(sd, wl, &kl, &kh, &sh);
    if (threadIdx.x == 0) {
        SelState* st = sel_region(head, head->parity) + sd.slot;
        st->kl = kl;
        st->kh = kh;
        st->shift = sh;
    }
}

/* one block per sub-chunk: block b takes sub-chunk (b % SPLIT) of table block (b / SPLIT).
 * The block also clears its share of the idle SelState region (the previous group's) and the
 * zero count of its segment's result; the last block to finish flips the region parity. */
template <int CT, int IT, bool WIN>
__global__ __launch_bounds__(CT) void k_collect_t(SegTable t, SelHeader* __restrict__ head, uint32_t* __restrict__ cand,
                                                  wtp_result* __restrict__ res) {
    constexpr int SUB = IT * CT * 4, SPLIT = CHUNK / SUB;
    static_assert(CHUNK % SUB == 0, "sub-chunk size");
    __shared__ uint32_t lsub[NSUB_MAX];  /* this block's keys per bucket, then the running offset */
    __shared__ uint32_t lbase[NSUB_MAX]; /* reserved start of this block's run in each bucket     */
    __shared__ uint32_t stage[STG * CT];
    __shared__ WindowLds<WIN ? CT : 64> wl_; /* only the inline window uses it */
    WindowLds<CT>* wl = WIN ? reinterpret_cast<WindowLds<CT>*>(&wl_) : nullptr;
    __shared__ uint32_t wred[CT / 64][4];
    __shared__ int wtot[CT / 64];
    const uint32_t q = head->parity;
    {   /* clear this block's slice of the idle region */
        uint4* idle = reinterpret_cast<uint4*>(sel_region(head, q ^ 1u));
        constexpr int NV4 = (int)(SEL_REGION / 16);
        const int per = (NV4 + (int)gridDim.x - 1) / (int)gridDim.x;
        for (int i = threadIdx.x; i < per; i += CT) {
            const int j = (int)blockIdx.x * per + i;
            if (j < NV4) idle[j] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    const int tb = blockIdx.x / SPLIT;
    const int si = find_seg(t, tb);
    const SegDesc& sd = t.s[si];
    const int64_t base = (int64_t)(tb - sd.blk_begin) * CHUNK + (int64_t)(blockIdx.x % SPLIT) * SUB;
    const int len = (int)max((int64_t)0, min((int64_t)SUB, sd.n - base));
    SelState* st = sel_region(head, q) + sd.slot;
    const bool first = base == 0;
    if (first && threadIdx.x == 0) res[sd.res].zero_count = 0; /* k_mask_select and the inverse add */
    if (len > 0) {
        if ((sd.flags & SEG_ALIGNED) && len == SUB)
            collect_body<CT, IT, true, WIN>(sd, st, cand, base, len, first, lsub, lbase, stage, wl, wred, wtot);
        else
            collect_body<CT, IT, false, WIN>(sd, st, cand, base, len, first, lsub, lbase, stage, wl, wred, wtot);
    }
    __syncthreads(); /* every wave has read the parity */
    /* the grid's last block flips the parity (visible to the next kernel at the boundary).  Its
     * count is sharded (blockIdx % 8; the last block of a shard adds to the top counter, as in
     * k_small), so no single word takes a returning add from each of a cfg5 launch's ~25K blocks
     * (measured ~1 % of k_collect).  The counters sit in this region's BarState, zero at the
     * start of the launch (the previous launch cleared it as its idle region). */
    if (threadIdx.x == 0) {
        BarState* br = bar_region(head, q);
        const uint32_t sh = blockIdx.x & (NSHARD - 1);
        const uint32_t nsh = (gridDim.x - sh + NSHARD - 1) / NSHARD; /* blocks of this shard */
        const uint32_t nact = min((uint32_t)NSHARD, gridDim.x);     /* shards with blocks */
        if (atomicAdd(&br->arrive[sh][0], 1u) == nsh - 1u && atomicAdd(&br->arrive[0][16], 1u) == nact - 1u)
            head->parity = q + 1u;
    }
}

/* The fused selection's retry collect: k_collect_t over the chunks of the segments whose select
 * read MODE_RETRY only, as a grid-stride loop (a fixed small grid: when nothing missed, every block
 * reads the records and leaves); the housekeeping as k_collect_t (idle region, parity flip). */
template <int CT, int IT>
__global__ __launch_bounds__(CT) void k_collect_retry(SegTable t, SelHeader* __restrict__ head, uint32_t* __restrict__ cand,
                                                      wtp_result* __restrict__ res) {
    constexpr int SUB = IT * CT * 4, SPLIT = CHUNK / SUB;
    __shared__ uint32_t lsub[NSUB_MAX];
    __shared__ uint32_t lbase[NSUB_MAX];
    __shared__ uint32_t stage[STG * CT];
    __shared__ uint32_t wred[CT / 64][4];
    __shared__ int wtot[CT / 64];
    const uint32_t q = head->parity;
    {   /* clear this block's slice of the idle region */
        uint4* idle = reinterpret_cast<uint4*>(sel_region(head, q ^ 1u));
        constexpr int NV4 = (int)(SEL_REGION / 16);
        const int per = (NV4 + (int)gridDim.x - 1) / (int)gridDim.x;
        for (int i = threadIdx.x; i < per; i += CT) {
            const int j = (int)blockIdx.x * per + i;
            if (j < NV4) idle[j] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    const int total = t.nblk * SPLIT;
    for (int bb = blockIdx.x; bb < total; bb += gridDim.x) {
        const int tb = bb / SPLIT;
        const int si = find_seg(t, tb);
        const SegDesc& sd = t.s[si];
        if (res[sd.res].path != MODE_RETRY) continue; /* block-uniform */
        const int64_t base = (int64_t)(tb - sd.blk_begin) * CHUNK + (int64_t)(bb % SPLIT) * SUB;
        const int len = (int)max((int64_t)0, min((int64_t)SUB, sd.n - base));
        SelState* st = sel_region(head, q) + sd.slot;
        if (len > 0) {
            if ((sd.flags & SEG_ALIGNED) && len == SUB)
                collect_body<CT, IT, true, false>(sd, st, cand, base, len, false, lsub, lbase, stage, nullptr, wred, wtot);
            else
                collect_body<CT, IT, false, false>(sd, st, cand, base, len, false, lsub, lbase, stage, nullptr, wred, wtot);
        }
        __syncthreads(); /* LDS reused by the next chunk */
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        BarState* br = bar_region(head, q);
        const uint32_t sh = blockIdx.x & (NSHARD - 1);
        const uint32_t nsh = (gridDim.x - sh + NSHARD - 1) / NSHARD;
        const uint32_t nact = min((uint32_t)NSHARD, gridDim.x);
        if (atomicAdd(&br->arrive[sh][0], 1u) == nsh - 1u && atomicAdd(&br->arrive[0][16], 1u) == nact - 1u)
            head->parity = q + 1u;
    }
}

/* ------------------------------------------------------ fused selection --- */
/* k_fwin: the window of a fused segment before its forward (wtp_internal.h).  FWIN_NP blocks of
 * 1024 threads per segment, each transforming one patch of FWIN_PS^2 input samples in LDS --
 * pywt's periodization analysis at each level, the patch's own periodic extension -- and adding
 * the keys of every coefficient of every level to the segment's histogram (the FWIN_NP patches
 * give M_SAMPLE_WIN keys in the levels' population proportions); the segment's last block searches
 * the window as k_window does over its sample and leaves the histogram zeroed.  The sample is an
 * estimate: a window that misses the ranks is caught by the select, which then takes its exact
 * full-scan path, so the patches decide speed, never the result.  Patches sit at the centres of a
 * 4 x 4 Latin-square layout of the image (images b = patch % B).  Rows of the LDS images are
 * FWIN_PP = 129 floats apart: the row pass's lanes walk consecutive rows, conflict-free. */
constexpr int FWIN_RUN = 4; /* consecutive outputs per thread item: their samples shared in registers */
constexpr int FWIN_PP = FWIN_PS + 1;
template <int FT>
__global__ __launch_bounds__(FWIN_THREADS) void k_fwin(FwinTable t, SelHeader* __restrict__ head) {
    constexpr int PS = FWIN_PS, PP = FWIN_PP, NS = 2 * FWIN_RUN + FT - 2;
    __shared__ float A[PS * PP]; /* the patch, then each level's approximation */
    __shared__ float T[PS * PP]; /* a level's row-pass output: L | H halves of each row */
    __shared__ WindowLds<FWIN_THREADS> wl;
    __shared__ int s_last;
    const int si = blockIdx.x / FWIN_NP, pt = blockIdx.x - si * FWIN_NP;
    const FwinSeg& sg = t.s[si];
    for (int i = threadIdx.x; i < WindowLds<FWIN_THREADS>::FBP * FWIN_THREADS; i += FWIN_THREADS) wl.h[i] = 0;
    if (threadIdx.x < 2) wl.found[threadIdx.x] = -1;
    auto key = [&](float v) { atomicAdd(&wl.h[key_bin(abs_key(v))], 1u); };
    {
        /* eighths of the free range: rows 1, 3, 5, 7 against columns 3, 7, 1, 5 */
        const int lr = 1 + 2 * (pt & 3), lc = (0x5173 >> (4 * (pt & 3))) & 0xF;
        const int b = pt % sg.B;
        const int r0 = (int)((int64_t)(sg.R - PS) * lr / 8), c0 = (int)((int64_t)(sg.C - PS) * lc / 8);
        const float* x = sg.in + ((int64_t)b * sg.R + r0) * sg.C + c0;
        constexpr int PER = PS * PS / FWIN_THREADS; /* every load in flight before the first LDS write */
        float v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = j * FWIN_THREADS + (int)threadIdx.x;
            v[j] = x[(int64_t)(i / PS) * sg.C + (i % PS)];
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = j * FWIN_THREADS + (int)threadIdx.x;
            A[(i / PS) * PP + (i % PS)] = v[j];
        }
    }
    __syncthreads();
    int N = PS; /* a power of two at every level: the periodic index is a mask */
    for (int k = 1; k <= sg.L; ++k) {
        const int h = N / 2, runs = (h + FWIN_RUN - 1) / FWIN_RUN; /* runs: a power of two or 1 */
        const int lN = __builtin_ctz(N);
        /* rows: output j of row r is sum_q f[q] x[(2j + 1 - q) mod N]; lanes take consecutive rows */
        for (int it = threadIdx.x; it < N * runs; it += FWIN_THREADS) {
            const int ru = it >> lN, r = it - (ru << lN), j0 = ru * FWIN_RUN;
            float v[NS];
#pragma unroll
            for (int m = 0; m < NS; ++m) v[m] = A[r * PP + ((2 * j0 + 2 - FT + m) & (N - 1))];
#pragma unroll
            for (int u = 0; u < FWIN_RUN; ++u) {
                float lo = 0.0f, hi = 0.0f;
#pragma unroll
                for (int q = 0; q < FT; ++q) {
                    lo += t.lo[q] * v[2 * u + FT - 1 - q];
                    hi += t.hi[q] * v[2 * u + FT - 1 - q];
                }
                if (j0 + u < h) { T[r * PP + j0 + u] = lo; T[r * PP + h + j0 + u] = hi; }
            }
        }
        __syncthreads();
        /* columns: lanes take consecutive columns */
        for (int it = threadIdx.x; it < N * runs; it += FWIN_THREADS) {
            const int ru = it >> lN, c = it - (ru << lN), i0 = ru * FWIN_RUN;
            float v[NS];
#pragma unroll
            for (int m = 0; m < NS; ++m) v[m] = T[((2 * i0 + 2 - FT + m) & (N - 1)) * PP + c];
#pragma unroll
            for (int u = 0; u < FWIN_RUN; ++u) {
                float lo = 0.0f, hi = 0.0f;
#pragma unroll
                for (int q = 0; q < FT; ++q) {
                    lo += t.lo[q] * v[2 * u + FT - 1 - q];
                    hi += t.hi[q] * v[2 * u + FT - 1 - q];
                }
                if (i0 + u < h) {
                    key(hi);
                    if (c >= h) key(lo);           /* a detail band */
                    else if (k == sg.L) key(lo);   /* the last level's approximation */
                    if (c < h) A[(i0 + u) * PP + c] = lo; /* the next level's input */
                }
            }
        }
        __syncthreads();
        N = h;
    }
    /* this patch's counts into the segment's histogram; the last patch block takes the window */
    uint32_t* gh = t.gh + (size_t)si * FWIN_HW;
    /* agent-scope atomics (performed at the coherence point), drained before the arrival -- no
     * release fence, whose L2 write-back per block cost ~0.6 us a block, serialised (MI355X_MICROARCH:
     * __threadfence); the last block reads the counts with sc1 loads */
    for (int i = threadIdx.x; i < NB; i += FWIN_THREADS)
        if (wl.h[i]) atomicAdd(&gh[i], wl.h[i]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&gh[NB], 1u) == (uint32_t)(FWIN_NP - 1);
    __syncthreads();
    if (!s_last) return; /* block-uniform */
    for (int i = threadIdx.x; i < WindowLds<FWIN_THREADS>::FBP * FWIN_THREADS; i += FWIN_THREADS) {
        wl.h[i] = i < NB ? ldc<true>(gh + i) : 0u;
        if (i <= NB) gh[i] = 0; /* zero for the next launch (the counter too) */
    }
    if (threadIdx.x < 2) wl.found[threadIdx.x] = -1;
    __syncthreads();
    SegDesc sd = {};
    sd.n = sg.n;
    sd.r0 = sg.r0;
    sd.above = sg.above;
    sd.nsub_log2 = sg.nsub_log2;
    uint32_t kl, kh, sh;
    window_search<FWIN_THREADS, M_SAMPLE_WIN>(sd, wl, &kl, &kh, &sh);
    if (threadIdx.x == 0) { /* the window, and the forward's counters zeroed */
        FslHeader* hd = sg.hdr;
        hd->kl = kl;
        hd->kh = kh;
        hd->shift = sh;
        hd->overflow = 0;
    }
    if (threadIdx.x < NSHARD) {
        sg.hdr->maxkey[threadIdx.x] = 0;
        sg.hdr->be[threadIdx.x] = 0;
    }
}

/* k_fslot_collect: a fused group's bucket pass over its wave slots (k_fwd_int's inside keys).
 * A wave takes 64 slots, two per load: lanes 0-31 read words 0-31 of one slot and lanes 32-63 of
 * the next -- one 128-byte line per slot, which holds the count and up to 31 keys (a wave of the
 * forward classifies 768 coefficients, ~18 of them inside the window); a slot with more keys has
 * its second line read too.  Lane word j >= 1 holds key j - 1 and is kept when j <= the count.  The
 * keys are then bucketed as collect_finish buckets a chunk's (a block LDS histogram over the
 * window's buckets, one reservation per non-empty bucket, the scatter).  The forward already
 * counted the keys below and at kl and the largest key.  Housekeeping as k_collect: the idle region
 * cleared, the zero counts reset, the last block flips the parity. */
constexpr int FSC_SPW = FSC_SLOTS / (FSC_THREADS / 64); /* slots per wave */
constexpr int FSC_NP = FSC_SPW / 2;                     /* slot pairs per wave */
__global__ __launch_bounds__(FSC_THREADS) void k_fslot_collect(SegTable t, SelHeader* __restrict__ head,
                                                               uint32_t* __restrict__ cand, wtp_result* __restrict__ res) {
    static_assert(FSL_WORDS == 64 && FSC_NP <= 32, "two 32-word halves per slot, a pair bit per mask bit");
    __shared__ uint32_t lsub[NSUB_MAX];
    __shared__ uint32_t lbase[NSUB_MAX];
    __shared__ uint32_t s_any;
    const uint32_t q = head->parity;
    {   /* clear this block's slice of the idle region */
        uint4* idle = reinterpret_cast<uint4*>(sel_region(head, q ^ 1u));
        constexpr int NV4 = (int)(SEL_REGION / 16);
        const int per = (NV4 + (int)gridDim.x - 1) / (int)gridDim.x;
        for (int i = threadIdx.x; i < per; i += FSC_THREADS) {
            const int j = (int)blockIdx.x * per + i;
            if (j < NV4) idle[j] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    const int si = find_seg(t, blockIdx.x);
    const SegDesc& sd = t.s[si];
    SelState* st = sel_region(head, q) + sd.slot;
    const FslHeader* hd = reinterpret_cast<const FslHeader*>(seg_fsl(sd));
    if ((int)blockIdx.x == sd.blk_begin) { /* the segment's first block: the head into the SelState */
        if (threadIdx.x == 0) {
            res[sd.res].zero_count = 0; /* the inverse adds */
            st->kl = hd->kl;
            st->kh = hd->kh;
            st->shift = hd->shift;
            if (hd->overflow) atomicOr(&st->overflow, 1u); /* other blocks may flag it too */
        }
        if (threadIdx.x < NSHARD) {
            const unsigned long long be = hd->be[threadIdx.x];
            st->below[threadIdx.x] = be & 0xFFFFFFFFull;
            st->eq_lo[threadIdx.x] = be >> 32;
            st->maxkey[threadIdx.x] = hd->maxkey[threadIdx.x];
        }
    }
    const int nsub = 1 << sd.nsub_log2;
    for (int i = threadIdx.x; i < nsub; i += FSC_THREADS) lsub[i] = 0;
    if (threadIdx.x == 0) s_any = 0;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, hl = lane >> 5, wj = lane & 31;
    const int s0 = ((int)blockIdx.x - sd.blk_begin) * FSC_SLOTS + wv * FSC_SPW;
    const int ns = max(0, min(FSC_SPW, seg_fsl_n(sd) - s0)); /* this wave's slots (uniform) */
    const uint32_t* base = seg_fsl(sd) + FSL_HDR_WORDS + (int64_t)s0 * FSL_WORDS;
    uint32_t w[FSC_NP];
#pragma unroll
    for (int p = 0; p < FSC_NP; ++p) w[p] = 2 * p + hl < ns ? base[(int64_t)(2 * p + hl) * FSL_WORDS + wj] : 0u;
    const uint32_t kl = hd->kl, sh = hd->shift;
    uint32_t keep = 0, ext = 0; /* bit p: this lane's first-line word of pair p is a key; pair p has a second line */
#pragma unroll
    for (int p = 0; p < FSC_NP; ++p) {
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)w[p], 0), c1 = (uint32_t)__builtin_amdgcn_readlane((int)w[p], 32);
        const uint32_t c = min(hl ? c1 : c0, (uint32_t)FSL_KEYS);
        if (2 * p + hl < ns && wj >= 1 && (uint32_t)wj <= c) keep |= 1u << p;
        if (max(c0, c1) > 31u) ext |= 1u << p; /* uniform */
    }
    /* a second-line word: key 31 + wj of its slot, kept when 32 + wj <= the count */
    auto second = [&](int p, uint32_t* kv) {
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)w[p], 0), c1 = (uint32_t)__builtin_amdgcn_readlane((int)w[p], 32);
        const uint32_t c = min(hl ? c1 : c0, (uint32_t)FSL_KEYS);
        const bool ok = 2 * p + hl < ns && (uint32_t)(32 + wj) <= c;
        *kv = ok ? base[(int64_t)(2 * p + hl) * FSL_WORDS + 32 + wj] : 0u;
        return ok;
    };
    /* a key's bucket; a key outside the window's buckets (never written by the forward, which
     * stores only inside keys) would mean a stale slot: dropped, and the segment retried */
    bool bad = false;
    auto bucket = [&](uint32_t k, uint32_t* b) {
        *b = (k - kl - 1) >> sh;
        const bool ok = *b < (uint32_t)nsub;
        bad = bad || !ok;
        return ok;
    };
    __syncthreads(); /* lsub cleared */
    if (keep || ext) {
        uint32_t b;
#pragma unroll
        for (int p = 0; p < FSC_NP; ++p)
            if (((keep >> p) & 1u) && bucket(w[p], &b)) atomicAdd(&lsub[b], 1u);
        for (uint32_t m = ext; m; m &= m - 1) { /* rare: a slot with more than 31 keys */
            uint32_t kv;
            if (second(__builtin_ctz(m), &kv) && bucket(kv, &b)) atomicAdd(&lsub[b], 1u);
        }
        if (keep) s_any = 1;
        if (bad) atomicOr(&st->overflow, 1u);
    }
    __syncthreads();
    if (!s_any && !__syncthreads_or(ext != 0)) goto done; /* uniform: no key in this block */
    {   /* one contiguous run per non-empty bucket (one returning atomic per bucket, all in flight) */
        constexpr int PER = NSUB_MAX / FSC_THREADS;
        uint32_t cj[PER], rj[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) cj[j] = (j * FSC_THREADS + (int)threadIdx.x < nsub) ? lsub[j * FSC_THREADS + threadIdx.x] : 0u;
#pragma unroll
        for (int j = 0; j < PER; ++j) rj[j] = cj[j] ? atomicAdd(&st->sub[j * FSC_THREADS + threadIdx.x], cj[j]) : 0u;
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if (j * FSC_THREADS + (int)threadIdx.x < nsub) { lbase[j * FSC_THREADS + threadIdx.x] = rj[j]; lsub[j * FSC_THREADS + threadIdx.x] = 0; }
    }
    __syncthreads();
    {
        const int64_t bcap = sd.bucket_cap;
        uint32_t* out = cand + sd.cand_off;
        auto put = [&](uint32_t k) {
            const uint32_t b = (k - kl - 1) >> sh;
            if (b >= (uint32_t)nsub) return;
            const uint32_t at = lbase[b] + atomicAdd(&lsub[b], 1u);
            if (at < bcap) out[(int64_t)b * bcap + at] = k; /* counted beyond capacity: the select sees it */
        };
#pragma unroll
        for (int p = 0; p < FSC_NP; ++p)
            if ((keep >> p) & 1u) put(w[p]);
        for (uint32_t m = ext; m; m &= m - 1) {
            uint32_t kv;
            if (second(__builtin_ctz(m), &kv)) put(kv);
        }
    }
done:
    __syncthreads(); /* every wave has read the parity */
    if (threadIdx.x == 0) {
        BarState* br = bar_region(head, q);
        const uint32_t shd = blockIdx.x & (NSHARD - 1);
        const uint32_t nsh = (gridDim.x - shd + NSHARD - 1) / NSHARD;
        const uint32_t nact = min((uint32_t)NSHARD, gridDim.x);
        if (atomicAdd(&br->arrive[shd][0], 1u) == nsh - 1u && atomicAdd(&br->arrive[0][16], 1u) == nact - 1u)
            head->parity = q + 1u;
    }
}

/* ---------------------------------------------------------- k_mask_select --- */
/* The select and the level-0 mask in one launch.  Every block resolves its segment's
 * threshold itself from k_collect's counters and the one or two buckets holding the ranks
 * (a few thousand keys, read from L2), then streams its chunk: where(|x| < thr, 0, x).  The segment's first block also computes the exact zero count and
 * publishes the result record and the per-tensor threshold (read by the inverse transform).
 * A DWT segment needs one select (its first block), not one per chunk. */
constexpr int MS_STAGE = 4096;
__global__ __launch_bounds__(STREAM_THREADS) void k_mask_select(SegTable t, const SelHeader* __restrict__ head,
                                                                const uint32_t* __restrict__ cand,
                                                                wtp_result* __restrict__ res,
                                                                float* __restrict__ thr_out) {
    __shared__ uint32_t stage[MS_STAGE];
    const int si = find_seg(t, blockIdx.x);
    const SegDesc& sd = t.s[si];
    const int64_t base = (int64_t)(blockIdx.x - sd.blk_begin) * CHUNK;
    const bool masked = (sd.flags & SEG_MASK) != 0;
    if (!masked && base != 0) return; /* block-uniform */
    if (t.retry && res[sd.res].path != MODE_RETRY) return;
    const int len = (int)min((int64_t)CHUNK, sd.n - base);
    const bool full = (sd.flags & SEG_ALIGNED) && len == CHUNK;
    /* the select first: loads return in issue order (vmcnt), so chunk loads issued ahead of
     * the select's would only delay its round trips -- and the chunk's 64 registers would sit
     * live through it */
    const SelState* st = sel_region(const_cast<SelHeader*>(head), head->parity ^ 1u) + sd.slot;
    int path = 0;
    const float thr = select_body<STREAM_THREADS>(sd, st, cand, res, thr_out, stage, MS_STAGE, base == 0, st->kl,
                                                  st->kh, st->shift, &path);
    if (!masked) return;
    /* a full-scan select reads the whole segment: in place, no block of it may write before
     * every block has scanned -- k_mask_inplace writes it in the next launch */
    if (path == MODE_FULL && sd.data == sd.out) return;
    float4 v[16];
    {
        const float* p = sd.data + base;
        if (full) load_chunk<16>(p, v);
        else load_chunk_ragged<16>(p, len, v);
    }
    float* q = sd.out + base;
    unsigned long long z = 0;
    auto f = [&](float xv) {
        const float y = wt_thr_mask(xv, thr);
        z += y == 0.0f;
        return y;
    };
    if (full) {
        float4* q4 = reinterpret_cast<float4*>(q);
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            float4 y;
            y.x = f(v[it].x); y.y = f(v[it].y); y.z = f(v[it].z); y.w = f(v[it].w);
            q4[it * STREAM_THREADS + threadIdx.x] = y;
        }
    } else {
        const __amdgpu_buffer_rsrc_t r = ragged_rsrc(q, len);
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int e = 4 * (it * STREAM_THREADS + (int)threadIdx.x);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float y = f(f4_get(v[it], c));
                if (e + c >= len) z -= y == 0.0f; /* the zeros read past the end */
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), r, 4 * (e + c), 0, 0);
            }
        }
    }
    if (thr != thr) { /* uniform: a NaN threshold prunes nothing, the copy's zeros are counted */
        const unsigned long long tot = block_sum_u64<STREAM_THREADS>(z);
        if (threadIdx.x == 0 && tot) atomicAdd((unsigned long long*)&res[sd.res].zero_count, tot);
    }
}

/* The in-place segments whose k_mask_select took the full-scan select: the mask pass that
 * k_mask_select skipped for them, with the threshold it published (launched only for groups
 * that hold an in-place level-0 segment; every other block returns at once). */
__global__ __launch_bounds__(STREAM_THREADS) void k_mask_inplace(SegTable t, const wtp_result* __restrict__ res,
                                                                 const float* __restrict__ thr_in) {
    const int si = find_seg(t, blockIdx.x);
    const SegDesc& sd = t.s[si];
    if (!(sd.flags & SEG_MASK) || sd.data != sd.out || res[sd.res].path != MODE_FULL) return;
    const int64_t base = (int64_t)(blockIdx.x - sd.blk_begin) * CHUNK;
    const int len = (int)min((int64_t)CHUNK, sd.n - base);
    const float thr = thr_in[sd.res];
    if ((sd.flags & SEG_ALIGNED) && len == CHUNK) (void)mask_body<true>(sd, base, len, thr);
    else (void)mask_body<false>(sd, base, len, thr);
}

/* -------------------------------------------------------- min-weight pruning --- */
/* percentage_min_pruning (ResNet/min_weight_pruning.py:66-74): zero the k smallest |w| of each
 * tensor.  The rank-(k-1) key t comes from the same window / collect / select machinery
 * (r0 = k-1, gamma 0).  Every |w| < t is pruned; of the |w| == t the lowest flat indices go
 * first until k are pruned (torch.topk's order among ties is unspecified).
 *   k_minsel   one block per segment: the exact t, and need = k - #(|w| < t)
 *   k_tiecount one block per chunk: #(|w| == t) in the chunk
 *   k_minmask  one block per chunk: its ties' global order = the counts of the segment's
 *              earlier chunks + an in-block scan in flat-index order; writes out, counts zeros */
struct MinPrune {
    uint32_t tkey;   /* |w| bit pattern of t (k = 0: 0, with need 0 nothing is pruned) */
    uint32_t pad;
    int64_t need;    /* ties to prune (lowest indices first) */
};

__global__ __launch_bounds__(STREAM_THREADS) void k_minsel(SegTable t, const SelHeader* __restrict__ head,
                                                           const uint32_t* __restrict__ cand,
                                                           wtp_result* __restrict__ res, float* __restrict__ thr_out,
                                                           MinPrune* __restrict__ mp) {
    __shared__ uint32_t stage[4096];
    const SegDesc& sd = t.s[blockIdx.x];
    const SelState* st = sel_region(const_cast<SelHeader*>(head), head->parity ^ 1u) + sd.slot;
    const int64_t k = (sd.flags & SEG_KZERO) ? 0 : sd.r0 + 1;
    float thr = 0.0f;
    if (k > 0) thr = select_body<STREAM_THREADS>(sd, st, cand, res, thr_out, stage, 4096, true, st->kl, st->kh, st->shift);
    __syncthreads();
    if (threadIdx.x == 0) {
        wtp_result& r = res[sd.res];
        MinPrune m;
        m.pad = 0;
        if (k > 0) {
            m.tkey = __float_as_uint(thr) & 0x7FFFFFFFu;
            m.need = k - r.zero_count; /* select_body left #(|w| < t) there */
        } else { /* nothing to prune */
            r.numel = sd.numel;
            r.coeff_numel = sd.n;
            r.thr64 = 0.0;
            r.thr32_bits = 0;
            r.max_abs_bits = 0;
            r.eff_level = 0;
            r.path = MODE_WINDOW;
            m.tkey = 0; /* no key is below 0, and no tie is pruned */
            m.need = 0;
        }
        r.zero_count = 0; /* k_minmask adds the zeros it writes */
        mp[sd.res] = m;
    }
}

__global__ __launch_bounds__(STREAM_THREADS) void k_tiecount(SegTable t, const MinPrune* __restrict__ mp,
                                                             uint32_t* __restrict__ tiecnt) {
    const int si = find_seg(t, blockIdx.x);
    const SegDesc& sd = t.s[si];
    const MinPrune m = mp[sd.res];
    const int64_t base = (int64_t)(blockIdx.x - sd.blk_begin) * CHUNK;
    const int len = (int)min((int64_t)CHUNK, sd.n - base);
    uint32_t c = 0;
    if (m.need > 0) { /* block-uniform */
        float4 v[16];
        if ((sd.flags & SEG_ALIGNED) && len == CHUNK) load_chunk<16>(sd.data + base, v);
        else load_chunk_ragged<16>(sd.data + base, len, v);
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int e = 4 * (it * STREAM_THREADS + (int)threadIdx.x);
#pragma unroll
            for (int q = 0; q < 4; ++q) c += (e + q < len) && abs_key(f4_get(v[it], q)) == m.tkey;
        }
    }
    const unsigned long long tot = block_sum_u64<STREAM_THREADS>(c);
    if (threadIdx.x == 0) tiecnt[blockIdx.x] = (uint32_t)tot;
}

__global__ __launch_bounds__(STREAM_THREADS) void k_minmask(SegTable t, const MinPrune* __restrict__ mp,
                                                            const uint32_t* __restrict__ tiecnt,
                                                            wtp_result* __restrict__ res) {
    __shared__ uint32_t wsum[STREAM_THREADS / 64];
    __shared__ int64_t s_off;
    const int si = find_seg(t, blockIdx.x);
    const SegDesc& sd = t.s[si];
    const MinPrune m = mp[sd.res];
    const int64_t base = (int64_t)(blockIdx.x - sd.blk_begin) * CHUNK;
    const int len = (int)min((int64_t)CHUNK, sd.n - base);
    const bool full = (sd.flags & SEG_ALIGNED) && len == CHUNK;
    float4 v[16];
    if (full) load_chunk<16>(sd.data + base, v);
    else load_chunk_ragged<16>(sd.data + base, len, v);
    /* ties of the segment's earlier chunks */
    const bool ties = m.need > 0 && tiecnt[blockIdx.x] > 0; /* block-uniform */
    if (ties && threadIdx.x < 64) {
        unsigned long long a = 0;
        for (int b = sd.blk_begin + (int)threadIdx.x; b < (int)blockIdx.x; b += 64) a += tiecnt[b];
        a = wave_sum_u64(a);
        if (threadIdx.x == 0) s_off = (int64_t)a;
    }
    __syncthreads();
    int64_t run = ties ? s_off : 0; /* ties before the current it-row */
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long z = 0;
    auto prune = [&](uint32_t k, int64_t rank) { return k < m.tkey || (k == m.tkey && rank < m.need); };
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int e = 4 * (it * STREAM_THREADS + (int)threadIdx.x);
        float4 y = v[it];
        if (ties) { /* flat-index order inside the block: it-row, then thread, then component */
            uint32_t c = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) c += (e + q < len) && abs_key(f4_get(v[it], q)) == m.tkey;
            const uint32_t incl = wave_scan_u32(c);
            if (lane == 63) wsum[wv] = incl;
            __syncthreads();
            int64_t before = run + (incl - c);
            uint32_t rowtot = 0;
            for (int w = 0; w < STREAM_THREADS / 64; ++w) {
                if (w < wv) before += wsum[w];
                rowtot += wsum[w];
            }
            __syncthreads();
            run += rowtot;
            float* yy = reinterpret_cast<float*>(&y);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t k = abs_key(yy[q]);
                if (prune(k, before)) yy[q] = 0.0f;
                before += (e + q < len) && k == m.tkey;
            }
        } else {
            float* yy = reinterpret_cast<float*>(&y);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (abs_key(yy[q]) < m.tkey) yy[q] = 0.0f;
        }
        v[it] = y;
#pragma unroll
        for (int q = 0; q < 4; ++q) z += (e + q < len) && f4_get(y, q) == 0.0f;
    }
    float* q = sd.out + base;
    if (full) {
        float4* q4 = reinterpret_cast<float4*>(q);
#pragma unroll
        for (int it = 0; it < 16; ++it) q4[it * STREAM_THREADS + threadIdx.x] = v[it];
    } else {
        const __amdgpu_buffer_rsrc_t r = ragged_rsrc(q, len);
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int e = 4 * (it * STREAM_THREADS + (int)threadIdx.x);
#pragma unroll
            for (int c = 0; c < 4; ++c) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(f4_get(v[it], c)), r, 4 * (e + c), 0, 0);
        }
    }
    const unsigned long long tot = block_sum_u64<STREAM_THREADS>(z);
    if (threadIdx.x == 0 && tot) atomicAdd((unsigned long long*)&res[sd.res].zero_count, tot);
}

/* ---------------------------------------------------------------- launchers --- */
static int collect_blocks(const SegTable& t) { return t.nblk * (CHUNK / (COLLECT_IT * COLLECT_THREADS * 4)); }
static bool window_inline(const SegTable& t) { return collect_blocks(t) <= WINDOW_INLINE_MAX_BLOCKS; }
void launch_window(const SegTable& t, SelHeader* head, hipStream_t s, const wtp_result* res) {
    if (!window_inline(t)) hipLaunchKernelGGL(k_window, dim3(t.nseg), dim3(WIN_THREADS), 0, s, t, head, res);
}
void launch_fused_retry(const SegTable& t, SelHeader* head, uint32_t* cand, wtp_result* res, float* thr_out,
                        hipStream_t s) {
    hipLaunchKernelGGL(k_window, dim3(t.nseg), dim3(WIN_THREADS), 0, s, t, head, (const wtp_result*)res);
    const int total = collect_blocks(t);
    hipLaunchKernelGGL((k_collect_retry<COLLECT_THREADS, COLLECT_IT>), dim3(total < 512 ? total : 512), dim3(COLLECT_THREADS), 0,
                       s, t, head, cand, res);
    launch_mask_select(t, head, cand, res, thr_out, s);
}
void launch_collect(const SegTable& t, SelHeader* head, uint32_t* cand, wtp_result* res, hipStream_t s) {
    if (window_inline(t))
        hipLaunchKernelGGL((k_collect_t<COLLECT_THREADS, COLLECT_IT, true>), dim3(collect_blocks(t)),
                           dim3(COLLECT_THREADS), 0, s, t, head, cand, res);
    else
        hipLaunchKernelGGL((k_collect_t<COLLECT_THREADS, COLLECT_IT, false>), dim3(collect_blocks(t)),
                           dim3(COLLECT_THREADS), 0, s, t, head, cand, res);
}
void launch_fwin(const FwinTable& t, SelHeader* head, hipStream_t s) {
    const dim3 g(t.nseg * FWIN_NP), b(FWIN_THREADS);
    switch (t.F) {
    case 2: hipLaunchKernelGGL(k_fwin<2>, g, b, 0, s, t, head); break;
    case 4: hipLaunchKernelGGL(k_fwin<4>, g, b, 0, s, t, head); break;
    case 6: hipLaunchKernelGGL(k_fwin<6>, g, b, 0, s, t, head); break;
    case 8: hipLaunchKernelGGL(k_fwin<8>, g, b, 0, s, t, head); break;
    case 10: hipLaunchKernelGGL(k_fwin<10>, g, b, 0, s, t, head); break;
    case 12: hipLaunchKernelGGL(k_fwin<12>, g, b, 0, s, t, head); break;
    case 16: hipLaunchKernelGGL(k_fwin<16>, g, b, 0, s, t, head); break;
    case 18: hipLaunchKernelGGL(k_fwin<18>, g, b, 0, s, t, head); break;
    default: break; /* the host fuses only k_fwd_int's filters */
    }
}
void launch_fslot_collect(const SegTable& t, SelHeader* head, uint32_t* cand, wtp_result* res, hipStream_t s) {
    hipLaunchKernelGGL(k_fslot_collect, dim3(t.nblk), dim3(FSC_THREADS), 0, s, t, head, cand, res);
}
void launch_minprune(const SegTable& t, SelHeader* head, const uint32_t* cand, wtp_result* res, float* thr_out,
                     void* mp, uint32_t* tiecnt, hipStream_t s) {
    hipLaunchKernelGGL(k_minsel, dim3(t.nseg), dim3(STREAM_THREADS), 0, s, t, head, cand, res, thr_out,
                       reinterpret_cast<MinPrune*>(mp));
    hipLaunchKernelGGL(k_tiecount, dim3(t.nblk), dim3(STREAM_THREADS), 0, s, t, reinterpret_cast<const MinPrune*>(mp),
                       tiecnt);
    hipLaunchKernelGGL(k_minmask, dim3(t.nblk), dim3(STREAM_THREADS), 0, s, t, reinterpret_cast<const MinPrune*>(mp),
                       tiecnt, res);
}
void launch_mask_select(const SegTable& t, SelHeader* head, const uint32_t* cand, wtp_result* res, float* thr_out,
                        hipStream_t s) {
    bool masked = false;
    for (int i = 0; i < t.nseg; ++i) masked = masked || (t.s[i].flags & SEG_MASK);
    if (masked) {
        hipLaunchKernelGGL(k_mask_select, dim3(t.nblk), dim3(STREAM_THREADS), 0, s, t, head, cand, res, thr_out);
        return;
    }
    /* no segment to mask (the DWT segments: the inverse thresholds on load): only the select of
     * each segment's first block runs, so the grid is one block per segment */
    SegTable d = t;
    for (int i = 0; i < t.nseg; ++i) d.s[i].blk_begin = d.blk_begin[i] = i;
    d.nblk = t.nseg;
    hipLaunchKernelGGL(k_mask_select, dim3(d.nblk), dim3(STREAM_THREADS), 0, s, d, head, cand, res, thr_out);
}
void launch_mask_inplace(const SegTable& t, const wtp_result* res, const float* thr, hipStream_t s) {
    hipLaunchKernelGGL(k_mask_inplace, dim3(t.nblk), dim3(STREAM_THREADS), 0, s, t, res, thr);
}

}  // namespace wtp

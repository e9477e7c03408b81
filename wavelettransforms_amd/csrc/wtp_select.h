/*
 * wtp_select.h -- device templates of the windowed selection that more than one kernel family
 * uses: the sample and window searches, the radix / wave / histogram selects, select_body (a
 * segment's threshold from its counters and buckets) and mask_body (the level-0 mask of a chunk).
 */
#ifndef WTP_SELECT_H
#define WTP_SELECT_H
#include "wtp_device.h"

#pragma clang fp contract(off)

namespace wtp {

/* ------------------------------------------------------------ the window --- */
/* The selection window of a segment comes from a deterministic sample: MS keys in groups of
 * SAMPLE_GROUP contiguous floats spread evenly over the segment (the whole segment when
 * n <= MS).  Every block of the segment draws the same sample and so derives the same window,
 * which lets each k_collect block compute it for itself instead of waiting for a launch. */
template <int THREADS, int MS>
__device__ __forceinline__ void sample_keys(const SegDesc& sd, uint32_t (&k)[MS / THREADS]) {
    constexpr int PER = MS / THREADS;
    const int64_t n = sd.n;
    const bool exact = n <= MS;
    const double step = exact ? 0.0 : (double)(n - SAMPLE_GROUP) / (double)(MS / SAMPLE_GROUP - 1);
    /* all loads unconditional and issued before any use (indices clamped) */
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = j * THREADS + threadIdx.x;
        const int64_t pos = exact ? min((int64_t)i, n - 1)
                                  : (int64_t)((double)(i / SAMPLE_GROUP) * step) + (i % SAMPLE_GROUP);
        k[j] = abs_key(sd.data[pos]);
    }
}

/* LDS scratch of window_from_keys: the bin histogram plus a few words */
template <int THREADS>
struct WindowLds {
    static constexpr int FBP = (NB + THREADS - 1) / THREADS; /* bins per thread */
    uint32_t h[FBP * THREADS];
    uint32_t wtot[THREADS / 64];
    int found[2];
};

/* Histogram the sampled keys over the NB bins, locate the sample ranks bracketing r0 and r1
 * (6 sigma + 24 sample ranks of margin; exact ranks for a fully sampled segment) and return
 * the window: kl = low edge of the bin of the lower bracket (0: open), kh = high edge of the
 * bin of the upper bracket (0xFFFFFFFF: open), and the bucket shift for nsub buckets. */
template <int THREADS, int MS>
__device__ __forceinline__ void window_search(const SegDesc& sd, WindowLds<THREADS>& L, uint32_t* kl_out,
                                              uint32_t* kh_out, uint32_t* sh_out);
template <int THREADS, int MS>
__device__ __forceinline__ void window_from_keys(const SegDesc& sd, const uint32_t (&k)[MS / THREADS],
                                                 WindowLds<THREADS>& L, uint32_t* kl_out, uint32_t* kh_out,
                                                 uint32_t* sh_out) {
    constexpr int PER = MS / THREADS, FBP = WindowLds<THREADS>::FBP;
    const int64_t n = sd.n;
    const bool exact = n <= MS;
    const int m = exact ? (int)n : MS;
    for (int i = threadIdx.x; i < FBP * THREADS; i += THREADS) L.h[i] = 0;
    if (threadIdx.x < 2) L.found[threadIdx.x] = -1;
    __syncthreads();
    WTP_WPROBE(0);
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (j * THREADS + (int)threadIdx.x < m) atomicAdd(&L.h[key_bin(k[j])], 1u);
    __syncthreads();
    WTP_WPROBE(1);
    window_search<THREADS, MS>(sd, L, kl_out, kh_out, sh_out);
}

/* the search half: L.h holds the histogram of the MS sampled keys (all n when n <= MS) */
template <int THREADS, int MS>
__device__ __forceinline__ void window_search(const SegDesc& sd, WindowLds<THREADS>& L, uint32_t* kl_out,
                                              uint32_t* kh_out, uint32_t* sh_out) {
    constexpr int FBP = WindowLds<THREADS>::FBP;
    const int64_t n = sd.n;
    const bool exact = n <= MS;
    const int m = exact ? (int)n : MS;
    /* sample ranks fit 32 bits; the bin counts stay in registers from the scan to the search */
    const int64_t r0 = sd.r0, r1 = sd.above ? sd.r0 : sd.r0 + 1;
    int sa, sb;
    if (exact) {
        sa = (int)r0;
        sb = (int)r1;
    } else {
        const double p = (double)r0 / (double)(n - 1);
        const double s0 = p * (double)(m - 1), s1 = (double)r1 / (double)(n - 1) * (double)(m - 1);
        const double d = 6.0 * sqrt((double)m * p * (1.0 - p)) + 24.0;
        sa = (int)floor(s0 - d);
        sb = (int)ceil(s1 + d);
    }
    uint32_t c[FBP];
#pragma unroll
    for (int j = 0; j < FBP; ++j) c[j] = L.h[threadIdx.x * FBP + j];
    uint32_t local = 0;
#pragma unroll
    for (int j = 0; j < FBP; ++j) local += c[j];
    const uint32_t incl = wave_scan_u32(local);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 63) L.wtot[wv] = incl;
    __syncthreads();
    WTP_WPROBE(2);
    int cum = (int)(incl - local);
#pragma unroll
    for (int i = 0; i < THREADS / 64; ++i) cum += i < wv ? (int)L.wtot[i] : 0;
    if (sa >= cum || sb >= cum) { /* only threads at or below the ranks search their bins */
#pragma unroll
        for (int j = 0; j < FBP; ++j) {
            const int nx = cum + (int)c[j];
            if (sa >= cum && sa < nx) L.found[0] = threadIdx.x * FBP + j;
            if (sb >= cum && sb < nx) L.found[1] = threadIdx.x * FBP + j;
            cum = nx;
        }
    }
    __syncthreads();
    WTP_WPROBE(3);
    const int f0 = L.found[0], f1 = L.found[1];
    const uint32_t kl = (sa < 0 || f0 < 0) ? 0u : bin_lo_key(f0);
    const uint32_t kh = (sb >= m || f1 < 0) ? 0xFFFFFFFFu : bin_hi_key(f1);
    uint32_t sh = 0;
    if (kh > kl + 1) {
        const uint32_t R = kh - kl - 1; /* inside keys kl < key <= kh: (key - kl - 1) in [0, R] */
        const int bits = 32 - __clz(R);
        sh = bits > sd.nsub_log2 ? bits - sd.nsub_log2 : 0;
    }
    *kl_out = kl;
    *kh_out = kh;
    *sh_out = sh;
}


/* window_from_keys for ONE wave (64 threads, no block barrier: the other waves of the block
 * are elsewhere).  Lane l owns the FBP consecutive bins from l * FBP (stride FBP odd: no bank
 * conflicts); the lane whose run holds a sample rank walks it. */
/* The search half of window_from_keys for ONE wave (no block barrier: the other waves are
 * issuing their loads meanwhile), over the block's histogram h of the MS sampled keys (NB bins)
 * and its coarse companion hc (bins of 128: WCB of them): one scan over the coarse bins finds
 * the 128 fine bins holding a sample rank, one more scan over those finds the bin. */
constexpr int WCB = (NB + 127) / 128; /* 33 <= 64 */
__device__ __forceinline__ int wave_find_bin(const uint32_t* h, const uint32_t* hc, int r) {
    const int lane = threadIdx.x & 63;
    if (r < 0) return -1;
    const uint32_t c = lane < WCB ? hc[lane] : 0u;
    const uint32_t incl = wave_scan_u32(c);
    const uint64_t m = __ballot((int)(incl - c) <= r && r < (int)incl);
    if (!m) return -1;
    const int cb = __ffsll((unsigned long long)m) - 1;
    const int before = __builtin_amdgcn_readlane((int)(incl - c), cb);
    const int b0 = cb * 128 + 2 * lane;
    const uint32_t f0 = b0 < NB ? h[b0] : 0u, f1 = b0 + 1 < NB ? h[b0 + 1] : 0u;
    const uint32_t s2 = f0 + f1;
    const int i2 = before + (int)wave_scan_u32(s2);
    const int e2 = i2 - (int)s2;
    const uint64_t m2 = __ballot(e2 <= r && r < i2);
    const int L = __ffsll((unsigned long long)m2) - 1;
    const int pick = (r < e2 + (int)f0) ? b0 : b0 + 1;
    return __builtin_amdgcn_readlane(pick, L);
}

template <int MS>
__device__ __forceinline__ void window_search_wave(const SegDesc& sd, const uint32_t* h, const uint32_t* hc,
                                                   uint32_t* kl_out, uint32_t* kh_out, uint32_t* sh_out,
                                                   double sig = 6.0, double add = 24.0) {
    const int64_t n = sd.n;
    const bool exact = n <= MS;
    const int m = exact ? (int)n : MS;
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
    const int f0 = wave_find_bin(h, hc, sa);
    const int f1 = sb < m ? wave_find_bin(h, hc, sb) : -1;
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

/* ------------------------------------------------------------- the select --- */
/* Radix select of ranks ra / rb among keys that all lie in [lo, hi]: the bits above the
 * highest bit where lo and hi differ are common and skipped (concentrated digits are what
 * makes an MSB-first LDS histogram contend). */
template <int THREADS, class Get, class Keep>
__device__ void select_in_range(const Get& get, const Keep& keep, int64_t m, uint32_t lo, uint32_t hi, int64_t ra,
                                int64_t rb, bool need_a, bool need_b, uint32_t* ka, uint32_t* kb) {
    __shared__ uint32_t ha[256], hb[256];
    __shared__ int dsel[2];
    __shared__ int64_t bsel[2];
    const uint32_t diff = lo ^ hi;
    int top = diff ? 31 - __clz(diff) : -1; /* highest unknown bit */
    const uint32_t known = top >= 31 ? 0u : (top < 0 ? 0xFFFFFFFFu : ~((2u << top) - 1u)); /* lo == hi: every bit */
    uint32_t pa = lo & known, pb = lo & known, mask = known;
    while (top >= 0) {
        const int width = top + 1 < 8 ? top + 1 : 8;
        const int shift = top + 1 - width;
        const uint32_t dm = (1u << width) - 1u;
        for (int i = threadIdx.x; i < 256; i += THREADS) { ha[i] = 0; hb[i] = 0; }
        __syncthreads();
        for (int64_t i = threadIdx.x; i < m; i += THREADS) {
            const uint32_t k = get(i);
            if (!keep(k)) continue;
            const uint32_t d = (k >> shift) & dm;
            if (need_a && (k & mask) == pa) atomicAdd(&ha[d], 1u);
            if (need_b && (k & mask) == pb) atomicAdd(&hb[d], 1u);
        }
        __syncthreads();
        const int wv = threadIdx.x >> 6;
        if (wv == 0 && need_a) wave_pick_digit(ha, ra, &dsel[0], &bsel[0]);
        if (wv == 1 && need_b) wave_pick_digit(hb, rb, &dsel[1], &bsel[1]);
        __syncthreads();
        if (need_a) { pa |= (uint32_t)dsel[0] << shift; ra -= bsel[0]; }
        if (need_b) { pb |= (uint32_t)dsel[1] << shift; rb -= bsel[1]; }
        mask |= dm << shift;
        top = shift - 1;
        __syncthreads();
    }
    *ka = pa;
    *kb = pb;
}

/* Rank r (0-based, ascending) among the m <= 64*KPL keys stage[0..m), all in [lo, hi]; one
 * wave, keys in registers.  Bit by bit below the common prefix of lo and hi, the result takes a
 * bit when at most r keys lie below it: it ends at the largest t with #(key < t) <= r, which is
 * the r-th key itself.  Every lane of the wave must be active. */
constexpr int WSEL_KPL = 16;
constexpr int STAGE_BATCH = 4;
template <int KPL>
__device__ __forceinline__ uint32_t wave_select_rank(const uint32_t* stage, int m, int64_t r, uint32_t lo, uint32_t hi) {
    const int lane = threadIdx.x & 63;
    uint32_t k[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int i = j * 64 + lane;
        k[j] = i < m ? stage[i] : 0xFFFFFFFFu; /* above every |x| key */
    }
    const uint32_t diff = lo ^ hi;
    const int top = diff ? 31 - __clz(diff) : -1;
    uint32_t res = top >= 31 ? 0u : (top < 0 ? lo : (lo & ~((2u << top) - 1u))); /* lo == hi: the key itself */
    const uint32_t rr = (uint32_t)r; /* r < m */
    for (int b = top; b >= 0; --b) {
        const uint32_t cand = res | (1u << b);
        uint32_t c = 0; /* counted on the scalar unit: compare masks and popcounts, no DPP chain */
#pragma unroll
        for (int j = 0; j < KPL; ++j) c += (uint32_t)__popcll(__ballot(k[j] < cand));
        if (c <= rr) res = cand;
    }
    return res;
}

/* Ranks ra / rb among the m keys stage[0..m), all in [lo, lo + W), W <= HS_PER * THREADS:
 * one LDS histogram over the W key values, a block scan of per-thread runs of HS_PER bins kept
 * in registers, and the thread whose run holds a rank names its key.  out[] and wt[] are LDS. */
constexpr int HS_PER = 16;
template <int THREADS>
__device__ __forceinline__ void block_hist_select(const uint32_t* stage, int m, uint32_t lo, int W, int ra, int rb,
                                                  uint32_t* hist, uint32_t* out, uint32_t* wt) {
    const int per = (W + THREADS - 1) / THREADS;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    for (int i = tid; i < per * THREADS; i += THREADS) hist[i] = 0;
    __syncthreads();
    WTP_PROBE_T(12, 0);
    for (int i = tid; i < m; i += THREADS) atomicAdd(&hist[stage[i] - lo], 1u);
    __syncthreads();
    WTP_PROBE_T(13, 0);
    uint32_t c[HS_PER];
    uint32_t local = 0;
#pragma unroll
    for (int j = 0; j < HS_PER; ++j) {
        c[j] = j < per ? hist[tid * per + j] : 0u;
        local += c[j];
    }
    const uint32_t incl = wave_scan_u32(local);
    if (lane == 63) wt[wv] = incl;
    __syncthreads();
    WTP_PROBE_T(14, 0);
    int cum = (int)(incl - local);
#pragma unroll
    for (int i = 0; i < THREADS / 64; ++i) cum += i < wv ? (int)wt[i] : 0;
    if (local && ((ra >= cum && ra < cum + (int)local) || (rb >= cum && rb < cum + (int)local))) {
#pragma unroll
        for (int j = 0; j < HS_PER; ++j) {
            const int nx = cum + (int)c[j];
            if (ra >= cum && ra < nx) out[0] = lo + (uint32_t)(tid * per + j);
            if (rb >= cum && rb < nx) out[1] = lo + (uint32_t)(tid * per + j);
            cum = nx;
        }
    }
    __syncthreads();
}

/* count of keys < tk among get(i), block-wide; valid in every thread */
template <int THREADS, class Get>
__device__ int64_t block_count_below(const Get& get, int64_t m, uint32_t tk) {
    __shared__ unsigned long long acc;
    if (threadIdx.x == 0) acc = 0;
    __syncthreads();
    uint32_t c = 0; /* per thread < 2^32 */
    for (int64_t i = threadIdx.x; i < m; i += THREADS) c += get(i) < tk;
    const unsigned long long w = wave_sum_u64(c);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&acc, w);
    __syncthreads();
    const int64_t r = (int64_t)acc;
    __syncthreads();
    return r;
}

/* The buckets holding ranks ra / rb from the counts in LDS: lane l takes the nsub/64
 * consecutive buckets from l * per (ds_read_b128), one wave scan of the lane sums, a ballot for
 * the lane, then a walk over that lane's buckets.  Writes bucket[i] and before[i] (the keys in
 * the buckets below it). */
__device__ __forceinline__ void wave_find_buckets(const uint32_t* lsub, int nsub, bool need_a, int64_t ra, bool need_b,
                                                  int64_t rb, int* bucket, int64_t* before) {
    const int lane = threadIdx.x & 63;
    const int per = nsub / 64; /* 1..16 */
    uint32_t c[16];
    const uint4* p4 = reinterpret_cast<const uint4*>(lsub + lane * per);
    if (per >= 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 t = q < per / 4 ? p4[q] : make_uint4(0u, 0u, 0u, 0u);
            c[4 * q] = t.x; c[4 * q + 1] = t.y; c[4 * q + 2] = t.z; c[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) c[q] = q < per ? lsub[lane * per + q] : 0u;
    }
    uint32_t s = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += c[q];
    const uint32_t incl = wave_scan_u32(s);
    const int64_t excl = (int64_t)(incl - s);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (!(i == 0 ? need_a : need_b)) continue; /* uniform */
        const int64_t r = i == 0 ? ra : rb;
        const bool hit = excl <= r && r < (int64_t)incl;
        if (hit) { /* one lane: walk its buckets */
            int64_t cum = excl;
            int b = lane * per;
            bool go = true;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                go = go && q < per && r >= cum + (int64_t)c[q];
                if (go) { cum += c[q]; ++b; }
            }
            bucket[i] = b;
            before[i] = cum;
        }
    }
}

/* Resolve the two order statistics of one segment from its counters and buckets, compute the
 * NumPy threshold and the level-0 zero count, publish the results, and leave the slot clean.
 * One block of THREADS threads; `stage` holds up to stage_cap keys in LDS. */
template <int THREADS, bool COH = false>
__device__ float select_body(const SegDesc& sd, const SelState* __restrict__ st, const uint32_t* __restrict__ cand,
                             wtp_result* __restrict__ res, float* __restrict__ thr_out, uint32_t* stage,
                             int stage_cap, bool publish, uint32_t kl, uint32_t kh, uint32_t sh,
                             int* path_out = nullptr, uint32_t* hscratch = nullptr, bool prefer_wave = false) {
    __shared__ int sbin[2];
    __shared__ int64_t sbefore[2];
    __shared__ uint32_t lsub[NSUB_MAX];
    __shared__ unsigned long long s_cnt[4]; /* below, eq_lo, eq_hi (unused: 0), inside */
    __shared__ uint32_t s_mk, s_ovf;
    const int nsub = 1 << sd.nsub_log2;
    const int64_t r0 = sd.r0, r1 = sd.above ? sd.r0 : sd.r0 + 1;
    WTP_PROBE(0);
    /* one round trip: threads 0..4 gather the sharded counters, wave 1 the bucket counts (to LDS) */
    if (threadIdx.x < 64) {
        const int l = threadIdx.x;
        if (l < 3) {
            const unsigned long long* a = l == 0 ? st->below : (l == 1 ? st->eq_lo : st->eq_hi);
            unsigned long long v = 0;
#pragma unroll
            for (int i = 0; i < NSHARD; ++i) v += ldc<COH>(a + i);
            s_cnt[l] = v;
        } else if (l == 3) {
            uint32_t m = 0;
#pragma unroll
            for (int i = 0; i < NSHARD; ++i) m = max(m, ldc<COH>(st->maxkey + i));
            s_mk = m;
        } else if (l == 4) {
            s_ovf = ldc<COH>(&st->overflow);
        }
    }
    /* wave 1: the bucket counts (bucket j * 64 + lane in sv[j]), every load issued before the
     * first is used -- 16 in flight per lane at nsub 1024, not 16 round trips in a row */
    uint32_t sv[NSUB_MAX / 64];
    if (threadIdx.x >= 64 && threadIdx.x < 128) {
        const int l = threadIdx.x - 64;
#pragma unroll
        for (int j = 0; j < NSUB_MAX / 64; ++j) sv[j] = (j * 64 + l < nsub) ? ldc<COH>(st->sub + j * 64 + l) : 0u;
        uint32_t sm = 0;
#pragma unroll
        for (int j = 0; j < NSUB_MAX / 64; ++j) {
            if (j * 64 + l < nsub) lsub[j * 64 + l] = sv[j];
            sm += sv[j];
        }
        sm = wave_sum_u32(sm);
        if (l == 0) s_cnt[3] = sm;
    }
    __syncthreads();
    WTP_PROBE(1);
    const int64_t below = (int64_t)s_cnt[0], eql = (int64_t)s_cnt[1], eqh = (int64_t)s_cnt[2];
    const int64_t ncand = (int64_t)s_cnt[3];
    uint32_t mk = s_mk;
    /* class of a rank: 0 miss, 1 == kl, 2 inside (kl, kh]  (eqh stays 0: keys == kh are inside) */
    auto classify = [&](int64_t r, int64_t* j) {
        if (r < below) return 0;
        r -= below;
        if (r < eql) return 1;
        r -= eql;
        if (r < ncand) { *j = r; return 2; }
        r -= ncand;
        if (r < eqh) return 3;
        return 0;
    };
    int64_t ja = 0, jb = 0;
    const int ca = classify(r0, &ja), cb = classify(r1, &jb);
    const float* x = sd.data;
    const int64_t bcap = sd.bucket_cap;
    const uint32_t* c = cand + sd.cand_off;
    uint32_t ka = 0, kb = 0;
    int path = MODE_WINDOW;
    int64_t nlo = 0, nhi = 0, before = 0;
    int blo = 0, bhi = 0;
    bool in_lds = false;
    bool full = ca == 0 || cb == 0 || s_ovf != 0;
    if (!full && (ca == 2 || cb == 2)) {
        WTP_PROBE_T(8, 64);
        if (threadIdx.x >= 64 && threadIdx.x < 128) /* wave 1: both ranks from one scan */
            wave_find_buckets(lsub, nsub, ca == 2, ja, cb == 2, jb, sbin, sbefore);
        WTP_PROBE_T(9, 64);
        __syncthreads();
        WTP_PROBE(2);
        blo = (ca == 2) ? sbin[0] : sbin[1];
        bhi = (cb == 2) ? sbin[1] : sbin[0];
        before = (ca == 2) ? sbefore[0] : sbefore[1];
        /* adjacent ranks: buckets strictly between blo and bhi are empty */
        nlo = lsub[blo];
        nhi = (bhi != blo) ? lsub[bhi] : 0;
        if (nlo > bcap || nhi > bcap) full = true;
        if (!full) {
            in_lds = nlo + nhi <= stage_cap;
            if (in_lds) { /* STAGE_BATCH loads in flight per thread before any is used */
                const int64_t m = nlo + nhi;
                for (int64_t i0 = 0; i0 < m; i0 += (int64_t)THREADS * STAGE_BATCH) {
                    uint32_t v[STAGE_BATCH];
#pragma unroll
                    for (int j = 0; j < STAGE_BATCH; ++j) {
                        const int64_t i = i0 + (int64_t)j * THREADS + threadIdx.x;
                        v[j] = i < m ? ldc<COH>(i < nlo ? c + (int64_t)blo * bcap + i : c + (int64_t)bhi * bcap + i - nlo)
                                     : 0u;
                    }
#pragma unroll
                    for (int j = 0; j < STAGE_BATCH; ++j) {
                        const int64_t i = i0 + (int64_t)j * THREADS + threadIdx.x;
                        if (i < m) stage[i] = v[j];
                    }
                }
                __syncthreads();
            }
            WTP_PROBE(3);
            const uint64_t lo64 = (uint64_t)kl + 1 + ((uint64_t)blo << sh);
            const uint64_t hi64 = min((uint64_t)kh, (uint64_t)kl + ((uint64_t)(bhi + 1) << sh));
            uint32_t xa = 0, xb = 0;
            const bool wave_ok = in_lds && nlo + nhi <= 64 * WSEL_KPL;
            if (in_lds && hscratch && hi64 - lo64 < (uint64_t)(HS_PER * THREADS) && !(prefer_wave && wave_ok)) {
                /* one LDS histogram over the bucket's key values: both ranks in one pass */
                __shared__ uint32_t sx[2], wt[THREADS / 64];
                block_hist_select<THREADS>(stage, (int)(nlo + nhi), (uint32_t)lo64, (int)(hi64 - lo64 + 1),
                                           (int)(ja - before), (int)(jb - before), hscratch, sx, wt);
                xa = sx[0];
                xb = sx[1];
            } else if (wave_ok) {
                /* a few hundred keys: one wave per rank, a bitwise search in registers */
                __shared__ uint32_t sx[2];
                const int wv = threadIdx.x >> 6;
                if (wv == 0 && ca == 2) {
                    const uint32_t k = wave_select_rank<WSEL_KPL>(stage, (int)(nlo + nhi), ja - before, (uint32_t)lo64, (uint32_t)hi64);
                    if ((threadIdx.x & 63) == 0) sx[0] = k;
                }
                if (wv == 1 && cb == 2) {
                    const uint32_t k = wave_select_rank<WSEL_KPL>(stage, (int)(nlo + nhi), jb - before, (uint32_t)lo64, (uint32_t)hi64);
                    if ((threadIdx.x & 63) == 0) sx[1] = k;
                }
                __syncthreads();
                xa = sx[0];
                xb = sx[1];
            } else {
                auto getb = [&](int64_t i) {
                    return in_lds ? stage[i]
                                  : ldc<COH>(i < nlo ? c + (int64_t)blo * bcap + i : c + (int64_t)bhi * bcap + i - nlo);
                };
                select_in_range<THREADS>(getb, [](uint32_t) { return true; }, nlo + nhi, (uint32_t)lo64,
                                         (uint32_t)hi64, ja - before, jb - before, ca == 2, cb == 2, &xa, &xb);
            }
            ka = (ca == 2) ? xa : (ca == 1 ? kl : kh);
            kb = (cb == 2) ? xb : (cb == 1 ? kl : kh);
            path = MODE_CAND;
            WTP_PROBE(4);
        }
    } else if (!full) {
        ka = (ca == 1) ? kl : kh;
        kb = (cb == 1) ? kl : kh;
    }
    if constexpr (!COH) { /* k_mask_select's select only (k_resident never sees a fused segment) */
        if (full && (sd.flags & SEG_FUSED)) {
            /* a fused segment: its window came from input patches; the retry launches take it
             * again from P (k_window / k_collect) -- nothing is published here */
            if (publish && threadIdx.x == 0) res[sd.res].path = MODE_RETRY;
            __syncthreads();
            return __uint_as_float(0x7FC00000u);
        }
    }
    if (full) {
        /* the window missed (or a block/bucket overflowed): exact radix select over the segment */
        select_in_range<THREADS>([&](int64_t i) { return abs_key(x[i]); }, [](uint32_t) { return true; }, sd.n, 0u,
                                 0xFFFFFFFFu, r0, r1, true, true, &ka, &kb);
        path = MODE_FULL;
    }
    __syncthreads();
    /* threshold: numpy/lib/function_base.py _lerp -- diff in float32, the blend in float64 */
    const float fa = __uint_as_float(ka), fb = __uint_as_float(kb);
    const float diff = fb - fa;
    const double g = sd.gamma;
    double thr = (g >= 0.5) ? (double)fb - (double)diff * (1.0 - g) : (double)fa + (double)diff * g;
    const bool minp = (sd.flags & SEG_MINPRUNE) != 0; /* rank select for min pruning: no NumPy NaN rule */
    if (mk > 0x7F800000u && !minp) thr = __longlong_as_double(0x7FF8000000000000ll); /* NaN present: np.percentile is NaN */
    const float thr32 = (float)thr;
    const bool nan = !minp && thr32 != thr32; /* also inf - inf inside the lerp */
    /* level-0 segments: zeros of where(|x| < thr, 0, x) = #(key < tk) with tk = bits(thr) when
     * thr > 0, else tk = 1 (only the zeros themselves).  ka <= thr <= kb and the two ranks are
     * adjacent, so #(key < tk) = below + [tk > kl] eq_lo + before + #(staged < tk).  A NaN
     * threshold prunes nothing: every k_mask_select block counts the zeros of its copy. */
    WTP_PROBE(5);
    if (path_out) *path_out = path;
    if (!publish) return minp ? __uint_as_float(ka) : thr32; /* block-uniform */
    int64_t zc = 0;
    /* min pruning (k_minsel) wants #(key < t) for the exact key t = ka: none when t == 0 */
    if (((sd.flags & SEG_MASK) || (minp && ka > 0)) && !nan) {
        const uint32_t tk = minp ? ka : (thr32 > 0.0f ? __float_as_uint(thr32) : 1u);
        if (path == MODE_FULL)
            zc = block_count_below<THREADS>([&](int64_t i) { return abs_key(x[i]); }, sd.n, tk);
        else if (path == MODE_CAND)
            zc = below + (tk > kl ? eql : 0) + before +
                 block_count_below<THREADS>(
                     [&](int64_t i) {
                         return in_lds ? stage[i]
                                       : ldc<COH>(i < nlo ? c + (int64_t)blo * bcap + i
                                                          : c + (int64_t)bhi * bcap + i - nlo);
                     },
                     nlo + nhi, tk);
        else
            zc = below + (tk > kl ? eql : 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        thr_out[sd.res] = thr32; /* per tensor: read by the inverse transform */
        wtp_result& r = res[sd.res];
        r.numel = sd.numel;
        r.coeff_numel = sd.n;
        if (minp) r.zero_count = zc; /* k_minsel turns it into the tie budget; k_minmask counts */
        else if (zc) atomicAdd((unsigned long long*)&r.zero_count, (unsigned long long)zc); /* zeroed by k_collect */
        r.thr64 = thr;
        r.thr32_bits = __float_as_uint(thr32);
        r.max_abs_bits = mk;
        r.eff_level = sd.eff_level;
        if constexpr (COH) atomicMax(&r.path, path); /* a timed-out workgroup may raise it to MODE_FAULT */
        else r.path = r.path == MODE_RETRY ? path + MODE_RETRIED : path; /* the fused retry's select */
    }
    WTP_PROBE(6);
    return minp ? __uint_as_float(ka) : thr32;
}

/* out = where(|x| < thr, 0, x) over one chunk; returns the zeros written */
template <bool FULL>
__device__ __forceinline__ unsigned long long mask_body(const SegDesc& sd, int64_t base, int len, float thr) {
    const float* p = sd.data + base;
    float* q = sd.out + base;
    float4 v[16];
    if (FULL) load_chunk<16>(p, v);
    else load_chunk_ragged<16>(p, len, v);
    unsigned long long z = 0;
    auto f = [&](float xv) {
        const float y = wt_thr_mask(xv, thr);
        z += y == 0.0f;
        return y;
    };
    if (FULL) {
        float4* q4 = reinterpret_cast<float4*>(q);
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            float4 y;
            y.x = f(v[it].x); y.y = f(v[it].y); y.z = f(v[it].z); y.w = f(v[it].w);
            q4[it * STREAM_THREADS + threadIdx.x] = y;
        }
    } else {
        /* range-checked stores: writes past len are dropped, no per-store branch */
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
    return z;
}

}  // namespace wtp
#endif

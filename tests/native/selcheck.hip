/*
 * selcheck.hip -- test-only unit: every wave and block step of the exact percentile selection
 * (csrc/wtp_device.h, csrc/wtp_select.h, the window search of csrc/resident.inc and collect_body of
 * csrc/select.inc) behind one small __global__ wrapper each, so tests/test_gpu_select_units.py can
 * hold each step to numpy on the same integers.  An extern "C" entry takes host pointers, copies
 * them to the device, launches once (a wrapper loops over its queries inside the launch),
 * synchronizes, copies back, frees, and returns the HIP error code.  Wave steps run in whole waves
 * with every lane active; block steps run with the THREADS the library instantiates.  Arguments
 * must stay inside each step's documented domain: outside it the steps index LDS out of bounds.
 * tests/selcheck_shim.py builds it with the library's compiler, target and parity flags.
 */
#include "wtp_select.h"
#include "select.inc"
#include "resident.inc"

#include <cstring>
#include <vector>

using namespace wtp;

namespace {

/* device copies of host arrays, freed together; the first HIP error is kept */
struct Arena {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    void note(hipError_t e) { if (err == hipSuccess && e != hipSuccess) err = e; }
    template <class T>
    T* zeros(size_t n) {
        void* d = nullptr;
        const size_t bytes = (n ? n : 1) * sizeof(T);
        note(hipMalloc(&d, bytes));
        if (d) { ptrs.push_back(d); note(hipMemset(d, 0, bytes)); }
        return static_cast<T*>(d);
    }
    template <class T>
    T* up(const T* h, size_t n) {
        T* d = zeros<T>(n);
        if (d && n) note(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <class T>
    void down(T* h, const T* d, size_t n) {
        if (err == hipSuccess && n) note(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
    }
    bool ok() const { return err == hipSuccess; }
    void ran() { note(hipGetLastError()); note(hipDeviceSynchronize()); }
    int finish() {
        for (void* p : ptrs) (void)hipFree(p);
        return (int)err;
    }
};

/* ---------------------------------------------------------------- wave primitives --- */
/* red: per case scan sum, max, min, or (as every lane holds them: lanes 0 and 63 must agree) */
__global__ __launch_bounds__(64) void k_wave_prims(const uint32_t* in, const unsigned long long* in64, int ncase,
                                                  uint32_t* scan, uint32_t* red, unsigned long long* sum64) {
    const int lane = threadIdx.x;
    for (int q = 0; q < ncase; ++q) {
        const uint32_t v = in[q * 64 + lane];
        scan[q * 64 + lane] = wave_scan_u32(v);
        const uint32_t s = wave_sum_u32(v), mx = wave_max_u32(v), mn = wave_min_u32(v), o = wave_or_u32(v);
        const unsigned long long s64 = wave_sum_u64(in64[q * 64 + lane]);
        if (lane == 0 || lane == 63) {
            uint32_t* r = red + (q * 2 + (lane == 63)) * 4;
            r[0] = s; r[1] = mx; r[2] = mn; r[3] = o;
            sum64[q * 2 + (lane == 63)] = s64;
        }
    }
}

__global__ __launch_bounds__(64) void k_pick_digit(const uint32_t* hist, const int64_t* ranks, int nr, int* digit,
                                                  int64_t* below) {
    __shared__ uint32_t h[256];
    for (int i = threadIdx.x; i < 256; i += 64) h[i] = hist[i];
    __syncthreads();
    for (int q = 0; q < nr; ++q) wave_pick_digit(h, ranks[q], digit + q, below + q); /* the hit lane writes */
}

__global__ __launch_bounds__(64) void k_find_bin(const uint32_t* hist, const uint32_t* hcoarse, const int* ranks, int nr,
                                                int* out) {
    __shared__ uint32_t h[NB], hc[WCB];
    for (int i = threadIdx.x; i < NB; i += 64) h[i] = hist[i];
    if (threadIdx.x < WCB) hc[threadIdx.x] = hcoarse[threadIdx.x];
    __syncthreads();
    for (int q = 0; q < nr; ++q) {
        const int b = wave_find_bin(h, hc, ranks[q]);
        if (threadIdx.x == (unsigned)(q & 63)) out[q] = b; /* uniform: any lane may report it */
    }
}

__global__ __launch_bounds__(64) void k_find_bins_flat(const uint32_t* hist, const int* ra, const int* rb, int nr,
                                                      int* fa, int* fb) {
    __shared__ uint32_t h[RES_HBINS];
    for (int i = threadIdx.x; i < RES_HBINS; i += 64) h[i] = i < NB ? hist[i] : 0u;
    __syncthreads();
    for (int q = 0; q < nr; ++q) {
        int a, b;
        wave_find_bins_flat(h, ra[q], rb[q], &a, &b);
        if (threadIdx.x == (unsigned)(q & 63)) { fa[q] = a; fb[q] = b; }
    }
}

/* ------------------------------------------------------------------ window search --- */
struct WinCase {
    int64_t n, r0;
    int32_t above, nsub_log2;
};
__device__ __forceinline__ SegDesc win_desc(const WinCase& c) {
    SegDesc sd = {};
    sd.n = c.n;
    sd.r0 = c.r0;
    sd.above = c.above;
    sd.nsub_log2 = c.nsub_log2;
    return sd;
}
template <int THREADS, int MS>
__global__ __launch_bounds__(THREADS) void k_window_block(const uint32_t* hist, const WinCase* cs, int ncase,
                                                         uint32_t* out) {
    __shared__ WindowLds<THREADS> L;
    for (int i = threadIdx.x; i < WindowLds<THREADS>::FBP * THREADS; i += THREADS) L.h[i] = i < NB ? hist[i] : 0u;
    for (int q = 0; q < ncase; ++q) {
        if (threadIdx.x < 2) L.found[threadIdx.x] = -1; /* as window_from_keys leaves it */
        __syncthreads();
        const SegDesc sd = win_desc(cs[q]);
        uint32_t kl, kh, sh;
        window_search<THREADS, MS>(sd, L, &kl, &kh, &sh);
        if (threadIdx.x == (unsigned)(q % THREADS)) { out[3 * q] = kl; out[3 * q + 1] = kh; out[3 * q + 2] = sh; }
        __syncthreads();
    }
}
template <bool FLAT>
__global__ __launch_bounds__(64) void k_window_wave(const uint32_t* hist, const uint32_t* hcoarse, const WinCase* cs,
                                                   int ncase, uint32_t* out) {
    __shared__ uint32_t h[RES_HBINS], hc[WCB];
    for (int i = threadIdx.x; i < RES_HBINS; i += 64) h[i] = i < NB ? hist[i] : 0u;
    if (threadIdx.x < WCB) hc[threadIdx.x] = hcoarse[threadIdx.x];
    __syncthreads();
    for (int q = 0; q < ncase; ++q) {
        const SegDesc sd = win_desc(cs[q]);
        uint32_t kl, kh, sh;
        if (FLAT) {
            const bool exact = sd.n <= RES_MS;
            window_search_flat(sd, h, exact ? (int)sd.n : RES_MS, exact, &kl, &kh, &sh, 6.0, 24.0);
        } else {
            window_search_wave<M_SAMPLE>(sd, h, hc, &kl, &kh, &sh);
        }
        if (threadIdx.x == (unsigned)(q & 63)) { out[3 * q] = kl; out[3 * q + 1] = kh; out[3 * q + 2] = sh; }
    }
}

__global__ void k_bins(const uint32_t* keys, int nk, int* bin, uint32_t* lo, uint32_t* hi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nk) bin[i] = key_bin(keys[i]);
    if (i < NB) { lo[i] = bin_lo_key(i); hi[i] = bin_hi_key(i); }
}

/* ------------------------------------------------------------------------ selects --- */
__global__ __launch_bounds__(64) void k_wave_select(const uint32_t* keys, int m, uint32_t lo, uint32_t hi,
                                                   uint32_t* out) {
    __shared__ uint32_t stage[64 * WSEL_KPL];
    for (int i = threadIdx.x; i < m; i += 64) stage[i] = keys[i];
    __syncthreads();
    for (int r = 0; r < m; ++r) {
        const uint32_t k = wave_select_rank<WSEL_KPL>(stage, m, r, lo, hi);
        if (threadIdx.x == (unsigned)(r & 63)) out[r] = k;
    }
}

struct RangeQuery {
    int64_t ra, rb;
    int32_t need_a, need_b;
};
__global__ __launch_bounds__(STREAM_THREADS) void k_select_in_range(const uint32_t* keys, int64_t m, uint32_t lo,
                                                                   uint32_t hi, const RangeQuery* qs, int nq,
                                                                   uint32_t* out) {
    for (int q = 0; q < nq; ++q) {
        uint32_t ka, kb;
        select_in_range<STREAM_THREADS>([&](int64_t i) { return keys[i]; }, [](uint32_t) { return true; }, m, lo, hi,
                                        qs[q].ra, qs[q].rb, qs[q].need_a != 0, qs[q].need_b != 0, &ka, &kb);
        if (threadIdx.x == (unsigned)(q % STREAM_THREADS)) { out[2 * q] = ka; out[2 * q + 1] = kb; }
        __syncthreads();
    }
}

/* block_hist_select over stage[0..m) in [lo, lo + W) for nq rank pairs, then block_count_below for nt keys */
__global__ __launch_bounds__(STREAM_THREADS) void k_block_hist(const uint32_t* stage, int m, uint32_t lo, int W,
                                                              const int* ra, const int* rb, int nq, uint32_t* sel,
                                                              const uint32_t* tks, int nt, int64_t* cnt) {
    __shared__ uint32_t hist[HS_PER * STREAM_THREADS], sx[2], wt[STREAM_THREADS / 64];
    for (int q = 0; q < nq; ++q) {
        if (threadIdx.x < 2) sx[threadIdx.x] = 0xFFFFFFFFu;
        __syncthreads();
        block_hist_select<STREAM_THREADS>(stage, m, lo, W, ra[q], rb[q], hist, sx, wt);
        if (threadIdx.x == 0) { sel[2 * q] = sx[0]; sel[2 * q + 1] = sx[1]; }
        __syncthreads();
    }
    for (int q = 0; q < nt; ++q) {
        const int64_t c = block_count_below<STREAM_THREADS>([&](int64_t i) { return stage[i]; }, (int64_t)m, tks[q]);
        if (threadIdx.x == (unsigned)((q * 37) % STREAM_THREADS)) cnt[q] = c; /* valid in every thread */
    }
}

struct BucketQuery {
    int64_t ra, rb;
    int32_t need_a, need_b;
};
__global__ __launch_bounds__(64) void k_find_buckets(const uint32_t* sub, int nsub, const BucketQuery* qs, int nq,
                                                    int* bucket, int64_t* before) {
    __shared__ __attribute__((aligned(16))) uint32_t lsub[NSUB_MAX];
    __shared__ int sbin[2];
    __shared__ int64_t sbefore[2];
    for (int i = threadIdx.x; i < nsub; i += 64) lsub[i] = sub[i];
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        if (threadIdx.x < 2) { sbin[threadIdx.x] = -1; sbefore[threadIdx.x] = -1; }
        __syncthreads();
        wave_find_buckets(lsub, nsub, qs[q].need_a != 0, qs[q].ra, qs[q].need_b != 0, qs[q].rb, sbin, sbefore);
        __syncthreads();
        if (threadIdx.x < 2) { bucket[2 * q + threadIdx.x] = sbin[threadIdx.x]; before[2 * q + threadIdx.x] = sbefore[threadIdx.x]; }
        __syncthreads();
    }
}

/* ------------------------------------------------- select_body and collect_body --- */
/* exactly as k_mask_select calls it: one block, stage_cap = MS_STAGE, COH false */
__global__ __launch_bounds__(STREAM_THREADS) void k_select_body(SegDesc sd, const SelState* st, const uint32_t* cand,
                                                               wtp_result* res, float* thr_out, int publish,
                                                               int use_hscratch, int prefer_wave, float* ret,
                                                               int* path_out) {
    __shared__ uint32_t stage[MS_STAGE];
    __shared__ uint32_t hscratch[HS_PER * STREAM_THREADS];
    int path = 0;
    const float thr = select_body<STREAM_THREADS>(sd, st, cand, res, thr_out, stage, MS_STAGE, publish != 0, st->kl,
                                                  st->kh, st->shift, &path, use_hscratch ? hscratch : nullptr,
                                                  prefer_wave != 0);
    if (threadIdx.x == STREAM_THREADS - 1) { *ret = thr; *path_out = path; } /* block-uniform */
}

/* one chunk as a k_collect_t block without the inline window takes it */
template <bool FULL>
__global__ __launch_bounds__(COLLECT_THREADS) void k_collect_body(SegDesc sd, SelState* st, uint32_t* cand, int len) {
    __shared__ uint32_t lsub[NSUB_MAX];
    __shared__ uint32_t lbase[NSUB_MAX];
    __shared__ uint32_t stage[STG * COLLECT_THREADS];
    __shared__ uint32_t wred[COLLECT_THREADS / 64][4];
    __shared__ int wtot[COLLECT_THREADS / 64];
    collect_body<COLLECT_THREADS, COLLECT_IT, FULL, false>(sd, st, cand, 0, len, true, lsub, lbase, stage, nullptr, wred,
                                                           wtot);
}

/* the window rule's bucket shift (wtp_select.h, window_search) */
uint32_t window_shift(uint32_t kl, uint32_t kh, int nsub_log2) {
    if (!(kh > kl + 1)) return 0;
    const uint32_t R = kh - kl - 1;
    int bits = 0;
    while (bits < 32 && (R >> bits)) ++bits;
    return bits > nsub_log2 ? (uint32_t)(bits - nsub_log2) : 0u;
}

/* The state k_collect leaves for a population and a window, by plain loops from the struct
 * definitions: below / eq_lo / maxkey spread over the shards, sub[b] counting every inside key
 * (kl < key <= kh), cand[b * bucket_cap + i] the first bucket_cap of them. */
void build_state(const float* x, int64_t n, uint32_t kl, uint32_t kh, int nsub_log2, int bucket_cap, int overflow,
                 SelState* st, std::vector<uint32_t>* cand) {
    memset(st, 0, sizeof(*st));
    const int nsub = 1 << nsub_log2;
    cand->assign((size_t)nsub * bucket_cap, 0u);
    st->kl = kl;
    st->kh = kh;
    st->shift = window_shift(kl, kh, nsub_log2);
    st->overflow = overflow ? 1u : 0u;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t key;
        memcpy(&key, x + i, 4);
        key &= 0x7FFFFFFFu;
        const int s = (int)(i % NSHARD);
        if (key > st->maxkey[s]) st->maxkey[s] = key;
        if (key < kl) ++st->below[s];
        else if (key == kl) ++st->eq_lo[s];
        else if (key <= kh) {
            const uint32_t b = (key - kl - 1) >> st->shift;
            const uint32_t at = st->sub[b]++;
            if (at < (uint32_t)bucket_cap) (*cand)[(size_t)b * bucket_cap + at] = key;
        }
    }
}

SegDesc seg_desc(const float* dx, int64_t n, int64_t r0, int above, double gamma, int flags, int nsub_log2,
                 int bucket_cap) {
    SegDesc sd;
    memset(&sd, 0, sizeof(sd));
    sd.data = dx;
    sd.n = n;
    sd.r0 = r0;
    sd.gamma = gamma;
    sd.numel = n;
    sd.flags = flags;
    sd.above = above;
    sd.cap = (int64_t)bucket_cap << nsub_log2;
    sd.nsub_log2 = nsub_log2;
    sd.bucket_cap = bucket_cap;
    return sd;
}

/* the summed counters of a SelState: {below, eq_lo, maxkey, overflow, shift} */
void state_sums(const SelState& st, int64_t* sums) {
    sums[0] = sums[1] = sums[2] = 0;
    for (int i = 0; i < NSHARD; ++i) {
        sums[0] += (int64_t)st.below[i];
        sums[1] += (int64_t)st.eq_lo[i];
        if ((int64_t)st.maxkey[i] > sums[2]) sums[2] = st.maxkey[i];
    }
    sums[3] = st.overflow;
    sums[4] = st.shift;
}

}  // namespace

extern "C" {

int sc_constant(const char* name) {
    struct { const char* n; int v; } t[] = {
        {"NB", NB}, {"BIN_ZERO", BIN_ZERO}, {"BIN_UNDER", BIN_UNDER}, {"BIN_OVER", BIN_OVER}, {"WCB", WCB},
        {"RES_BPL", RES_BPL}, {"WSEL_KPL", WSEL_KPL}, {"HS_PER", HS_PER}, {"STREAM_THREADS", STREAM_THREADS},
        {"COLLECT_THREADS", COLLECT_THREADS}, {"COLLECT_IT", COLLECT_IT}, {"WIN_THREADS", WIN_THREADS},
        {"M_SAMPLE", M_SAMPLE}, {"M_SAMPLE_WIN", M_SAMPLE_WIN}, {"RES_MS", RES_MS}, {"MS_STAGE", MS_STAGE},
        {"NSUB_MAX", NSUB_MAX}, {"NSHARD", NSHARD}, {"STG", STG}, {"CHUNK", CHUNK}, {"BUCKET_MAX", BUCKET_MAX},
        {"MODE_CAND", MODE_CAND}, {"MODE_WINDOW", MODE_WINDOW}, {"MODE_FULL", MODE_FULL}, {"SEG_MASK", SEG_MASK},
        {"SEG_MINPRUNE", SEG_MINPRUNE}, {"WIN_E0", (int)WIN_E0}, {"WIN_EXP", WIN_EXP}, {"MANT_BITS", MANT_BITS},
    };
    for (const auto& e : t)
        if (!strcmp(e.n, name)) return e.v;
    return -1;
}

/* key_bin / bin_lo_key / bin_hi_key compiled for the host (no device needed) */
void sc_bins_host(const uint32_t* keys, int nk, int* bin, uint32_t* lo, uint32_t* hi) {
    for (int i = 0; i < nk; ++i) bin[i] = key_bin(keys[i]);
    for (int b = 0; b < NB; ++b) { lo[b] = bin_lo_key(b); hi[b] = bin_hi_key(b); }
}

int sc_bins(const uint32_t* keys, int nk, int* bin, uint32_t* lo, uint32_t* hi) {
    Arena A;
    uint32_t* dk = A.up(keys, nk);
    int* db = A.zeros<int>(nk);
    uint32_t *dl = A.zeros<uint32_t>(NB), *dh = A.zeros<uint32_t>(NB);
    if (A.ok()) {
        const int n = nk > NB ? nk : NB;
        k_bins<<<(n + 255) / 256, 256>>>(dk, nk, db, dl, dh);
        A.ran();
    }
    A.down(bin, db, nk); A.down(lo, dl, NB); A.down(hi, dh, NB);
    return A.finish();
}

/* scan: ncase * 64; red: ncase * 2 (lane 0, lane 63) * 4 (sum, max, min, or); sum64: ncase * 2 */
int sc_wave_prims(const uint32_t* in, const unsigned long long* in64, int ncase, uint32_t* scan, uint32_t* red,
                  unsigned long long* sum64) {
    Arena A;
    uint32_t* di = A.up(in, (size_t)ncase * 64);
    unsigned long long* di64 = A.up(in64, (size_t)ncase * 64);
    uint32_t *ds = A.zeros<uint32_t>((size_t)ncase * 64), *dr = A.zeros<uint32_t>((size_t)ncase * 8);
    unsigned long long* d64 = A.zeros<unsigned long long>((size_t)ncase * 2);
    if (A.ok()) { k_wave_prims<<<1, 64>>>(di, di64, ncase, ds, dr, d64); A.ran(); }
    A.down(scan, ds, (size_t)ncase * 64); A.down(red, dr, (size_t)ncase * 8); A.down(sum64, d64, (size_t)ncase * 2);
    return A.finish();
}

/* digit / below keep the caller's fill where no lane holds the rank */
int sc_pick_digit(const uint32_t* hist, const int64_t* ranks, int nr, int* digit, int64_t* below) {
    Arena A;
    uint32_t* dh = A.up(hist, 256);
    int64_t* dr = A.up(ranks, nr);
    int* dd = A.up(digit, nr);
    int64_t* db = A.up(below, nr);
    if (A.ok()) { k_pick_digit<<<1, 64>>>(dh, dr, nr, dd, db); A.ran(); }
    A.down(digit, dd, nr); A.down(below, db, nr);
    return A.finish();
}

/* hist: NB bins; the coarse companion (bins of 128) is summed here */
static void coarse_of(const uint32_t* hist, uint32_t* hc) {
    for (int i = 0; i < WCB; ++i) hc[i] = 0;
    for (int b = 0; b < NB; ++b) hc[b >> 7] += hist[b];
}

int sc_find_bin(const uint32_t* hist, const int* ranks, int nr, int* out) {
    Arena A;
    uint32_t hc[WCB];
    coarse_of(hist, hc);
    uint32_t *dh = A.up(hist, NB), *dc = A.up(hc, WCB);
    int* dr = A.up(ranks, nr);
    int* dout = A.zeros<int>(nr);
    if (A.ok()) { k_find_bin<<<1, 64>>>(dh, dc, dr, nr, dout); A.ran(); }
    A.down(out, dout, nr);
    return A.finish();
}

int sc_find_bins_flat(const uint32_t* hist, const int* ra, const int* rb, int nr, int* fa, int* fb) {
    Arena A;
    uint32_t* dh = A.up(hist, NB);
    int *da = A.up(ra, nr), *db = A.up(rb, nr);
    int *dfa = A.zeros<int>(nr), *dfb = A.zeros<int>(nr);
    if (A.ok()) { k_find_bins_flat<<<1, 64>>>(dh, da, db, nr, dfa, dfb); A.ran(); }
    A.down(fa, dfa, nr); A.down(fb, dfb, nr);
    return A.finish();
}

/* which: 0 window_search<256, 4096> (k_collect's inline window), 1 window_search<1024, 4096>,
 * 2 window_search_wave<4096>, 3 window_search_flat (6 sigma + 24, m = min(n, 4096)),
 * 4 window_search<1024, 65536> (k_window, k_fwin).  cases: ncase x {n, r0, above, nsub_log2} as
 * int64; out: ncase x {kl, kh, sh}.  hist must sum to min(n, MS) for every case. */
int sc_window(int which, const uint32_t* hist, const int64_t* cases, int ncase, uint32_t* out) {
    Arena A;
    std::vector<WinCase> cs(ncase);
    for (int i = 0; i < ncase; ++i)
        cs[i] = WinCase{cases[4 * i], cases[4 * i + 1], (int32_t)cases[4 * i + 2], (int32_t)cases[4 * i + 3]};
    uint32_t hc[WCB];
    coarse_of(hist, hc);
    uint32_t *dh = A.up(hist, NB), *dc = A.up(hc, WCB);
    WinCase* dcs = A.up(cs.data(), ncase);
    uint32_t* dout = A.zeros<uint32_t>((size_t)ncase * 3);
    if (which < 0 || which > 4) { A.finish(); return -1; }
    if (A.ok()) {
        if (which == 0) k_window_block<COLLECT_THREADS, M_SAMPLE><<<1, COLLECT_THREADS>>>(dh, dcs, ncase, dout);
        if (which == 1) k_window_block<WIN_THREADS, M_SAMPLE><<<1, WIN_THREADS>>>(dh, dcs, ncase, dout);
        if (which == 2) k_window_wave<false><<<1, 64>>>(dh, dc, dcs, ncase, dout);
        if (which == 3) k_window_wave<true><<<1, 64>>>(dh, dc, dcs, ncase, dout);
        if (which == 4) k_window_block<WIN_THREADS, M_SAMPLE_WIN><<<1, WIN_THREADS>>>(dh, dcs, ncase, dout);
        A.ran();
    }
    A.down(out, dout, (size_t)ncase * 3);
    return A.finish();
}

/* every rank 0..m-1 of keys[0..m), m <= 64 * WSEL_KPL, all keys in [lo, hi] */
int sc_wave_select(const uint32_t* keys, int m, uint32_t lo, uint32_t hi, uint32_t* out) {
    if (m < 1 || m > 64 * WSEL_KPL) return -1;
    Arena A;
    uint32_t* dk = A.up(keys, m);
    uint32_t* dout = A.zeros<uint32_t>(m);
    if (A.ok()) { k_wave_select<<<1, 64>>>(dk, m, lo, hi, dout); A.ran(); }
    A.down(out, dout, m);
    return A.finish();
}

/* queries: nq x {ra, rb, need_a, need_b} as int64; out: nq x {ka, kb} */
int sc_select_in_range(const uint32_t* keys, int64_t m, uint32_t lo, uint32_t hi, const int64_t* queries, int nq,
                       uint32_t* out) {
    Arena A;
    std::vector<RangeQuery> qs(nq);
    for (int i = 0; i < nq; ++i) {
        qs[i] = RangeQuery{queries[4 * i], queries[4 * i + 1], (int32_t)queries[4 * i + 2], (int32_t)queries[4 * i + 3]};
        if ((qs[i].need_a && (qs[i].ra < 0 || qs[i].ra >= m)) || (qs[i].need_b && (qs[i].rb < 0 || qs[i].rb >= m))) return -1;
    }
    uint32_t* dk = A.up(keys, (size_t)m);
    RangeQuery* dq = A.up(qs.data(), nq);
    uint32_t* dout = A.zeros<uint32_t>((size_t)nq * 2);
    if (A.ok()) { k_select_in_range<<<1, STREAM_THREADS>>>(dk, m, lo, hi, dq, nq, dout); A.ran(); }
    A.down(out, dout, (size_t)nq * 2);
    return A.finish();
}

/* sel: nq x {key of ra, key of rb}; cnt: nt counts of keys < tks[q] */
int sc_block_hist(const uint32_t* keys, int m, uint32_t lo, int W, const int* ra, const int* rb, int nq, uint32_t* sel,
                  const uint32_t* tks, int nt, int64_t* cnt) {
    if (W < 1 || W > HS_PER * STREAM_THREADS || m < 1) return -1;
    for (int i = 0; i < m; ++i)
        if (keys[i] < lo || keys[i] - lo >= (uint32_t)W) return -1;
    for (int i = 0; i < nq; ++i)
        if (ra[i] < 0 || ra[i] >= m || rb[i] < 0 || rb[i] >= m) return -1;
    Arena A;
    uint32_t* dk = A.up(keys, m);
    int *da = A.up(ra, nq), *db = A.up(rb, nq);
    uint32_t* dsel = A.zeros<uint32_t>((size_t)nq * 2);
    uint32_t* dt = A.up(tks, nt);
    int64_t* dc = A.zeros<int64_t>(nt);
    if (A.ok()) { k_block_hist<<<1, STREAM_THREADS>>>(dk, m, lo, W, da, db, nq, dsel, dt, nt, dc); A.ran(); }
    A.down(sel, dsel, (size_t)nq * 2); A.down(cnt, dc, nt);
    return A.finish();
}

/* queries: nq x {ra, rb, need_a, need_b} as int64; bucket / before: nq x 2 (-1 where not wanted) */
int sc_find_buckets(const uint32_t* sub, int nsub, const int64_t* queries, int nq, int* bucket, int64_t* before) {
    if (nsub < 64 || nsub > NSUB_MAX || (nsub & (nsub - 1))) return -1;
    Arena A;
    std::vector<BucketQuery> qs(nq);
    for (int i = 0; i < nq; ++i)
        qs[i] = BucketQuery{queries[4 * i], queries[4 * i + 1], (int32_t)queries[4 * i + 2], (int32_t)queries[4 * i + 3]};
    uint32_t* ds = A.up(sub, nsub);
    BucketQuery* dq = A.up(qs.data(), nq);
    int* db = A.zeros<int>((size_t)nq * 2);
    int64_t* dbe = A.zeros<int64_t>((size_t)nq * 2);
    if (A.ok()) { k_find_buckets<<<1, 64>>>(ds, nsub, dq, nq, db, dbe); A.ran(); }
    A.down(bucket, db, (size_t)nq * 2); A.down(before, dbe, (size_t)nq * 2);
    return A.finish();
}

/* The host-built state alone: sums = {below, eq_lo, maxkey, overflow, shift}; sub: 1 << nsub_log2
 * counts; cand: (1 << nsub_log2) * bucket_cap keys (bucket b's first min(sub[b], bucket_cap)). */
int sc_build_state(const float* x, int64_t n, uint32_t kl, uint32_t kh, int nsub_log2, int bucket_cap, int64_t* sums,
                   uint32_t* sub, uint32_t* cand) {
    if (nsub_log2 < 6 || nsub_log2 > 10 || bucket_cap < 1 || !(kl < kh)) return -1;
    SelState st;
    std::vector<uint32_t> c;
    build_state(x, n, kl, kh, nsub_log2, bucket_cap, 0, &st, &c);
    state_sums(st, sums);
    memcpy(sub, st.sub, sizeof(uint32_t) << nsub_log2);
    memcpy(cand, c.data(), c.size() * 4);
    return 0;
}

/* select_body<STREAM_THREADS> on the host-built state of (x, window).  rec_i64 = {numel,
 * zero_count, coeff_numel}, rec_u32 = {thr32_bits, max_abs_bits, eff_level, path}: the record goes
 * in as the caller filled it and comes back as the select left it; thr_word likewise. */
int sc_select_body(const float* x, int64_t n, int64_t r0, int above, double gamma, int flags, int nsub_log2,
                   int bucket_cap, uint32_t kl, uint32_t kh, int overflow, int publish, int use_hscratch,
                   int prefer_wave, float* ret, int* path, int64_t* rec_i64, double* rec_thr64, uint32_t* rec_u32,
                   float* thr_word) {
    if (nsub_log2 < 6 || nsub_log2 > 10 || bucket_cap < 1 || !(kl < kh) || n < 1 || r0 < 0 || r0 >= n || (!above && r0 + 1 >= n))
        return -1;
    SelState st;
    std::vector<uint32_t> c;
    build_state(x, n, kl, kh, nsub_log2, bucket_cap, overflow, &st, &c);
    wtp_result r;
    memset(&r, 0, sizeof(r));
    r.numel = rec_i64[0]; r.zero_count = rec_i64[1]; r.coeff_numel = rec_i64[2];
    r.thr64 = *rec_thr64;
    r.thr32_bits = rec_u32[0]; r.max_abs_bits = rec_u32[1]; r.eff_level = (int32_t)rec_u32[2]; r.path = (int32_t)rec_u32[3];
    Arena A;
    float* dx = A.up(x, (size_t)n);
    SelState* dst = A.up(&st, 1);
    uint32_t* dc = A.up(c.data(), c.size());
    wtp_result* dr = A.up(&r, 1);
    float* dthr = A.up(thr_word, 1);
    float* dret = A.zeros<float>(1);
    int* dpath = A.zeros<int>(1);
    if (A.ok()) {
        const SegDesc sd = seg_desc(dx, n, r0, above, gamma, flags, nsub_log2, bucket_cap);
        k_select_body<<<1, STREAM_THREADS>>>(sd, dst, dc, dr, dthr, publish, use_hscratch, prefer_wave, dret, dpath);
        A.ran();
    }
    A.down(ret, dret, 1); A.down(path, dpath, 1); A.down(&r, dr, 1); A.down(thr_word, dthr, 1);
    rec_i64[0] = r.numel; rec_i64[1] = r.zero_count; rec_i64[2] = r.coeff_numel;
    *rec_thr64 = r.thr64;
    rec_u32[0] = r.thr32_bits; rec_u32[1] = r.max_abs_bits; rec_u32[2] = (uint32_t)r.eff_level; rec_u32[3] = (uint32_t)r.path;
    return A.finish();
}

/* collect_body<COLLECT_THREADS, COLLECT_IT, FULL, false> over x[off .. off + len) with the window
 * written into the SelState; outputs as sc_build_state's.  full = 1 needs len == CHUNK and off == 0
 * (a whole 16-byte-aligned chunk). */
int sc_collect_body(const float* x, int off, int len, int full, uint32_t kl, uint32_t kh, int nsub_log2,
                    int bucket_cap, int64_t* sums, uint32_t* sub, uint32_t* cand) {
    if (nsub_log2 < 6 || nsub_log2 > 10 || bucket_cap < 1 || !(kl < kh) || len < 1 || len > CHUNK || off < 0) return -1;
    if (full && (len != CHUNK || off != 0)) return -1;
    const size_t ncand = (size_t)bucket_cap << nsub_log2;
    SelState st;
    memset(&st, 0, sizeof(st));
    st.kl = kl;
    st.kh = kh;
    st.shift = window_shift(kl, kh, nsub_log2);
    Arena A;
    float* dx = A.up(x, (size_t)off + len);
    SelState* dst = A.up(&st, 1);
    uint32_t* dc = A.zeros<uint32_t>(ncand);
    if (A.ok()) {
        const SegDesc sd = seg_desc(dx + off, len, 0, 0, 0.0, SEG_MASK | (off ? 0 : SEG_ALIGNED), nsub_log2, bucket_cap);
        if (full) k_collect_body<true><<<1, COLLECT_THREADS>>>(sd, dst, dc, len);
        else k_collect_body<false><<<1, COLLECT_THREADS>>>(sd, dst, dc, len);
        A.ran();
    }
    A.down(&st, dst, 1);
    A.down(cand, dc, ncand);
    state_sums(st, sums);
    memcpy(sub, st.sub, sizeof(uint32_t) << nsub_log2);
    return A.finish();
}

}  // extern "C"

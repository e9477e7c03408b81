// Host build of the global percentile's pooled selection (csrc/wt_global_core.h over
// csrc/wt_sweep_core.h): the three histogram passes run piece by piece -- a piece stands for one
// tensor's part of the pool, and like a workgroup of csrc/global.hip it histograms its keys apart
// (gl_hist_index) and then adds the bins it filled into the pool's ONE histogram -- and one scan per
// pass with the ranks of the pooled count.  tests/test_global_core.py loads it as a shared object;
// tests/native/sanglobal.cpp is the stand-alone program over it.
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC globalcore.cpp
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../wavelettransforms_amd/csrc/wt_global_core.h"

namespace {

// inclusive prefix sums, then every rank of `slot` located in them
void scan_slot(const uint32_t* hist, int nbins, int slot, int pass, int nranks, const uint8_t* rank_slot,
               const uint32_t* rank_r, const uint32_t* rank_pre, uint32_t* npre, uint32_t* nres) {
    std::vector<uint32_t> incl(nbins);
    uint32_t s = 0;
    for (int i = 0; i < nbins; ++i) incl[i] = (s += hist[i]);
    for (int i = 0; i < nranks; ++i) {
        if (rank_slot[i] != slot) continue;
        uint32_t resid;
        const int d = sw_locate(incl.data(), nbins, rank_r[i], &resid);
        npre[i] = sw_extend(rank_pre[i], (uint32_t)d, pass);
        nres[i] = resid;
    }
}

// one pass over every piece: a histogram per piece, flushed (non-empty bins only) into `pool`
void pooled_pass(const uint32_t* keys, const long long* piece_len, int npieces, int pass, const uint8_t* tab1,
                 const uint8_t* tab2, std::vector<uint32_t>& pool, uint32_t* maxkey) {
    std::vector<uint32_t> h(pool.size());
    long long at = 0;
    for (int p = 0; p < npieces; ++p) {
        std::fill(h.begin(), h.end(), 0u);
        uint32_t mk = 0;
        for (long long i = 0; i < piece_len[p]; ++i) {
            const uint32_t key = keys[at + i];
            mk = std::max(mk, key);
            const int b = gl_hist_index(key, pass, tab1, tab2);
            if (b >= 0) ++h[(size_t)b];
        }
        at += piece_len[p];
        for (size_t b = 0; b < h.size(); ++b)
            if (h[b]) pool[b] += h[b];
        if (pass == 1 && mk > *maxkey) *maxkey = mk;
    }
}

}  // namespace

extern "C" {

// 1 when the populations pops[0 .. n) make a pool the selection takes; *total their sum.
int global_core_pool(const long long* pops, int n, unsigned long long* total) {
    std::vector<int64_t> p(pops, pops + n);
    uint64_t t = 0;
    const int ok = gl_pool_count(p.data(), n, &t);
    *total = t;
    return ok;
}

// The keys of ranks[0 .. nranks) (0-based, ascending) of the pool keys[0 .. sum(piece_len)), whose
// pieces lie one after another.  slots[0], slots[1]: the slots passes 2 and 3 used; *maxkey: the
// pool's largest key.  Returns 0, or a negative number on a bad argument.
int global_core_select(const uint32_t* keys, const long long* piece_len, int npieces, const uint32_t* ranks, int nranks,
                       uint32_t* out_keys, int* slots, uint32_t* maxkey) {
    if (npieces < 1 || nranks < 1 || nranks > SW_MAX_RANKS) return -1;
    std::vector<int64_t> pops(piece_len, piece_len + npieces);
    uint64_t n = 0;
    if (!gl_pool_count(pops.data(), npieces, &n) || n < 1) return -1;
    for (int i = 0; i < nranks; ++i)
        if ((uint64_t)ranks[i] >= n) return -1;
    uint32_t rank_pre[SW_MAX_RANKS] = {}, rank_res[SW_MAX_RANKS], npre[SW_MAX_RANKS], nres[SW_MAX_RANKS];
    uint32_t slot_prefix[2][SW_MAX_RANKS];
    uint8_t rank_slot[SW_MAX_RANKS] = {};
    std::vector<uint8_t> tab1(SW_BINS1, SW_NO_SLOT), tab2((size_t)SW_MAX_RANKS * SW_BINS, SW_NO_SLOT);
    // pass 1
    std::vector<uint32_t> h1(SW_BINS1, 0u);
    *maxkey = 0;
    pooled_pass(keys, piece_len, npieces, 1, tab1.data(), tab2.data(), h1, maxkey);
    scan_slot(h1.data(), SW_BINS1, 0, 1, nranks, rank_slot, ranks, rank_pre, npre, nres);
    int ns[2];
    ns[0] = sw_assign_slots(npre, nranks, slot_prefix[0], rank_slot);
    memcpy(rank_pre, npre, sizeof npre);
    memcpy(rank_res, nres, sizeof nres);
    // pass 2: top digit -> slot
    for (int s = 0; s < ns[0]; ++s) tab1[slot_prefix[0][s]] = (uint8_t)s;
    std::vector<uint32_t> h((size_t)SW_MAX_RANKS * SW_BINS, 0u);
    pooled_pass(keys, piece_len, npieces, 2, tab1.data(), tab2.data(), h, maxkey);
    for (int s = 0; s < ns[0]; ++s)
        scan_slot(h.data() + (size_t)s * SW_BINS, SW_BINS, s, 2, nranks, rank_slot, rank_res, rank_pre, npre, nres);
    ns[1] = sw_assign_slots(npre, nranks, slot_prefix[1], rank_slot);
    memcpy(rank_pre, npre, sizeof npre);
    memcpy(rank_res, nres, sizeof nres);
    // pass 3: (pass-2 slot, second digit) -> slot
    for (int s = 0; s < ns[1]; ++s) {
        const uint32_t p = slot_prefix[1][s];
        const uint32_t s2 = tab1[(p >> 10) & (SW_BINS1 - 1)];
        if (s2 == SW_NO_SLOT) return -2;
        tab2[s2 * SW_BINS + (p & (SW_BINS - 1))] = (uint8_t)s;
    }
    std::fill(h.begin(), h.end(), 0u);
    pooled_pass(keys, piece_len, npieces, 3, tab1.data(), tab2.data(), h, maxkey);
    for (int s = 0; s < ns[1]; ++s)
        scan_slot(h.data() + (size_t)s * SW_BINS, SW_BINS, s, 3, nranks, rank_slot, rank_res, rank_pre, npre, nres);
    for (int i = 0; i < nranks; ++i) out_keys[i] = npre[i];
    slots[0] = ns[0];
    slots[1] = ns[1];
    return 0;
}

// np.percentile of the pool at npct percentiles given as (r0, above, gamma): thr64, thr32.
int global_core_thresholds(const uint32_t* keys, const long long* piece_len, int npieces, const uint32_t* r0,
                           const int* above, const double* gamma, int npct, double* thr64, float* thr32, uint32_t* maxkey) {
    if (npct < 1 || npct > SW_MAX_PCT) return -1;
    uint32_t ranks[SW_MAX_RANKS], sel[SW_MAX_RANKS];
    for (int k = 0; k < npct; ++k) {
        ranks[2 * k] = gl_rank(r0[k], above[k], 0);
        ranks[2 * k + 1] = gl_rank(r0[k], above[k], 1);
    }
    int slots[2];
    const int rc = global_core_select(keys, piece_len, npieces, ranks, 2 * npct, sel, slots, maxkey);
    if (rc) return rc;
    for (int k = 0; k < npct; ++k) thr32[k] = sw_lerp(sel[2 * k], sel[2 * k + 1], gamma[k], *maxkey, &thr64[k]);
    return 0;
}

// Record (k, t) of a call of ntensors as gl_fill_record and gl_record_index lay it out: the
// record is written into recs (npct * ntensors of them); returns its index.
long long global_core_record(wtp_result* recs, int k, int ntensors, int t, long long numel, long long coeff_numel,
                             int eff_level, double thr64, uint32_t thr32_bits, uint32_t maxkey) {
    const size_t ri = gl_record_index(k, ntensors, t);
    gl_fill_record(&recs[ri], numel, coeff_numel, eff_level, thr64, thr32_bits, maxkey);
    return (long long)ri;
}

}  // extern "C"

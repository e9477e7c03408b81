// Host build of the percentile sweep's selection (csrc/wt_sweep_core.h): the three histogram passes
// and their scans over an arbitrary key array, with the same digit split, rank search, slot
// assignment and lerp the kernels of csrc/sweep.hip run.  tests/test_sweep_core.py loads it as a
// shared object; built as a program, main() checks it against std::sort (a sanitizer build of the
// program needs nothing else).
//   g++ -O2 -std=c++17 -ffp-contract=off [-shared -fPIC] sweepcore.cpp
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../wavelettransforms_amd/csrc/wt_sweep_core.h"

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

}  // namespace

extern "C" {

// The keys of ranks[0 .. nranks) (0-based, ascending) of keys[0 .. n).  slots[0], slots[1]: the
// slots passes 2 and 3 used; *maxkey: the largest key.  Returns 0, or -1 on a bad argument.
int sweep_core_select(const uint32_t* keys, long long n, const uint32_t* ranks, int nranks, uint32_t* out_keys,
                      int* slots, uint32_t* maxkey) {
    if (n < 1 || nranks < 1 || nranks > SW_MAX_RANKS) return -1;
    for (int i = 0; i < nranks; ++i)
        if ((long long)ranks[i] >= n) return -1;
    uint32_t rank_pre[SW_MAX_RANKS] = {}, rank_res[SW_MAX_RANKS], npre[SW_MAX_RANKS], nres[SW_MAX_RANKS];
    uint32_t slot_prefix[2][SW_MAX_RANKS];
    uint8_t rank_slot[SW_MAX_RANKS] = {};
    // pass 1
    std::vector<uint32_t> h1(SW_BINS1, 0u);
    uint32_t mk = 0;
    for (long long i = 0; i < n; ++i) {
        mk = std::max(mk, keys[i]);
        ++h1[sw_digit(keys[i], 1)];
    }
    *maxkey = mk;
    scan_slot(h1.data(), SW_BINS1, 0, 1, nranks, rank_slot, ranks, rank_pre, npre, nres);
    int ns[2];
    ns[0] = sw_assign_slots(npre, nranks, slot_prefix[0], rank_slot);
    memcpy(rank_pre, npre, sizeof npre);
    memcpy(rank_res, nres, sizeof nres);
    // pass 2: top digit -> slot
    std::vector<uint8_t> tab1(SW_BINS1, SW_NO_SLOT), tab2((size_t)SW_MAX_RANKS * SW_BINS, SW_NO_SLOT);
    for (int s = 0; s < ns[0]; ++s) tab1[slot_prefix[0][s]] = (uint8_t)s;
    std::vector<uint32_t> h((size_t)SW_MAX_RANKS * SW_BINS, 0u);
    for (long long i = 0; i < n; ++i) {
        const uint32_t s2 = tab1[sw_digit(keys[i], 1)];
        if (s2 != SW_NO_SLOT) ++h[s2 * SW_BINS + sw_digit(keys[i], 2)];
    }
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
    for (long long i = 0; i < n; ++i) {
        const uint32_t s2 = tab1[sw_digit(keys[i], 1)];
        if (s2 == SW_NO_SLOT) continue;
        const uint32_t s3 = tab2[s2 * SW_BINS + sw_digit(keys[i], 2)];
        if (s3 != SW_NO_SLOT) ++h[s3 * SW_BINS + sw_digit(keys[i], 3)];
    }
    for (int s = 0; s < ns[1]; ++s)
        scan_slot(h.data() + (size_t)s * SW_BINS, SW_BINS, s, 3, nranks, rank_slot, rank_res, rank_pre, npre, nres);
    for (int i = 0; i < nranks; ++i) out_keys[i] = npre[i];
    slots[0] = ns[0];
    slots[1] = ns[1];
    return 0;
}

// np.percentile of the population at npct percentiles given as (r0, above, gamma): thr64, thr32.
int sweep_core_thresholds(const uint32_t* keys, long long n, const uint32_t* r0, const int* above, const double* gamma,
                          int npct, double* thr64, float* thr32, int* slots) {
    if (npct < 1 || npct > SW_MAX_PCT) return -1;
    uint32_t ranks[SW_MAX_RANKS], sel[SW_MAX_RANKS], mk;
    for (int k = 0; k < npct; ++k) {
        ranks[2 * k] = r0[k];
        ranks[2 * k + 1] = r0[k] + (above[k] ? 0u : 1u);
    }
    const int rc = sweep_core_select(keys, n, ranks, 2 * npct, sel, slots, &mk);
    if (rc) return rc;
    for (int k = 0; k < npct; ++k) thr32[k] = sw_lerp(sel[2 * k], sel[2 * k + 1], gamma[k], mk, &thr64[k]);
    return 0;
}

uint32_t sweep_core_digit(uint32_t key, int pass) { return sw_digit(key, pass); }

}  // extern "C"

int main() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        return x;
    };
    int bad = 0;
    for (int trial = 0; trial < 40; ++trial) {
        const long long n = 1 + (long long)(next() % 70000);
        std::vector<uint32_t> keys(n);
        const int kind = trial % 4;
        for (auto& k : keys) {
            const uint64_t r = next();
            k = kind == 0 ? (uint32_t)(r & 0x7FFFFFFFu)                      // every bit pattern
                : kind == 1 ? (uint32_t)(0x3D000000u + (r & 0xFFFFFFu))      // one octave range
                : kind == 2 ? (uint32_t)(r % 5) * 0x00100401u                // five distinct values
                            : ((r & 3) ? 0u : (uint32_t)(r >> 33));           // 75 % zeros
        }
        uint32_t ranks[SW_MAX_RANKS], sel[SW_MAX_RANKS], mk;
        const int nranks = 1 + (int)(next() % SW_MAX_RANKS);
        for (int i = 0; i < nranks; ++i) ranks[i] = (uint32_t)(next() % (uint64_t)n);
        if (trial & 1) { ranks[0] = 0; ranks[nranks - 1] = (uint32_t)(n - 1); }
        int slots[2];
        if (sweep_core_select(keys.data(), n, ranks, nranks, sel, slots, &mk)) { ++bad; continue; }
        std::vector<uint32_t> sorted(keys);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 0; i < nranks; ++i) bad += sel[i] != sorted[ranks[i]];
        bad += mk != sorted.back() || slots[0] < 1 || slots[0] > nranks || slots[1] < slots[0] || slots[1] > nranks;
    }
    printf("sweepcore: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

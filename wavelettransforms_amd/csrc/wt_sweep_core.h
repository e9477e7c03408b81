/* The index arithmetic of the percentile sweep (sweep.hip, wtp_prune_sweep_f32): an exact radix
 * select of up to SW_MAX_RANKS order statistics at once over the 31-bit keys |x| (the float32 bit
 * pattern without its sign), in three histogram passes with digits of 11 / 10 / 10 bits.
 *
 *   pass 1   one histogram of the top digit (SW_BINS1 bins) per population;
 *   scan     every rank finds its bin (sw_locate) and its residual rank inside that bin; the
 *            distinct bins get slot numbers (sw_assign_slots), at most one per rank;
 *   pass 2/3 a key whose bits above the pass's digit (sw_prefix) own a slot adds to that slot's
 *            SW_BINS-bin histogram of the pass's digit; a scan like the first narrows every rank.
 *
 * After the third scan a rank's prefix is its key.  sw_lerp is NumPy 1.x's _lerp of the two order
 * statistics of one percentile with np.percentile's NaN rule.  Shared by the kernels of sweep.hip
 * and the host-side check (tests/native/sweepcore.cpp), which runs the same passes over arbitrary
 * key arrays.  Build with -ffp-contract=off: the blend is a separate multiply and add.
 */
#ifndef WT_SWEEP_CORE_H
#define WT_SWEEP_CORE_H

#include <stdint.h>

#include "wt_dwt_core.h"

#define SW_MAX_PCT 8
#define SW_MAX_RANKS (2 * SW_MAX_PCT)
#define SW_BINS1 2048
#define SW_BINS 1024
#define SW_NO_SLOT 0xFFu

/* the digit of `key` that pass 1, 2 or 3 histograms */
WT_CORE uint32_t sw_digit(uint32_t key, int pass) {
    return pass == 1 ? (key >> 20) & (SW_BINS1 - 1) : (pass == 2 ? (key >> 10) & (SW_BINS - 1) : key & (SW_BINS - 1));
}
/* the bits above that digit: what a slot of pass 2 (11 bits) or 3 (21 bits) stands for; pass 4:
 * the key itself */
WT_CORE uint32_t sw_prefix(uint32_t key, int pass) {
    return pass <= 1 ? 0u : (pass == 2 ? key >> 20 : (pass == 3 ? key >> 10 : key));
}
/* a rank's prefix after the scan of `pass`, from its prefix before and the digit it located */
WT_CORE uint32_t sw_extend(uint32_t prefix, uint32_t digit, int pass) {
    return pass == 1 ? digit : (prefix << 10) | digit;
}

/* incl[0 .. nbins): inclusive prefix sums of a histogram that holds more than r keys.  Returns the
 * bin of the key of rank r (0-based, ascending): the first bin d with incl[d] > r; *residual is
 * r's rank among that bin's keys. */
WT_CORE int sw_locate(const uint32_t* incl, int nbins, uint32_t r, uint32_t* residual) {
    int lo = 0, hi = nbins - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (incl[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    *residual = r - (lo ? incl[lo - 1] : 0u);
    return lo;
}

/* Slot numbers for the distinct values of prefix[0 .. nranks), in order of first appearance:
 * slot_prefix[s] is slot s's prefix, rank_slot[i] rank i's slot.  Returns the slot count. */
WT_CORE int sw_assign_slots(const uint32_t* prefix, int nranks, uint32_t* slot_prefix, uint8_t* rank_slot) {
    int ns = 0;
    for (int i = 0; i < nranks; ++i) {
        int s = 0;
        while (s < ns && slot_prefix[s] != prefix[i]) ++s;
        if (s == ns) slot_prefix[ns++] = prefix[i];
        rank_slot[i] = (uint8_t)s;
    }
    return ns;
}

WT_CORE float sw_key_float(uint32_t k) {
    float f;
    __builtin_memcpy(&f, &k, 4);
    return f;
}
WT_CORE uint32_t sw_float_bits(float f) {
    uint32_t k;
    __builtin_memcpy(&k, &f, 4);
    return k;
}

/* np.percentile's value from its two order statistics ka <= kb (keys) and gamma:
 * numpy/lib/function_base.py _lerp -- the difference in float32, the blend in float64, from the
 * upper end when gamma >= 0.5.  A NaN in the population (a key above +inf's: maxkey) makes the
 * percentile NaN.  Returns float32(thr64), the value the compare uses. */
WT_CORE float sw_lerp(uint32_t ka, uint32_t kb, double gamma, uint32_t maxkey, double* thr64) {
    const float fa = sw_key_float(ka), fb = sw_key_float(kb);
    const float diff = fb - fa;
    const double da = (double)diff * (1.0 - gamma), db = (double)diff * gamma;
    double thr = (gamma >= 0.5) ? (double)fb - da : (double)fa + db;
    if (maxkey > 0x7F800000u) {
        const uint64_t nanb = 0x7FF8000000000000ull;
        __builtin_memcpy(&thr, &nanb, 8);
    }
    *thr64 = thr;
    return (float)thr;
}

#endif

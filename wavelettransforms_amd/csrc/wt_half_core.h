/* The arithmetic of the float16 path (half.hip, wtp_prune_f16): what NumPy 1.x does with a float16
 * array that gets no transform (ndim < 2, or level 0 after the clamp; dwt_pruning.py:25-32 on the
 * array as it is), and the two conversions around the float32 path of the tensors that get one.
 *
 *   key      |w| of an IEEE binary16 word is its low 15 bits, and the order of those keys is the
 *            order of |w| (NaN keys lie above +inf's, 0x7C00).  A population has 2^15 possible
 *            keys, so an exact selection is two histogram passes: the top H16_BITS1 bits
 *            (H16_BINS1 bins), then the low H16_BITS2 bits of the keys under one top digit.
 *   ranks    np.percentile's two order statistics (host_plan's seg_ranks), found in the histograms
 *            by h16_locate; the maximum is the order statistic of rank n - 1.
 *   rule     d = b - a is NumPy's HALF subtraction: the float32 difference rounded once to half;
 *            the blend runs in float64 from the upper end when gamma >= 0.5 (NumPy's _lerp);
 *            the compare |w| < thr runs in float16 on half(thr64), one round-to-nearest-even from
 *            float64 (value-based casting), i.e. key(w) < key(half(thr64)).
 *   convert  h16_to_float (exact), h16_from_double / h16_from_float (round to nearest even, once;
 *            subnormals, overflow to inf, NaN kept quiet).
 *
 * Pinned on +-inf and NaN in the input as well (tests/half_ref.kind_b_ref): a NaN makes the
 * threshold NaN and nothing is pruned; an inf at a rank goes through the same difference and blend
 * (inf - inf is NaN).  Not pinned: finite |w| >= 65000 (the compare's type changes there).  The
 * code is safe on them -- a key is always a valid bin -- but no parity with the reference is
 * claimed.  Shared by half.hip and tests/native/halfcore.cpp.  Build with -ffp-contract=off: the
 * blend is a separate multiply and add.
 */
#ifndef WT_HALF_CORE_H
#define WT_HALF_CORE_H

#include <stdint.h>

#include "wt_dwt_core.h"

#ifndef H16_BITS1
#define H16_BITS1 11 /* the split the library is built with; -DH16_BITS1=8 .. 13 builds others */
#endif
#define H16_BITS2 (15 - H16_BITS1)
#define H16_BINS1 (1 << H16_BITS1)
#define H16_BINS2 (1 << H16_BITS2)
#define H16_NRANK 3 /* the order statistics a tensor needs: rank lo, rank hi, the maximum */

WT_CORE uint32_t h16_key(uint16_t bits) { return bits & 0x7FFFu; }
WT_CORE uint32_t h16_digit1(uint32_t key) { return key >> H16_BITS2; }
WT_CORE uint32_t h16_digit2(uint32_t key) { return key & (H16_BINS2 - 1); }
WT_CORE uint32_t h16_join(uint32_t d1, uint32_t d2) { return (d1 << H16_BITS2) | d2; }

/* the value of a binary16 word as float32 bits (exact) */
WT_CORE uint32_t h16_to_float_bits(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1Fu;
    uint32_t m = h & 0x3FFu;
    if (e == 0x1Fu) return sign | 0x7F800000u | (m << 13);
    if (e != 0) return sign | ((e + 112u) << 23) | (m << 13);
    if (m == 0) return sign;
    /* subnormal: m * 2^-24, normalised */
    const int sh = __builtin_clz(m) - 21; /* m < 2^10: moves its top bit to bit 10 */
    m = (m << sh) & 0x3FFu;
    return sign | ((uint32_t)(113 - sh) << 23) | (m << 13);
}
WT_CORE float h16_to_float(uint16_t h) {
    const uint32_t b = h16_to_float_bits(h);
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

/* float64 -> binary16, round to nearest even, once */
WT_CORE uint16_t h16_from_double(double x) {
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
    const int e = (int)((b >> 52) & 0x7FF);
    const uint64_t m = b & 0xFFFFFFFFFFFFFull;
    if (e == 0x7FF) return (uint16_t)(sign | 0x7C00u | (m ? (0x200u | (uint16_t)(m >> 42)) : 0u));
    const int he = e - 1023 + 15; /* the half's biased exponent, were it normal */
    if (he >= 0x1F) return (uint16_t)(sign | 0x7C00u);
    if (he <= -11) return sign; /* |x| < 2^-25: below half of the smallest subnormal (float64 subnormals too) */
    /* the significand with its hidden bit, shifted so that the kept part is the half's 10 (normal)
     * or fewer (subnormal) fraction bits */
    const uint64_t sig = m | (1ull << 52);
    const int shift = he >= 1 ? 42 : 43 - he; /* 42 .. 53 */
    uint64_t q = sig >> shift;
    const uint64_t rem = sig & ((1ull << shift) - 1), halfway = 1ull << (shift - 1);
    if (rem > halfway || (rem == halfway && (q & 1))) ++q;
    /* normal: q holds the hidden bit at 2^10, so adding (he - 1) << 10 gives the word, and a carry
     * out of the fraction moves into the exponent (up to inf) by itself; subnormal: q is the word,
     * and a carry to 2^10 is the smallest normal */
    const uint32_t w = he >= 1 ? (uint32_t)q + ((uint32_t)(he - 1) << 10) : (uint32_t)q;
    return (uint16_t)(sign | w);
}
/* float32 -> binary16: the widening to float64 is exact, so this rounds once */
WT_CORE uint16_t h16_from_float(float x) { return h16_from_double((double)x); }

/* hist[0 .. nbins) holds more than r keys.  The bin of the key of rank r (0-based, ascending): the
 * first bin whose inclusive prefix sum exceeds r; *residual is r's rank among that bin's keys. */
WT_CORE int h16_locate(const uint32_t* hist, int nbins, uint32_t r, uint32_t* residual) {
    uint32_t below = 0;
    int d = 0;
    while (d < nbins - 1 && below + hist[d] <= r) below += hist[d++];
    *residual = r - below;
    return d;
}
/* the same over a histogram whose groups of `per` bins have inclusive prefix sums gincl[0 .. nbins / per):
 * a binary search for the group, h16_locate inside it */
WT_CORE int h16_locate_grouped(const uint32_t* hist, const uint32_t* gincl, int nbins, int per, uint32_t r,
                               uint32_t* residual) {
    int lo = 0, hi = nbins / per - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (gincl[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t before = lo ? gincl[lo - 1] : 0u;
    return lo * per + h16_locate(hist + lo * per, per, r - before, residual);
}

/* NumPy's half subtraction b - a of two non-negative halves given by their keys */
WT_CORE uint16_t h16_diff(uint32_t ka, uint32_t kb) {
    return h16_from_float(h16_to_float((uint16_t)kb) - h16_to_float((uint16_t)ka));
}

/* np.percentile of |w| over a float16 population from its order statistics ka <= kb (keys), gamma
 * and `above` (the percentile is the maximum, kmax: NumPy takes a = b = max and gamma = n, so an
 * infinite maximum gives d = inf - inf and a NaN threshold).  A NaN anywhere in the population
 * (kmax above inf's key) makes the percentile NaN.  Returns the key of half(thr64): the value the
 * float16 compare uses. */
WT_CORE uint32_t h16_threshold(uint32_t ka, uint32_t kb, uint32_t kmax, double gamma, int above, double* thr64) {
    if (above) ka = kb = kmax;
    const double a = (double)h16_to_float((uint16_t)ka), b = (double)h16_to_float((uint16_t)kb);
    const double d = (double)h16_to_float(h16_diff(ka, kb));
    const double da = d * (1.0 - gamma), db = d * gamma;
    double thr = (gamma >= 0.5) ? b - da : a + db;
    if (kmax > 0x7C00u) thr = (double)__builtin_nanf("");
    *thr64 = thr;
    const uint32_t ck = h16_key(h16_from_double(thr));
    return ck > 0x7C00u ? 0u : ck; /* a NaN threshold compares false with everything: nothing is pruned */
}

/* the masked word: +0 where |w| < thr (on keys), else w as it is (-0 included) */
WT_CORE uint16_t h16_mask(uint16_t w, uint32_t ckey) { return h16_key(w) < ckey ? (uint16_t)0 : w; }
WT_CORE int h16_is_zero(uint16_t w) { return h16_key(w) == 0; }

/* A tensor of n halves at byte address `addr` (2-byte aligned): `head` leading words up to the
 * first 16-byte boundary, `nvec` aligned vectors of 8 words, the rest from `tail` on. */
typedef struct h16_span {
    int64_t head, nvec, tail;
} h16_span;
WT_CORE h16_span h16_split(uint64_t addr, int64_t n) {
    h16_span s;
    s.head = (int64_t)(((16u - (uint32_t)(addr & 15u)) & 15u) / 2u);
    if (s.head > n) s.head = n;
    s.nvec = (n - s.head) / 8;
    s.tail = s.head + 8 * s.nvec;
    return s;
}

#endif

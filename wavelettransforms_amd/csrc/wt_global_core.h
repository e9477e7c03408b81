/* The index arithmetic of the global percentile (global.hip, wtp_prune_global_f32) that is not
 * already wt_sweep_core.h's: the selection is the sweep's exact radix select (digits of 11 / 10 /
 * 10 bits, sw_locate, sw_assign_slots, sw_lerp), run over ONE population, the pool of every
 * tensor's keys.  New here:
 *
 *   the pooled count   gl_pool_count: the sum of the tensors' populations, and the overflow rule --
 *                      ranks, residuals and bins are 32 bits wide and one bin may hold the whole
 *                      pool, so a pool holds at most GL_MAX_POOL = 2^32 - 1 keys;
 *   the ranks          gl_rank: the two order statistics of percentile k among the pool's keys;
 *   the bin of a key   gl_hist_index: where a key adds in the pass's histogram, through the two
 *                      small tables (top digit -> pass-2 slot, (pass-2 slot, second digit) ->
 *                      pass-3 slot) that the pass kernels build in LDS, or nowhere;
 *   the records        gl_fill_record: which field of record (k, t) is tensor t's own and which
 *                      is the pool's at percentile k; gl_record_index: where that record sits.
 *
 * Shared by the kernels of global.hip and the host-side check (tests/native/globalcore.cpp), which
 * runs the pooled passes over key arrays cut into pieces. */
#ifndef WT_GLOBAL_CORE_H
#define WT_GLOBAL_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/wtprune.h"
#include "wt_sweep_core.h"

#define GL_MAX_POOL 0xFFFFFFFFull

/* The pool's key count: the sum of pops[0 .. n), each >= 0.  Returns 1 when it is at most
 * GL_MAX_POOL, else 0; *total is the exact sum either way (n < 2^31 populations of < 2^63 / n
 * keys: the host hands it populations of at most 2^31 - 1). */
WT_CORE int gl_pool_count(const int64_t* pops, int n, uint64_t* total) {
    uint64_t s = 0;
    for (int i = 0; i < n; ++i) s += (uint64_t)pops[i];
    *total = s;
    return s <= GL_MAX_POOL;
}

/* rank `half` (0: the lower, 1: the upper order statistic) of a percentile whose lower rank is r0;
 * `above`: both are the maximum (np.percentile's index -1).  r0 + 1 <= N - 1 < 2^32. */
WT_CORE uint32_t gl_rank(uint32_t r0, int above, int half) { return r0 + ((half && !above) ? 1u : 0u); }

/* The word of the pass's histogram that `key` adds to, or -1: pass 1 the top digit's bin; pass 2
 * bin (slot of the top digit, second digit); pass 3 bin (slot of the 21-bit prefix, third digit).
 * tab1[SW_BINS1]: top digit -> pass-2 slot, tab2[slots * SW_BINS]: (pass-2 slot, second digit) ->
 * pass-3 slot; SW_NO_SLOT where no rank lives. */
WT_CORE int gl_hist_index(uint32_t key, int pass, const uint8_t* tab1, const uint8_t* tab2) {
    if (pass == 1) return (int)sw_digit(key, 1);
    const uint32_t s2 = tab1[sw_digit(key, 1)];
    if (s2 == SW_NO_SLOT) return -1;
    if (pass == 2) return (int)(s2 * SW_BINS + sw_digit(key, 2));
    const uint32_t s3 = tab2[s2 * SW_BINS + sw_digit(key, 2)];
    if (s3 == SW_NO_SLOT) return -1;
    return (int)(s3 * SW_BINS + sw_digit(key, 3));
}

/* records are percentile-major, as the sweep's: tensor t at percentile k */
WT_CORE size_t gl_record_index(int k, int ntensors, int t) { return (size_t)k * (size_t)ntensors + (size_t)t; }

/* Record (k, t): numel, coeff_numel and eff_level are the tensor's own (zero_count too: the
 * kernels that write its output add to it); thr64, thr32_bits and max_abs_bits are the pool's at
 * percentile k -- the maximum is the pool's because the thresholded array is the pool. */
WT_CORE void gl_fill_record(wtp_result* r, int64_t numel, int64_t coeff_numel, int32_t eff_level, double pool_thr64,
                            uint32_t pool_thr32_bits, uint32_t pool_maxkey) {
    r->numel = numel;
    r->zero_count = 0;
    r->coeff_numel = coeff_numel;
    r->thr64 = pool_thr64;
    r->thr32_bits = pool_thr32_bits;
    r->max_abs_bits = pool_maxkey;
    r->eff_level = eff_level;
    r->path = WTP_PATH_GLOBAL;
}

#endif

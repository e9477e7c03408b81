/*
 * wtp_half.h -- what host_half.hip and half.hip share: the table of float16 tensors a launch
 * takes as its kernel argument, the per-tensor selection state and the launch_* entry points of
 * half.hip.  Nothing of the float32 units includes it.
 */
#ifndef WTP_HALF_H
#define WTP_HALF_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wtprune.h"
#include "wt_half_core.h"

namespace wtp {

constexpr int H16_PER_LAUNCH = 32;   /* tensors per table (the table is the kernels' argument) */
constexpr int H16_THREADS = 256;
constexpr int H16_VEC_IT = 8;        /* 16-byte vectors per thread: 64 words */
constexpr int H16_VPB = H16_THREADS * H16_VEC_IT; /* vectors per block: 16384 words, 32 KB */

/* one tensor of a launch */
struct H16Seg {
    const uint16_t* in; /* the float16 input (kind B: selected and masked; kind A: widened)      */
    uint16_t* out;      /* the float16 output (may be `in`)                                       */
    float* stage;       /* kind A: its float32 staging (input and output of the inner call)       */
    int64_t n;          /* words                                                                  */
    int64_t r0;         /* kind B: np.percentile's lower rank ...                                 */
    double gamma;       /* ... its weight ...                                                     */
    int32_t above;      /* ... or: the percentile is the maximum                                  */
    int32_t res;        /* its record in the caller's results                                     */
    int32_t sub;        /* kind A: its record among the inner call's; kind B: its state and histograms */
    int32_t eff_level;
};
struct H16Table {
    int32_t nseg, nblk;
    int32_t blk_begin[H16_PER_LAUNCH]; /* first block of segment i; INT32_MAX past nseg */
    H16Seg s[H16_PER_LAUNCH];
};
static_assert(sizeof(H16Table) <= 3072, "the table travels as a kernel argument");

/* kind B, per tensor: the three order statistics (rank lo, rank hi, the maximum) as they narrow */
struct H16State {
    uint32_t d1[H16_NRANK];    /* top digits                                  */
    uint32_t resid[H16_NRANK]; /* ranks inside their top digit's keys          */
    uint32_t ckey;             /* key(half(thr64)): what the mask compares with */
    uint32_t pad;
};

/* the workspace words of the kind-B selection */
struct H16Ws {
    uint32_t* hist1; /* per tensor H16_BINS1 */
    uint32_t* hist2; /* per tensor H16_NRANK x H16_BINS2 */
    H16State* st;
};

/* zeroes `words` 32-bit words at `a` and the `nres` records at `res` (a kernel, not a memset node) */
void launch_h16_init(uint32_t* a, int64_t words, wtp_result* res, int nres, hipStream_t s);
/* kind B, in this order: the top-digit histograms; the ranks' top digits; the low-digit histograms
 * of those; the threshold and the record; the mask, store and zero count */
void launch_h16_hist1(const H16Table& t, H16Ws w, hipStream_t s);
void launch_h16_scan1(const H16Table& t, H16Ws w, hipStream_t s);
void launch_h16_hist2(const H16Table& t, H16Ws w, hipStream_t s);
void launch_h16_scan2(const H16Table& t, H16Ws w, wtp_result* res, hipStream_t s);
void launch_h16_mask(const H16Table& t, H16Ws w, wtp_result* res, hipStream_t s);
/* kind A: float16 -> staging before the inner float32 call; staging -> float16 after it, with the
 * zero count of the narrowed words and the inner call's record `sub` copied to record `res` */
void launch_h16_widen(const H16Table& t, hipStream_t s);
void launch_h16_narrow(const H16Table& t, const wtp_result* sub, wtp_result* res, hipStream_t s);

}  // namespace wtp

#endif

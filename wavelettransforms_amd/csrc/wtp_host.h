/*
 * wtp_host.h -- what the host units of libwtprune.so share (host_plan.hip, host_chains.hip,
 * host_prune.hip, host_methods.hip, host_query.hip): the error state, the plan of one tensor, the
 * workspace layout, a transform chain and the helpers every entry family uses.  The host side
 * reaches the device only through the launch_* declarations of wtp_internal.h.  No allocation, no
 * synchronisation: everything is stream-ordered and graph-capturable.
 */
#ifndef WTP_HOST_H
#define WTP_HOST_H

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wtp_internal.h"

namespace wtp {

/* ---- error state (host_plan.hip): wtp_last_error / wtp_last_error_tensor of this thread ---- */
extern thread_local std::string g_err;
extern thread_local int g_err_tensor;
int fail(int code, int tensor, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline void clear_error() {
    g_err.clear();
    g_err_tensor = -1;
}
int check_launch(); /* WTP_OK, or WTP_EHIP with hipGetLastError's text */

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }
template <class T = char>
inline T* wsb(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

/* ---- the wavelet table (wt_filters.inc, compiled into host_plan.hip only) ---- */
int wavelet_count();
const char* wavelet_name(int wid); /* null for an unknown id */
int wavelet_flen(int wid);         /* -1 for an unknown id */
inline bool wavelet_known(int wid) { return wid >= 0 && wid < wavelet_count(); }
Taps taps_for(int wid);            /* Taps{} for an unknown id (only ndim < 2 tensors plan under one) */
int max_level(int64_t n, int F);   /* pywt.dwt_max_level */

/* ---- flags and modes ---- */
inline bool flags_ok(int flags) { return !(flags & ~(WTP_CARRY_LEVEL | WTP_FLATTEN | WTP_NO_RESIDENT)); }
int mode_check(int mode_id, int flags); /* WTP_OK when the mode and the flags can run; else the error is set */

/* One tensor of the call, as the reference would see it. */
struct TPlan {
    int ndim = 0;
    int64_t numel = 0;
    int64_t B = 1, H = 1, W = 1;
    int L = 0;
    bool dwt = false;     /* wavelet transform actually runs (ndim >= 2 and L >= 1)    */
    int64_t pop = 0;      /* selection population: numel, or the packed coefficient count */
    bool tight = true;
    wt_level_geom g;
    int64_t cap = 0;      /* candidate capacity                                         */
    size_t p_off = 0;     /* workspace byte offset of the packed array (dwt only)       */
    size_t cand_off = 0;  /* element offset into the candidate region                   */
    size_t t_off = 0;     /* workspace byte offset of this tensor's three level temps      */
    size_t t_elems = 0;   /* elements per temp                                              */
    bool flat = false;    /* 1-D flattened mode: pywt.wavedec / waverec of the flat tensor   */
    int64_t f_slots = 0;  /* fused selection: k_fwd_int wave slots of its forward (0: never fused) */
    size_t f_off = 0;     /* workspace byte offset of its slot area (per group parity and slot) */
    int64_t len[34] = {}; /* flat: len[0] = numel, len[k] = ceil(len[k-1] / 2)              */
    bool strict = false;  /* unclamped levels (wtp_prune_abs_f32): lvl_tiled keeps short sides per-point */
    int mode = 0;         /* WTP_MODE_* of a transform that runs in modes.hip (0: the periodized kernels) */
    int tiny_lg = -1;     /* mode != 0: log2 of the lanes k_mtiny_* give the tensor's images (-1: per-level kernels) */
};

/* The prefix every validator shares: the ndim range, no negative dimension, numel, and (check_ptrs)
 * the pointers of a non-empty tensor.  Fills p.ndim and p.numel. */
int read_shape(const wtp_tensor& x, int t, bool check_ptrs, TPlan& p);
/* B images of H x W at level L (valid: 0..32) of an F-tap filter under `mode`: dwt, the geometry,
 * pop and tight.  Level 0 is the same in every mode: it keeps the periodized plan (and kernels). */
void plan_image(TPlan& p, int64_t B, int64_t H, int64_t W, int L, int F, int mode);
/* Validate and plan every tensor in the reference's order; returns WTP_OK or the first error. */
int plan_tensors(const wtp_tensor* ts, int n, int wid, int level, double pct, bool check_ptrs, std::vector<TPlan>& out,
                 bool carry, bool flat, int mode);
bool lvl_tiled(const TPlan& p, int64_t B, int64_t R, int64_t C, const Taps& tp);
size_t temp_elems(const TPlan& p, const Taps& tp);
int64_t fused_slot_count(const TPlan& p, const float* in, const Taps& tp, bool sizing);

struct Layout {
    size_t hist = 0, sel = 0, thr = 0, cand = 0, P = 0, total = 0;
    size_t fwh = 0; /* k_fwin's histograms (when some tensor can be fused) */
};
Layout make_layout(std::vector<TPlan>& ps, const Taps& tp);
/* the workspace queries: plan (no pointers, percentile 50) and lay out; 0 for an invalid request */
size_t layout_bytes(const wtp_tensor* ts, int n, int wid, int level, bool carry, bool flat, int mode);

/* The outputs of tensor t of a sweep over n tensors (set-major: set k's at outs[k * n + t]): none
 * null, no two the same buffer.  Each sweep entry calls it in its tensor loop for the tensors that
 * need outputs, so its other per-tensor complaints keep their place. */
inline int check_sweep_outs(float* const* outs, int nsets, int n, int t) {
    for (int k = 0; k < nsets; ++k) {
        if (!outs[(size_t)k * n + t]) return fail(WTP_EARG, t, "tensor %d: output %d is a null pointer", t, k);
        for (int j = 0; j < k; ++j)
            if (outs[(size_t)j * n + t] == outs[(size_t)k * n + t])
                return fail(WTP_EARG, t, "tensor %d: outputs %d and %d are the same buffer", t, j, k);
    }
    return WTP_OK;
}

/* ---- segment tables (the percentile path and min pruning) ---- */
void bucket_plan(int64_t n, int* nsub_log2, int* bucket_cap, bool dwt);
int64_t cap_for(int64_t n, bool dwt);
void seg_ranks(int64_t n, double pct, SegDesc& sd); /* np.percentile's two order statistics */
/* Appends tensor p as result `res` with `nblk` blocks of the grouped grid: every field but the
 * ranks; `flags` gains SEG_ALIGNED.  The caller adds the ranks and what its kernels need more. */
SegDesc& seg_add(SegTable& tab, const TPlan& p, const float* data, float* out, int res, int flags, int nblk);
void seg_close(SegTable& tab); /* block -> segment sweep: INT32_MAX past nseg */

/* ---- transform chains (host_chains.hip) ---- */
/* one image batch's transform chain: its input / output, packed array and three level temps */
struct Chain {
    const TPlan* p;
    const float* in;   /* forward input */
    float* out;        /* inverse output */
    float* P;
    float* T[3];
    const float* thr;
    unsigned long long* zc;
    uint32_t* fsl = nullptr; /* fused selection: the tensor's slot area (null: not fused) */
};
/* the three level temps lie `stride` bytes apart from `temps` on */
Chain make_chain(const TPlan& p, const float* in, float* out, float* P, void* temps, size_t stride, const float* thr,
                 unsigned long long* zc);
void forward_chains(const std::vector<Chain>& cs, const Taps& tp, hipStream_t s, bool fused = false);
void inverse_chains(const std::vector<Chain>& cs, const Taps& tp, hipStream_t s);
void forward_flat(const TPlan& p, const float* in, float* P, float* T0, float* T1, const Taps& tp, hipStream_t s);
void inverse_flat(const TPlan& p, const float* P, float* out, float* T0, float* T1, const Taps& tp, const float* thr,
                  unsigned long long* zc, hipStream_t s);

}  // namespace wtp

#endif

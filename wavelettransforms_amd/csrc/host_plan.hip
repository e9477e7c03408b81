/*
 * host_plan.hip -- planning and layout: the error state, the wavelet table, validation in the
 * reference's order (ResNet/dwt_pruning.py:35-95), the plan of one tensor, the workspace layout and
 * the segment tables of the selection launches.  Nothing here calls HIP but check_launch().
 */
#include <cstdarg>
#include <cstdio>

#include "wtp_host.h"
#include "wt_filters.inc"

namespace wtp {

thread_local std::string g_err;
thread_local int g_err_tensor = -1;

int fail(int code, int tensor, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    g_err_tensor = tensor;
    return code;
}

int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WTP_EHIP, -1, "HIP: %s", hipGetErrorString(e));
    return WTP_OK;
}

int wavelet_count() { return WT_NUM_WAVELETS; }
const char* wavelet_name(int wid) { return wavelet_known(wid) ? wt_names[wid] : nullptr; }
int wavelet_flen(int wid) { return wavelet_known(wid) ? wt_flen[wid] : -1; }

Taps taps_for(int wid) {
    Taps tp;
    memset(&tp, 0, sizeof tp);
    if (!wavelet_known(wid)) return tp;
    const int F = wt_flen[wid];
    tp.F = F;
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < F; ++j) {
            uint32_t b = wt_taps_bits[wt_foff[wid] + k * F + j];
            memcpy(&tp.f[k][j], &b, 4);
        }
    return tp;
}

int max_level(int64_t n, int F) {
    if (F < 2) return -1;
    if (n < F - 1) return 0;
    int L = 0;
    while (((int64_t)(F - 1) << (L + 1)) <= n && L < 62) ++L;
    return L;
}

int mode_check(int mode_id, int flags) {
    if (!flags_ok(flags)) return fail(WTP_EARG, -1, "bad flags 0x%x", flags);
    if (mode_id < 0 || mode_id > WTP_MODE_ANTIREFLECT) return fail(WTP_EARG, -1, "Unknown mode id %d", mode_id);
    if (!wtm_mode_known(mode_id)) return fail(WTP_EARG, -1, "mode '%s' is not implemented", wtp_mode_name(mode_id));
    if (mode_id != WTP_MODE_PERIODIZATION && (flags & WTP_FLATTEN))
        return fail(WTP_EARG, -1, "WTP_FLATTEN runs under periodization only");
    return WTP_OK;
}

static bool pct_ok(double pct) { return pct >= 0.0 && pct <= 100.0; }

/* candidate buckets of the three-launch form: ~1000 keys of 5% of the population per bucket
 * (64..1024 buckets; the window holds ~5-6%) with capacity for 4x that (an overflowing bucket
 * sends the select to its exact full-scan path).  A DWT segment's select runs once (its first
 * k_mask_select block), so its buckets hold ~2000 keys -- still one LDS stage for the select
 * (MS_STAGE), twice as long runs per k_collect block (its ~900 inside keys are ~1 key per bucket
 * at 1024 buckets: partial-line stores, 4x the candidate bytes).  64 buckets cut those stores to
 * 1.2x but the select then radix-selects ~28K keys from L2 (+55 us per launch on cfg5, more
 * than k_collect saved).  The resident form always uses NSUB_MAX buckets: its runs are per
 * workgroup, and narrow buckets let one LDS histogram finish the select. */
void bucket_plan(int64_t n, int* nsub_log2, int* bucket_cap, bool dwt) {
    /* a segment too large for the inline window always gets k_window's M_SAMPLE_WIN-key window:
     * 2 (6 sigma + 24) sample ranks wide, plus the bins' outward rounding */
    const double m = (double)M_SAMPLE_WIN;
    const double wfrac = n > (int64_t)WINDOW_INLINE_MAX_BLOCKS * CHUNK ? (6.0 * sqrt(m) + 48.0) / m + 0.005 : 0.05;
    const double expect = wfrac * (double)n;
    int lg = 6;
    while (lg < 10 && (double)(1 << lg) * (dwt ? 2048.0 : 1024.0) < expect) ++lg;
    int64_t bc = (int64_t)(4.0 * expect / (double)(1 << lg)) + 1;
    if (bc < 256) bc = 256;
    if (bc > (dwt ? BUCKET_MAX_DWT : BUCKET_MAX)) bc = dwt ? BUCKET_MAX_DWT : BUCKET_MAX;
    *nsub_log2 = lg;
    *bucket_cap = (int)bc;
}

int64_t cap_for(int64_t n, bool dwt) {
    int lg, bc;
    bucket_plan(n, &lg, &bc, dwt);
    return (int64_t)bc << lg;
}

int read_shape(const wtp_tensor& x, int t, bool check_ptrs, TPlan& p) {
    if (x.ndim < 0 || x.ndim > WTP_MAX_DIMS) return fail(WTP_EARG, t, "tensor %d: ndim %d unsupported", t, x.ndim);
    p.ndim = x.ndim;
    p.numel = 1;
    for (int d = 0; d < x.ndim; ++d) {
        if (x.shape[d] < 0) return fail(WTP_EARG, t, "tensor %d: negative dimension", t);
        p.numel *= x.shape[d];
    }
    if (check_ptrs && p.numel > 0 && (!x.in || !x.out)) return fail(WTP_EARG, t, "tensor %d: null pointer", t);
    return WTP_OK;
}

void plan_image(TPlan& p, int64_t B, int64_t H, int64_t W, int L, int F, int mode) {
    p.B = B;
    p.H = H;
    p.W = W;
    p.L = L;
    p.dwt = L > 0;
    p.mode = p.dwt ? mode : WTP_MODE_PERIODIZATION;
    wtm_geom(H, W, L, F, p.mode, &p.g);
    p.pop = B * p.g.PR * p.g.PC;
    p.tight = wtm_block_cells(&p.g, L) == p.g.PR * p.g.PC;
}

static int bad_wavelet(int t) {
    return fail(WTP_EBADWAVELET, t, "Unknown wavelet name, check wavelist() for the list of available builtin wavelets.");
}
/* the clamped level of a tensor whose transform is max_level(n, F) levels deep at most; the clamp
 * is carried in *cur_level (dwt_pruning.py:64-65) */
static int clamp_level(int64_t n, int F, int t, int* cur_level) {
    const int maxL = max_level(n, F);
    if (maxL < *cur_level) *cur_level = maxL;
    if (*cur_level < 0) return fail(WTP_EBADLEVEL, t, "Level value of %d is too low . Minimum level is 0.", *cur_level);
    if (*cur_level > 32) return fail(WTP_EARG, t, "tensor %d: level %d unsupported", t, *cur_level);
    return WTP_OK;
}

int plan_tensors(const wtp_tensor* ts, int n, int wid, int level, double pct, bool check_ptrs, std::vector<TPlan>& out,
                 bool carry, bool flat, int mode) {
    out.assign(n, TPlan());
    int cur_level = level;
    for (int t = 0; t < n; ++t) {
        if (!carry) cur_level = level;
        const wtp_tensor& x = ts[t];
        TPlan& p = out[t];
        int rc = read_shape(x, t, check_ptrs, p);
        if (rc != WTP_OK) return rc;
        if (x.ndim < 2) {
            /* dwt_pruning.py:58-62 -- plain percentile, no wavelet lookup */
            if (!pct_ok(pct)) return fail(WTP_EBADPCT, t, "Percentiles must be in the range [0, 100]");
            if (p.numel == 0) return fail(WTP_EEMPTY, t, "index -1 is out of bounds for axis 0 with size 0");
            p.L = cur_level;
            p.pop = p.numel;
        } else if (flat) {
            /* 1-D flattened mode: pywt.wavedec(w.ravel(), wavelet, 'periodization', level) with
             * the level clamped as calculate_max_level clamps it for the 2-D path (:12-13, :64-65) */
            if (!wavelet_known(wid)) return bad_wavelet(t);
            p.flat = true;
            if ((rc = clamp_level(p.numel, wt_flen[wid], t, &cur_level)) != WTP_OK) return rc;
            p.L = cur_level;
            if (!pct_ok(pct)) return fail(WTP_EBADPCT, t, "Percentiles must be in the range [0, 100]");
            p.len[0] = p.numel;
            for (int k = 1; k <= p.L; ++k) p.len[k] = (p.len[k - 1] + 1) / 2;
            p.pop = p.len[p.L];
            for (int k = 1; k <= p.L; ++k) p.pop += p.len[k];
            if (p.pop == 0) return fail(WTP_EEMPTY, t, "index -1 is out of bounds for axis 0 with size 0");
            p.dwt = p.L > 0;
        } else {
            if (!wavelet_known(wid)) return bad_wavelet(t);
            const int64_t H = x.shape[x.ndim - 2], W = x.shape[x.ndim - 1];
            int64_t B = 1;
            for (int d = 0; d < x.ndim - 2; ++d) B *= x.shape[d];
            const int F = wt_flen[wid];
            if ((rc = clamp_level(std::min(H, W), F, t, &cur_level)) != WTP_OK) return rc;
            p.L = cur_level;
            if (p.L > 0 && mode && !wtm_levels_ok(H, W, p.L, F, mode))
                return fail(WTP_EARG, t, "tensor %d: the mode cannot extend its lines (an odd filter length, or reflect "
                            "of a one-sample line)", t);
            plan_image(p, B, H, W, p.L, F, mode);
            if (!pct_ok(pct)) return fail(WTP_EBADPCT, t, "Percentiles must be in the range [0, 100]");
            if (p.pop == 0) return fail(WTP_EEMPTY, t, "index -1 is out of bounds for axis 0 with size 0");
            if (p.dwt) {
                if (p.mode && p.B <= (int64_t)INT32_MAX) p.tiny_lg = wtm_tiny_lanes_log2(p.H, p.W, p.L, F);
                /* waverec2 yields (2R1, 2C1), under an extension mode (2R1 - F + 2, 2C1 - F + 2);
                 * the 4-index crop of :79-82 then fails for 2-D/3-D
                 * tensors (IndexError), cannot crop W for 5-D or anything for >= 6-D (the
                 * later .view(original_shape) raises RuntimeError) */
                const bool hbad = wtm_out_len(p.g.R[1], F, p.mode) != p.H, wbad = wtm_out_len(p.g.C[1], F, p.mode) != p.W;
                if ((x.ndim < 4 && (hbad || wbad)) || (x.ndim == 5 && wbad) || (x.ndim >= 6 && (hbad || wbad)))
                    return fail(WTP_ECROP, t, x.ndim < 4 ? "tuple index out of range"
                                                         : "shape is invalid for input of this size");
            }
        }
        /* selection counts are kept in 32 bits on the device (8 GiB of float32 per tensor) */
        if (p.pop > (int64_t)INT32_MAX) return fail(WTP_EARG, t, "tensor %d: more than 2^31-1 coefficients", t);
        p.cap = cap_for(p.pop, p.dwt);
    }
    return WTP_OK;
}

/* Whether one level of p, whose larger side (the analysis input / the synthesis output) is
 * (B, R, C), runs in the tiled kernels.  The percentile path clamps the level, so its levels
 * always have an input of at least 2 (F - 1) and an output of at least F - 1 samples a side, and
 * the tiled kernels were written for that (k_inv_int's edge form wraps a coordinate once).  A
 * plan with unclamped levels (strict) holds every level to the same bound: shorter sides take
 * the per-point kernels, which wrap any number of times (wt_dwt_core.h). */
bool lvl_tiled(const TPlan& p, int64_t B, int64_t R, int64_t C, const Taps& tp) {
    if (!fb_tiled_ok(B, R, C, tp)) return false;
    return !p.strict || std::min(R, C) >= 2 * (int64_t)(tp.F - 1);
}

/* Elements one level temp of tensor p needs: the largest intermediate its forward and inverse
 * write to a temp, level by level, with the kernels forward_chains / inverse_chains pick (tiled:
 * the next approximation / the synthesis output below level 1; per-point: the column pass's two
 * outputs / the row pass's two outputs).  Level 1's synthesis writes the caller's output. */
size_t temp_elems(const TPlan& p, const Taps& tp) {
    if (p.flat) return (size_t)p.numel + 2; /* two ping-pong lines of up to numel + 1 samples */
    int64_t need = 0;
    if (p.mode) { /* modes.hip: a half transform of either direction (R[k] x C[k-1]), an approximation */
        if (p.tiny_lg >= 0) return 0;
        for (int k = 1; k <= p.L; ++k) need = std::max(need, p.B * p.g.R[k] * std::max(p.g.C[k - 1], p.g.C[k]));
        return (size_t)need;
    }
    for (int k = 1; k <= p.L; ++k) {
        const int64_t R0 = p.g.R[k - 1], C0 = p.g.C[k - 1], R = p.g.R[k], C = p.g.C[k];
        need = std::max(need, p.B * R * (lvl_tiled(p, p.B, R0, C0, tp) ? C : C0));
        if (!lvl_tiled(p, p.B, 2 * R, 2 * C, tp)) need = std::max(need, p.B * R * 2 * C);
        if (k >= 2) need = std::max(need, p.B * 4 * R * C);
    }
    return (size_t)need;
}

/* Fused selection (wtp_internal.h, FwdSel / k_fwin / k_fslot_collect): a tensor qualifies when
 * it is large (its window pass and bucket pass are then small beside the P re-read they replace),
 * tight (every packed coefficient is written by the forward: no padding zeros in the population),
 * its images hold k_fwin's patches and its level count leaves them at least 4 x 4, and every
 * forward level runs in k_fwd_int.  Returns the wave slots of its forward, 0 when it does not
 * qualify.  `sizing`: the workspace query -- the interior mode and the input's alignment are
 * not known yet, so the slots are reserved whenever the shape qualifies. */
constexpr int64_t FUSED_MIN_POP = (int64_t)1 << 22;
int64_t fused_slot_count(const TPlan& p, const float* in, const Taps& tp, bool sizing) {
    if (!p.dwt || p.flat || p.mode || !p.tight || p.L < 1 || p.L > 6 || p.pop < FUSED_MIN_POP) return 0;
    if (p.g.R[0] < FWIN_PS || p.g.C[0] < FWIN_PS) return 0;
    int64_t tot = 0;
    for (int k = 1; k <= p.L; ++k) {
        /* level 1 reads the caller's input, the others a 256-byte aligned temp */
        const float* src = (k == 1 && !sizing) ? in : reinterpret_cast<const float*>((uintptr_t)ALIGN);
        const FwdItem x{src, p.B, p.g.R[k - 1], p.g.C[k - 1], nullptr, nullptr, p.g.PR, p.g.PC, p.g.offR[k], p.g.offC[k],
                        k == p.L};
        int64_t sl = 0;
        if (!fwd_level_fused_ok(x, tp, &sl, sizing)) return 0;
        tot += sl;
    }
    return tot;
}

/* persistent slot region: identical position and size in every layout */
constexpr size_t PERSIST_BYTES = ((sizeof(SelHeader) + 2 * SEL_REGION) + 255) / 256 * 256;

Layout make_layout(std::vector<TPlan>& ps, const Taps& tp) {
    Layout L;
    L.hist = 0;
    L.sel = 0;
    size_t off = PERSIST_BYTES;
    L.thr = off;
    off = align_up(off + ps.size() * sizeof(float));
    L.cand = off;
    size_t ce = 0;
    for (auto& p : ps) { p.cand_off = ce; ce += (size_t)p.cap; }
    /* a resident launch (k_resident) keeps one published region of RES_WG_WORDS per workgroup there instead */
    int64_t rwg = 0;
    for (auto& p : ps)
        if (!p.dwt) rwg += (p.pop + RES_CHUNK - 1) / RES_CHUNK;
    ce = std::max(ce, (size_t)std::min<int64_t>(rwg, RES_MAX_WG) * RES_WG_WORDS);
    /* the one-launch small path keeps one slot of SM_SLOT_WORDS per workgroup there */
    ce = std::max(ce, (size_t)RES_MAX_WG * SM_SLOT_WORDS);
    off = align_up(off + ce * sizeof(uint32_t));
    L.P = off;
    for (auto& p : ps) {
        if (!p.dwt) continue;
        p.p_off = off;
        off = align_up(off + (size_t)p.pop * sizeof(float));
    }
    /* level temps per launch-group SLOT (tensor t uses slot t % SEG_PER_LAUNCH), not per tensor:
     * the same level of one launch group's tensors runs as one grouped launch, so their temps are
     * live together, but the groups' transforms run one group after another on the caller's
     * stream (prune_impl; the side stream only selects from P), so group g + 1 reuses group g's
     * temps.  cfg5 (64 x 4096^2, db8 L5): 24 slots x 3 x 16.8 MB instead of 64 x 3 x 67 MB */
    size_t slot_elems[SEG_PER_LAUNCH] = {};
    for (size_t t = 0; t < ps.size(); ++t)
        if (ps[t].dwt) slot_elems[t % SEG_PER_LAUNCH] = std::max(slot_elems[t % SEG_PER_LAUNCH], temp_elems(ps[t], tp));
    size_t slot_off[SEG_PER_LAUNCH] = {};
    for (int j = 0; j < SEG_PER_LAUNCH; ++j) {
        if (!slot_elems[j]) continue;
        slot_off[j] = off;
        off = align_up(off + 3 * align_up(slot_elems[j] * sizeof(float)));
    }
    for (size_t t = 0; t < ps.size(); ++t) {
        if (!ps[t].dwt) continue;
        ps[t].t_off = slot_off[t % SEG_PER_LAUNCH];
        ps[t].t_elems = slot_elems[t % SEG_PER_LAUNCH];
    }
    /* fused selection's wave slots, also per launch-group slot: a fused group's bucket pass reads
     * them before the next group's forward writes its own */
    size_t fsl_words[SEG_PER_LAUNCH] = {};
    for (size_t t = 0; t < ps.size(); ++t) {
        ps[t].f_slots = fused_slot_count(ps[t], nullptr, tp, true);
        if (ps[t].f_slots)
            fsl_words[t % SEG_PER_LAUNCH] =
                std::max(fsl_words[t % SEG_PER_LAUNCH], (size_t)FSL_HDR_WORDS + (size_t)ps[t].f_slots * FSL_WORDS);
    }
    /* two sets when the call has several groups: group g uses set g & 1, so group g + 1's forward
     * fills its slots while group g's bucket pass (side stream) still reads its own */
    const int nsets = ps.size() > (size_t)SEG_PER_LAUNCH ? 2 : 1;
    size_t fsl_off[2][SEG_PER_LAUNCH] = {};
    for (int k = 0; k < nsets; ++k)
        for (int j = 0; j < SEG_PER_LAUNCH; ++j) {
            if (!fsl_words[j]) continue;
            fsl_off[k][j] = off;
            off = align_up(off + fsl_words[j] * sizeof(uint32_t));
        }
    bool anyf = false;
    for (size_t t = 0; t < ps.size(); ++t)
        if (ps[t].f_slots) { ps[t].f_off = fsl_off[(t / SEG_PER_LAUNCH) & 1][t % SEG_PER_LAUNCH]; anyf = true; }
    if (anyf) {
        L.fwh = off;
        off = align_up(off + FWIN_HIST_BYTES);
    }
    L.total = off;
    return L;
}

size_t layout_bytes(const wtp_tensor* ts, int n, int wid, int level, bool carry, bool flat, int mode) {
    std::vector<TPlan> ps;
    if (plan_tensors(ts, n, wid, level, 50.0, false, ps, carry, flat, mode) != WTP_OK) return 0;
    return make_layout(ps, taps_for(wid)).total;
}

void seg_ranks(int64_t n, double pct, SegDesc& sd) {
    /* numpy/lib/function_base.py: q = pct/100 (:4279); linear vi = (n-1)*q (:110);
     * _get_indexes (:4730-4763): vi >= n-1 -> index -1 (the max), gamma = vi - (-1) */
    const double q = pct / 100.0;
    const double vi = (double)(n - 1) * q;
    if (vi >= (double)(n - 1)) {
        sd.above = 1;
        sd.r0 = n - 1;
        sd.gamma = vi - (-1.0);
    } else {
        const double fl = std::floor(vi);
        sd.above = 0;
        sd.r0 = (int64_t)fl;
        sd.gamma = vi - fl;
    }
}

SegDesc& seg_add(SegTable& tab, const TPlan& p, const float* data, float* out, int res, int flags, int nblk) {
    SegDesc& sd = tab.s[tab.nseg];
    sd.data = data;
    sd.out = out;
    sd.n = p.pop;
    sd.numel = p.numel;
    sd.blk_begin = tab.blk_begin[tab.nseg] = tab.nblk;
    tab.nblk += nblk;
    sd.slot = tab.nseg++;
    sd.res = res;
    sd.eff_level = p.L;
    sd.flags = flags;
    const uintptr_t a = reinterpret_cast<uintptr_t>(data), o = reinterpret_cast<uintptr_t>(out);
    if ((a % 16) == 0 && (o % 16) == 0) sd.flags |= SEG_ALIGNED;
    sd.cand_off = (int64_t)p.cand_off;
    sd.cap = p.cap;
    bucket_plan(p.pop, &sd.nsub_log2, &sd.bucket_cap, p.dwt);
    return sd;
}

void seg_close(SegTable& tab) {
    for (int i = tab.nseg; i < SEG_PER_LAUNCH; ++i) tab.blk_begin[i] = INT32_MAX;
}

}  // namespace wtp

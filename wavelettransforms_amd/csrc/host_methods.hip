/*
 * host_methods.hip -- the entries beside the percentile path: min-weight pruning, random pruning,
 * the sparsity count, the absolute-threshold method and its sweep, the transform components and the synthetic
 * inputs.  Each validates with its own rules on top of read_shape / plan_image (host_plan.hip).
 */
#include <type_traits>

#include "wtp_host.h"
#include "wt_perm.h"

using namespace wtp;

/* ---------------------------------------------------------- min pruning --- */
/* percentage_min_pruning (ResNet/min_weight_pruning.py:66-74): k = int(numel * fraction)
 * (Python int(): truncation toward zero); torch.topk rejects k outside [0, numel]. */
struct MinPlan {
    std::vector<TPlan> ps;
    std::vector<int64_t> k;
    Layout lay;
    size_t mp_off = 0, tie_off = 0, total = 0;
    int nblk = 0;
};

static int plan_min(const wtp_tensor* ts, int n, double fraction, bool check_ptrs, MinPlan& m) {
    m.ps.assign(n, TPlan());
    m.k.assign(n, 0);
    if (!(fraction == fraction)) return fail(WTP_EARG, -1, "cannot convert float NaN to integer");
    for (int t = 0; t < n; ++t) {
        TPlan& p = m.ps[t];
        const int rc = read_shape(ts[t], t, check_ptrs, p);
        if (rc != WTP_OK) return rc;
        if (p.numel > (int64_t)INT32_MAX) return fail(WTP_EARG, t, "tensor %d: more than 2^31-1 elements", t);
        const double kd = (double)p.numel * fraction; /* min_weight_pruning.py:70 */
        if (!(kd > -1.0 && kd < (double)p.numel + 1.0))
            return fail(WTP_EARG, t, "selected index k out of range");
        m.k[t] = (int64_t)kd; /* C cast truncates toward zero, like int() */
        p.pop = p.numel;
        p.cap = p.numel ? cap_for(p.pop, false) : 0;
        m.nblk += (int)((p.pop + CHUNK - 1) / CHUNK);
    }
    m.lay = make_layout(m.ps, Taps{}); /* level-0 populations only: no temps */
    m.mp_off = align_up(m.lay.total);
    m.tie_off = align_up(m.mp_off + (size_t)n * 16);
    m.total = align_up(m.tie_off + (size_t)(m.nblk + 1) * sizeof(uint32_t));
    return WTP_OK;
}

/* ------------------------------------------- the absolute-threshold method --- */
/* dwt_pruning_NoEntropy.py:29-60.  Workspace: [the float32 threshold, one word on a line of its
 * own | one chain region: a packed array and three level temps, sized for the largest chain
 * tensor -- the chain tensors run one after another on the stream and share it]. */
struct AbsPlan {
    std::vector<TPlan> ps;
    std::vector<int> path;
    std::vector<int> nl_log2; /* tiny: lanes a wave uses */
    size_t p_bytes = 0, t_bytes = 0, total = 0;
};

static int plan_abs(const wtp_tensor* ts, int n, int wid, int level, bool check_ptrs, AbsPlan& a) {
    a.ps.assign(n, TPlan());
    a.path.assign(n, WTP_ABS_PATH_MASK);
    a.nl_log2.assign(n, 0);
    const Taps tp = taps_for(wid);
    for (int t = 0; t < n; ++t) {
        const wtp_tensor& x = ts[t];
        TPlan& p = a.ps[t];
        const int rc = read_shape(x, t, check_ptrs, p);
        if (rc != WTP_OK) return rc;
        p.strict = true;
        if (x.ndim < 2) { /* :35-38 -- a plain mask, no wavelet lookup, no level */
            p.pop = p.numel;
            continue;
        }
        if (!wavelet_known(wid))
            return fail(WTP_EBADWAVELET, t, "Unknown wavelet name, check wavelist() for the list of available builtin wavelets.");
        if (level < 0) return fail(WTP_EBADLEVEL, t, "Level value of %d is too low . Minimum level is 0.", level);
        if (level > 32) return fail(WTP_EARG, t, "tensor %d: level %d unsupported", t, level);
        if (p.numel == 0) return fail(WTP_EARG, t, "tensor %d: empty tensor with ndim >= 2", t);
        const int64_t H = x.shape[x.ndim - 2], W = x.shape[x.ndim - 1];
        plan_image(p, p.numel / (H * W), H, W, level, tp.F, WTP_MODE_PERIODIZATION);
        const int lg = p.B <= (int64_t)INT32_MAX ? abs_lanes_log2(p.H, p.W, p.L) : -1;
        if (lg >= 0) {
            a.path[t] = WTP_ABS_PATH_TINY;
            a.nl_log2[t] = lg;
            continue;
        }
        if (!p.dwt) continue;
        a.path[t] = WTP_ABS_PATH_CHAIN;
        p.t_elems = temp_elems(p, tp);
        a.p_bytes = std::max(a.p_bytes, align_up((size_t)p.pop * sizeof(float)));
        a.t_bytes = std::max(a.t_bytes, align_up(p.t_elems * sizeof(float)));
    }
    a.total = ALIGN + a.p_bytes + 3 * a.t_bytes;
    return WTP_OK;
}

/* np.abs(a_f32) < python_float compares in float32 with the threshold rounded to float32 */
static AbsThr abs_thr(const double* thresholds, int nthr) {
    AbsThr thr;
    memset(&thr, 0, sizeof thr);
    thr.n = nthr;
    for (int k = 0; k < nthr; ++k) {
        const float t32 = (float)thresholds[k];
        memcpy(&thr.bits[k], &t32, 4);
    }
    return thr;
}

/* Every tiny-image tensor of the call, as many per launch as the table -- the kernel's argument --
 * has segments (AbsTable: ABS_MAX_SEG, AbsSweepTable: ABS_SWEEP_MAX_SEG).  `head` is a table without
 * segments, its call-wide fields set; set_out(sg, t) gives tensor t's segment its output(s). */
template <class Table, class SetOut>
static void abs_tiny_launches(const Table& head, const wtp_tensor* tensors, int ntensors, const AbsPlan& a,
                              const SetOut& set_out, wtp_abs_result* results, hipStream_t s) {
    constexpr int max_seg = (int)std::extent<decltype(Table::s)>::value;
    Table tab = head;
    for (int t = 0; t <= ntensors; ++t) {
        const bool tiny = t < ntensors && a.path[t] == WTP_ABS_PATH_TINY;
        const bool flush = t == ntensors || tab.nseg == max_seg ||
                           (tiny && (int64_t)tab.nwave + tiny_waves(a.ps[t].B, a.nl_log2[t]) > (int64_t)INT32_MAX);
        if (flush && tab.nseg) {
            launch_abs_tiny(tab, results, s);
            tab = head;
        }
        if (!tiny) continue;
        const TPlan& p = a.ps[t];
        auto& sg = tiny_append(tab, tensors[t].in, p.B, p.H, p.W, p.L, a.nl_log2[t]);
        sg.res = t;
        set_out(sg, t);
    }
}

/* The launch sequence of both absolute-threshold entries: thr.n thresholds, tensor t's output at
 * threshold k in outs[k * n + t] and its record in results[k * n + t].  `sweep` picks the tiny
 * kernel and nothing else: k_abs_tiny_sweep whatever thr.n is, or k_abs_tiny (thr.n == 1), which
 * is the faster of the two for one threshold. */
static int abs_run(const wtp_tensor* tensors, int n, const AbsPlan& a, const Taps& tp, const AbsThr& thr,
                   float* const* outs, bool sweep, void* ws, wtp_abs_result* results, hipStream_t s) {
    static_assert(WTP_ABS_SWEEP_MAX_THR == ABS_SWEEP_MAX_THR && ABS_SWEEP_MAX_THR * sizeof(float) <= ALIGN,
                  "the threshold words fit the workspace's first line");
    float* thr_dev = reinterpret_cast<float*>(ws);
    bool any_other = false;
    for (int t = 0; t < n; ++t) any_other = any_other || (a.path[t] != WTP_ABS_PATH_TINY && a.ps[t].numel > 0);
    /* the counts are accumulated: every record starts from zero (an empty tensor's stays so); the
     * mask and the inverse read their threshold from device memory: the same launch sets the words */
    launch_abs_init(results, thr.n * n, any_other ? thr_dev : nullptr, thr, s);
    /* 1. every tiny-image tensor: read, taken forward and counted once, all thresholds in the launch */
    if (sweep) {
        AbsSweepTable head;
        memset(&head, 0, sizeof head);
        head.ntensors = n;
        head.thr = thr;
        head.tp = tp;
        abs_tiny_launches(head, tensors, n, a, [&](AbsSweepSeg& sg, int t) {
            for (int k = 0; k < thr.n; ++k) sg.out[k] = outs[(size_t)k * n + t];
        }, results, s);
    } else {
        AbsTable head;
        memset(&head, 0, sizeof head);
        head.thr_bits = thr.bits[0];
        head.tp = tp;
        abs_tiny_launches(head, tensors, n, a, [&](AbsSeg& sg, int t) { sg.out = outs[t]; }, results, s);
    }
    /* 2. the others, one after another: count_nonzero(in) and (chain) the forward transform once,
     * before any output is written; then per threshold the mask or the inverse with that
     * threshold's word on the load, and count_nonzero of that output.  An output that is the
     * input goes last: the mask reads the input for every threshold. */
    float* P = wsb<float>(ws, ALIGN);
    for (int t = 0; t < n; ++t) {
        const TPlan& p = a.ps[t];
        if (a.path[t] == WTP_ABS_PATH_TINY || p.numel == 0) continue;
        const bool chain = a.path[t] == WTP_ABS_PATH_CHAIN;
        wtp_abs_result init;
        memset(&init, 0, sizeof init);
        init.numel = p.numel;
        init.coeff_numel = p.pop;
        init.level = p.ndim >= 2 ? p.L : 0;
        init.path = a.path[t];
        launch_abs_count_in(tensors[t].in, p.numel, results + t, n, thr, init, s);
        /* one chain: the forward reads its `in`, each inverse its `out` and `thr` */
        Chain c = make_chain(p, tensors[t].in, nullptr, P, wsb(ws, ALIGN + a.p_bytes), a.t_bytes, nullptr, nullptr);
        if (chain) {
            if (!p.tight) launch_abs_zero(P, p.pop, s);
            forward_chains({c}, tp, s);
        }
        int order[WTP_ABS_SWEEP_MAX_THR], no = 0;
        for (int k = 0; k < thr.n; ++k)
            if (outs[(size_t)k * n + t] != tensors[t].in) order[no++] = k;
        for (int k = 0; k < thr.n; ++k)
            if (outs[(size_t)k * n + t] == tensors[t].in) order[no++] = k;
        for (int i = 0; i < thr.n; ++i) {
            const int k = order[i];
            const size_t ri = (size_t)k * n + t;
            if (chain) {
                c.out = outs[ri];
                c.thr = thr_dev + k;
                inverse_chains({c}, tp, s);
            } else {
                launch_copy_threshold(tensors[t].in, outs[ri], p.numel, thr_dev + k, nullptr, s);
            }
            launch_abs_count(outs[ri], p.numel, reinterpret_cast<unsigned long long*>(&results[ri].nonzero_out), s);
        }
    }
    return check_launch();
}

/* ---------------------------------------------------------- components --- */
/* the requested level as given (no clamp); under an extension mode the per-level kernels of
 * modes.hip (level 0 and WTP_MODE_PERIODIZATION: the periodized plan) */
static int component_plan(int64_t B, int64_t H, int64_t W, int wid, int level, int mode_id, TPlan& p) {
    int rc = mode_check(mode_id, 0);
    if (rc != WTP_OK) return rc;
    if (!wavelet_known(wid)) return fail(WTP_EBADWAVELET, -1, "Unknown wavelet name");
    if (level < 0) return fail(WTP_EBADLEVEL, -1, "Level value of %d is too low . Minimum level is 0.", level);
    if (level > 32 || B < 0 || H <= 0 || W <= 0) return fail(WTP_EARG, -1, "bad component arguments");
    const int F = wavelet_flen(wid);
    if (level > 0 && !wtm_levels_ok(H, W, level, F, mode_id))
        return fail(WTP_EARG, -1, "the mode cannot extend a %lld x %lld image under a %d-tap filter at level %d",
                    (long long)H, (long long)W, F, level);
    plan_image(p, B, H, W, level, F, mode_id);
    if (p.mode && p.pop > (int64_t)INT32_MAX) return fail(WTP_EARG, -1, "more than 2^31-1 coefficients");
    return WTP_OK;
}

/* the three level temps of a component call: the public periodized formula, or the mode kernels' */
static size_t component_ws_bytes(const TPlan& p) {
    if (!p.mode) return wtp_dwt_workspace_size(p.B, p.H, p.W, p.L);
    return 3 * align_up(temp_elems(p, Taps{}) * sizeof(float));
}

static int wavedec2_impl(const float* in, float* packed, int64_t B, int64_t H, int64_t W, int wid, int level, int mode_id,
                         void* ws, size_t ws_bytes, wtp_stream_t stream) {
    TPlan p;
    int rc = component_plan(B, H, W, wid, level, mode_id, p);
    if (rc != WTP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (level == 0) {
        if (hipMemcpyAsync(packed, in, (size_t)(B * H * W) * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(WTP_EHIP, -1, "hipMemcpyAsync failed");
        return WTP_OK;
    }
    const size_t need = component_ws_bytes(p);
    if (!ws || ws_bytes < need) return fail(WTP_EWORKSPACE, -1, "workspace too small: need %zu", need);
    if (!p.tight && hipMemsetAsync(packed, 0, (size_t)p.pop * sizeof(float), s) != hipSuccess)
        return fail(WTP_EHIP, -1, "hipMemsetAsync failed");
    forward_chains({make_chain(p, in, nullptr, packed, ws, need / 3, nullptr, nullptr)}, taps_for(wid), s);
    return check_launch();
}

static int waverec2_impl(const float* packed, float* out, int64_t B, int64_t H, int64_t W, int wid, int level, int mode_id,
                         const float* thr32, void* ws, size_t ws_bytes, wtp_stream_t stream) {
    TPlan p;
    int rc = component_plan(B, H, W, wid, level, mode_id, p);
    if (rc != WTP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (level == 0) {
        launch_copy_threshold(packed, out, B * H * W, thr32, nullptr, s);
        return check_launch();
    }
    const size_t need = component_ws_bytes(p);
    if (!ws || ws_bytes < need) return fail(WTP_EWORKSPACE, -1, "workspace too small: need %zu", need);
    inverse_chains({make_chain(p, nullptr, out, const_cast<float*>(packed), ws, need / 3, thr32, nullptr)}, taps_for(wid), s);
    return check_launch();
}

extern "C" {

size_t wtp_min_prune_workspace_size(const wtp_tensor* tensors, int ntensors, double fraction) {
    if (ntensors < 0 || (ntensors > 0 && !tensors)) return 0;
    MinPlan m;
    if (plan_min(tensors, ntensors, fraction, false, m) != WTP_OK) return 0;
    return m.total;
}

int wtp_min_prune_f32(const wtp_tensor* tensors, int ntensors, double fraction, void* ws, size_t ws_bytes,
                      wtp_result* results, wtp_stream_t stream) {
    clear_error();
    if (ntensors < 0 || (ntensors > 0 && (!tensors || !results))) return fail(WTP_EARG, -1, "bad arguments");
    if (ntensors == 0) return WTP_OK;
    MinPlan m;
    int rc = plan_min(tensors, ntensors, fraction, true, m);
    if (rc != WTP_OK) return rc;
    if (!ws || ws_bytes < m.total)
        return fail(WTP_EWORKSPACE, -1, "workspace too small: need %zu bytes, got %zu", m.total, ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    SelHeader* head = wsb<SelHeader>(ws, m.lay.sel);
    uint32_t* cand = wsb<uint32_t>(ws, m.lay.cand);
    float* thr_t = wsb<float>(ws, m.lay.thr);
    void* mp = wsb(ws, m.mp_off);
    uint32_t* tiecnt = wsb<uint32_t>(ws, m.tie_off);
    /* empty tensors: nothing to select; their records are zero */
    for (int t = 0; t < ntensors; ++t)
        if (m.ps[t].numel == 0 && hipMemsetAsync(results + t, 0, sizeof(wtp_result), s) != hipSuccess)
            return fail(WTP_EHIP, t, "hipMemsetAsync failed");
    std::vector<int> live;
    for (int t = 0; t < ntensors; ++t)
        if (m.ps[t].numel > 0) live.push_back(t);
    for (size_t g0 = 0; g0 < live.size(); g0 += SEG_PER_LAUNCH) {
        SegTable tab;
        memset(&tab, 0, sizeof tab);
        for (size_t j = g0; j < live.size() && j < g0 + SEG_PER_LAUNCH; ++j) {
            const int t = live[j];
            const TPlan& p = m.ps[t];
            SegDesc& sd = seg_add(tab, p, tensors[t].in, tensors[t].out, t, SEG_MINPRUNE | (m.k[t] == 0 ? SEG_KZERO : 0),
                                  (int)((p.pop + CHUNK - 1) / CHUNK));
            sd.above = 1; /* one rank: r1 = r0 */
            sd.gamma = 0.0;
            sd.r0 = m.k[t] > 0 ? m.k[t] - 1 : 0;
        }
        seg_close(tab);
        launch_window(tab, head, s);
        launch_collect(tab, head, cand, results, s);
        launch_minprune(tab, head, cand, results, thr_t, mp, tiecnt, s);
    }
    return check_launch();
}

/* ---------------------------------------------------------- random pruning --- */
int wtp_random_prune_f32(const wtp_tensor* tensors, int ntensors, const int64_t* prune_counts, uint64_t seed,
                         wtp_result* results, wtp_stream_t stream) {
    clear_error();
    if (ntensors < 0 || (ntensors > 0 && (!tensors || !results || !prune_counts))) return fail(WTP_EARG, -1, "bad arguments");
    if (ntensors == 0) return WTP_OK;
    std::vector<int64_t> numel(ntensors), keff(ntensors);
    for (int t = 0; t < ntensors; ++t) {
        TPlan p; /* no 2^31 limit here: only the shape is read */
        const int rc = read_shape(tensors[t], t, true, p);
        if (rc != WTP_OK) return rc;
        const int64_t k = prune_counts[t], n = p.numel;
        numel[t] = n;
        keff[t] = k >= 0 ? std::min(k, n) : std::max<int64_t>(0, n + k); /* randperm(n)[:k], Python slicing */
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(results, 0, sizeof(wtp_result) * (size_t)ntensors, s) != hipSuccess)
        return fail(WTP_EHIP, -1, "hipMemsetAsync failed");
    for (int g0 = 0; g0 < ntensors; g0 += SEG_PER_LAUNCH) {
        RandTable tab;
        memset(&tab, 0, sizeof tab);
        int cb = 0, zb = 0;
        for (int t = g0; t < ntensors && t < g0 + SEG_PER_LAUNCH; ++t) {
            RandSeg& sg = tab.s[tab.nseg];
            sg.in = tensors[t].in;
            sg.out = tensors[t].out;
            sg.numel = numel[t];
            sg.k = keff[t];
            sg.key = wt_perm_key(seed, (uint32_t)t);
            sg.h = wt_perm_half_bits((uint64_t)numel[t]);
            sg.res = t;
            tab.copy_begin[tab.nseg] = cb;
            tab.zero_begin[tab.nseg] = zb;
            cb += (int)((numel[t] + CHUNK - 1) / CHUNK);
            zb += (int)((keff[t] + STREAM_THREADS - 1) / STREAM_THREADS);
            ++tab.nseg;
        }
        tab.copy_begin[tab.nseg] = cb;
        tab.zero_begin[tab.nseg] = zb;
        for (int i = tab.nseg + 1; i <= SEG_PER_LAUNCH; ++i) { tab.copy_begin[i] = cb; tab.zero_begin[i] = zb; }
        launch_random_prune(tab, results, s);
    }
    return check_launch();
}

int wtp_count_small_f32(const float* x, int64_t n, float thr, unsigned long long* count_dev, wtp_stream_t stream) {
    if (n < 0 || (n > 0 && !x) || !count_dev) return fail(WTP_EARG, -1, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count_dev, 0, sizeof(unsigned long long), s) != hipSuccess)
        return fail(WTP_EHIP, -1, "hipMemsetAsync failed");
    if (n > 0) launch_count_small(x, n, thr, count_dev, s);
    return check_launch();
}

size_t wtp_abs_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level) {
    if (ntensors < 0 || (ntensors > 0 && !tensors)) return 0;
    AbsPlan a;
    if (plan_abs(tensors, ntensors, wavelet_id, level, false, a) != WTP_OK) return 0;
    return a.total;
}

int wtp_prune_abs_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double threshold, void* ws,
                      size_t ws_bytes, wtp_abs_result* results, wtp_stream_t stream) {
    clear_error();
    if (ntensors < 0 || (ntensors > 0 && (!tensors || !results))) return fail(WTP_EARG, -1, "bad arguments");
    if (ntensors == 0) return WTP_OK;
    AbsPlan a;
    int rc = plan_abs(tensors, ntensors, wavelet_id, level, true, a);
    if (rc != WTP_OK) return rc;
    if (!ws || ws_bytes < a.total)
        return fail(WTP_EWORKSPACE, -1, "workspace too small: need %zu bytes, got %zu", a.total, ws_bytes);
    std::vector<float*> outs(ntensors);
    for (int t = 0; t < ntensors; ++t) outs[t] = tensors[t].out;
    return abs_run(tensors, ntensors, a, taps_for(wavelet_id), abs_thr(&threshold, 1), outs.data(), false, ws, results,
                   (hipStream_t)stream);
}

/* ---- the absolute-threshold sweep: one forward per tensor, every threshold's mask and inverse.
 * plan_abs's plan and workspace; the line at its start holds a float32 word per threshold. ---- */
size_t wtp_abs_sweep_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int nthr) {
    if (ntensors < 0 || (ntensors > 0 && !tensors) || nthr < 1 || nthr > WTP_ABS_SWEEP_MAX_THR) return 0;
    AbsPlan a;
    if (plan_abs(tensors, ntensors, wavelet_id, level, false, a) != WTP_OK) return 0;
    return a.total;
}

int wtp_prune_abs_sweep_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, const double* thresholds,
                            int nthr, float* const* outs, void* ws, size_t ws_bytes, wtp_abs_result* results,
                            wtp_stream_t stream) {
    clear_error();
    if (ntensors < 0 || (ntensors > 0 && (!tensors || !results))) return fail(WTP_EARG, -1, "bad arguments");
    if (nthr < 1 || nthr > WTP_ABS_SWEEP_MAX_THR || !thresholds)
        return fail(WTP_EARG, -1, "a sweep takes 1 to %d thresholds", WTP_ABS_SWEEP_MAX_THR);
    if (ntensors == 0) return WTP_OK;
    const int n = ntensors;
    /* the outputs are outs': the plan reads shapes and inputs only (tensors[t].out is ignored) */
    std::vector<wtp_tensor> ts(tensors, tensors + n);
    for (auto& x : ts) x.out = const_cast<float*>(x.in);
    AbsPlan a;
    int rc = plan_abs(ts.data(), n, wavelet_id, level, true, a);
    if (rc != WTP_OK) return rc;
    bool any_live = false;
    for (int t = 0; t < n; ++t) any_live = any_live || a.ps[t].numel > 0;
    if (any_live && !outs) return fail(WTP_EARG, -1, "outs is NULL");
    for (int t = 0; t < n; ++t) {
        if (a.ps[t].numel == 0) continue;
        rc = check_sweep_outs(outs, nthr, n, t);
        if (rc != WTP_OK) return rc;
    }
    if (!ws || ws_bytes < a.total)
        return fail(WTP_EWORKSPACE, -1, "workspace too small: need %zu bytes, got %zu", a.total, ws_bytes);
    return abs_run(tensors, n, a, taps_for(wavelet_id), abs_thr(thresholds, nthr), outs, true, ws, results,
                   (hipStream_t)stream);
}

size_t wtp_dwt_workspace_size(int64_t B, int64_t H, int64_t W, int level) {
    if (level <= 0) return 0;
    wt_level_geom g;
    wt_geom(H, W, level, &g);
    const size_t a = (size_t)(B * g.R[1] * (W > 2 * g.C[1] ? W : 2 * g.C[1]));
    const size_t b = (size_t)(B * 2 * g.R[1] * 2 * g.C[1]);
    return 3 * align_up(std::max(a, b) * sizeof(float));
}

size_t wtp_dwt_workspace_size_mode(int64_t B, int64_t H, int64_t W, int wavelet_id, int level, int mode_id) {
    TPlan p;
    if (component_plan(B, H, W, wavelet_id, level, mode_id, p) != WTP_OK) return 0;
    return component_ws_bytes(p);
}

int wtp_wavedec2_f32(const float* in, float* packed, int64_t B, int64_t H, int64_t W, int wid, int level, void* ws,
                     size_t ws_bytes, wtp_stream_t stream) {
    return wavedec2_impl(in, packed, B, H, W, wid, level, WTP_MODE_PERIODIZATION, ws, ws_bytes, stream);
}
int wtp_wavedec2_mode_f32(const float* in, float* packed, int64_t B, int64_t H, int64_t W, int wid, int level,
                          int mode_id, void* ws, size_t ws_bytes, wtp_stream_t stream) {
    return wavedec2_impl(in, packed, B, H, W, wid, level, mode_id, ws, ws_bytes, stream);
}
int wtp_waverec2_f32(const float* packed, float* out, int64_t B, int64_t H, int64_t W, int wid, int level,
                     const float* thr32, void* ws, size_t ws_bytes, wtp_stream_t stream) {
    return waverec2_impl(packed, out, B, H, W, wid, level, WTP_MODE_PERIODIZATION, thr32, ws, ws_bytes, stream);
}
int wtp_waverec2_mode_f32(const float* packed, float* out, int64_t B, int64_t H, int64_t W, int wid, int level,
                          int mode_id, const float* thr32, void* ws, size_t ws_bytes, wtp_stream_t stream) {
    return waverec2_impl(packed, out, B, H, W, wid, level, mode_id, thr32, ws, ws_bytes, stream);
}

int wtp_synth_f32(float* out, int64_t n, uint64_t seed, uint32_t tensor_id, int e, wtp_stream_t stream) {
    if (n < 0 || (n > 0 && !out)) return fail(WTP_EARG, -1, "bad synth arguments");
    if (n == 0) return WTP_OK;
    launch_synth(out, n, seed, tensor_id, e, (hipStream_t)stream);
    return check_launch();
}

}  // extern "C"

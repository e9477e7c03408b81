/*
 * host_half.hip -- float16 weights (wtp_prune_f16): plan_tensors' plan of the list, then two kinds
 * of tensor.  Kind B (no transform) runs the float16 selection and mask of half.hip.  Kind A
 * (transformed) is widened into float32 staging, goes through wtp_prune_mode_f32 as a sub-list
 * with the staging as input and output, and is narrowed back with its zeros counted again.
 *
 * The sub-list is exact under WTP_CARRY_LEVEL: a tensor of ndim < 2 leaves the carried level alone,
 * and once a tensor of ndim >= 2 clamps it to 0 every later tensor is level 0 too, so the
 * transformed tensors meet the same running level in the sub-list as in the full list.
 * plan_half() checks that on every call instead of trusting it.
 *
 * Workspace: [the inner float32 call's workspace | top-digit histograms | low-digit histograms |
 * H16State per kind-B tensor | the inner call's records | float32 staging per kind-A tensor].
 * The part after the inner workspace is zeroed (the histograms and states) or overwritten by
 * every call.
 */
#include "wtp_half.h"
#include "wtp_host.h"

using namespace wtp;

namespace {

struct HalfPlan {
    std::vector<TPlan> ps;
    std::vector<int> a_idx, b_idx;  /* the kind-A / kind-B tensors, in list order */
    std::vector<wtp_tensor> sub;    /* the inner call's descriptors (pointers filled at run time) */
    std::vector<size_t> stage;      /* staging byte offset per kind-A tensor */
    size_t inner = 0, hist1 = 0, hist2 = 0, st = 0, zero_end = 0, subres = 0, total = 0;
};

int plan_half(const wtp_tensor* ts, int n, int wid, int level, double pct, int flags, int mode, bool check_ptrs,
              HalfPlan& hp) {
    int rc = mode_check(mode, flags);
    if (rc != WTP_OK) return rc;
    if (flags & WTP_FLATTEN) return fail(WTP_EARG, -1, "WTP_FLATTEN takes float32 tensors only");
    const bool carry = (flags & WTP_CARRY_LEVEL) != 0;
    if ((rc = plan_tensors(ts, n, wid, level, pct, check_ptrs, hp.ps, carry, false, mode)) != WTP_OK) return rc;
    for (int t = 0; t < n; ++t) {
        if (check_ptrs && ((reinterpret_cast<uintptr_t>(ts[t].in) | reinterpret_cast<uintptr_t>(ts[t].out)) & 1))
            return fail(WTP_EARG, t, "tensor %d: a float16 pointer is not 2-byte aligned", t);
        if (hp.ps[t].dwt) {
            hp.a_idx.push_back(t);
            wtp_tensor x = ts[t];
            x.in = nullptr;
            x.out = nullptr;
            hp.sub.push_back(x);
        } else {
            hp.b_idx.push_back(t);
        }
    }
    const size_t na = hp.a_idx.size(), nb = hp.b_idx.size();
    std::vector<TPlan> sps;
    if (na && plan_tensors(hp.sub.data(), (int)na, wid, level, pct, false, sps, carry, false, mode) != WTP_OK)
        return fail(WTP_EARG, -1, "internal: the transformed sub-list does not plan");
    for (size_t j = 0; j < na; ++j)
        if (sps[j].L != hp.ps[hp.a_idx[j]].L || !sps[j].dwt)
            return fail(WTP_EARG, hp.a_idx[j], "internal: tensor %d runs at level %d in the sub-list, %d in the list",
                        hp.a_idx[j], sps[j].L, hp.ps[hp.a_idx[j]].L);
    /* The inner call's layout, an empty sub-list's too: every layout begins with the float32
     * entries' persistent selection state, which a call of level-0 tensors only must leave alone
     * for the next call's transformed tensors (the scratch below starts past it in every call). */
    hp.inner = make_layout(sps, taps_for(wid)).total;
    size_t off = align_up(hp.inner);
    hp.hist1 = off;
    off = align_up(off + nb * H16_BINS1 * sizeof(uint32_t));
    hp.hist2 = off;
    off = align_up(off + nb * H16_NRANK * H16_BINS2 * sizeof(uint32_t));
    hp.st = off;
    off = align_up(off + nb * sizeof(H16State));
    hp.zero_end = off; /* k_h16_init zeroes [hist1, zero_end) */
    hp.subres = off;
    off = align_up(off + na * sizeof(wtp_result));
    hp.stage.resize(na);
    for (size_t j = 0; j < na; ++j) {
        hp.stage[j] = off;
        off = align_up(off + (size_t)hp.ps[hp.a_idx[j]].numel * sizeof(float));
    }
    hp.total = std::max(off, ALIGN);
    return WTP_OK;
}

/* tables of the tensors `idx` (H16_PER_LAUNCH each); the blocks follow h16_split of the input, or
 * of the output for the narrowing */
std::vector<H16Table> make_tables(const HalfPlan& hp, const std::vector<int>& idx, const wtp_tensor* ts, void* ws,
                                  double pct, bool kind_a, bool by_out) {
    std::vector<H16Table> tabs;
    for (size_t j = 0; j < idx.size(); ++j) {
        if (j % H16_PER_LAUNCH == 0) {
            tabs.emplace_back();
            memset(&tabs.back(), 0, sizeof(H16Table));
        }
        H16Table& tab = tabs.back();
        const int t = idx[j];
        const TPlan& p = hp.ps[t];
        H16Seg& sg = tab.s[tab.nseg];
        sg.in = reinterpret_cast<const uint16_t*>(ts[t].in);
        sg.out = reinterpret_cast<uint16_t*>(ts[t].out);
        sg.stage = kind_a ? wsb<float>(ws, hp.stage[j]) : nullptr;
        sg.n = p.numel;
        if (!kind_a) {
            SegDesc sd;
            memset(&sd, 0, sizeof sd);
            seg_ranks(p.numel, pct, sd);
            sg.r0 = sd.r0;
            sg.gamma = sd.gamma;
            sg.above = sd.above;
        }
        sg.res = t;
        sg.sub = (int32_t)j;
        sg.eff_level = p.L;
        const h16_span sp = h16_split(reinterpret_cast<uintptr_t>(by_out ? (const void*)sg.out : (const void*)sg.in), sg.n);
        tab.blk_begin[tab.nseg++] = tab.nblk;
        tab.nblk += (int32_t)std::max<int64_t>(1, (sp.nvec + H16_VPB - 1) / H16_VPB);
    }
    for (auto& tab : tabs)
        for (int i = tab.nseg; i < H16_PER_LAUNCH; ++i) tab.blk_begin[i] = INT32_MAX;
    return tabs;
}

}  // namespace

extern "C" {

size_t wtp_workspace_size_f16(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int flags,
                              int mode_id) {
    if (ntensors < 0 || (ntensors > 0 && !tensors)) return 0;
    HalfPlan hp;
    if (plan_half(tensors, ntensors, wavelet_id, level, 50.0, flags, mode_id, false, hp) != WTP_OK) return 0;
    return hp.total;
}

int wtp_prune_f16(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, int flags,
                  int mode_id, void* ws, size_t ws_bytes, wtp_result* results, wtp_stream_t stream) {
    clear_error();
    if (ntensors < 0 || (ntensors > 0 && (!tensors || !results))) return fail(WTP_EARG, -1, "bad arguments");
    HalfPlan hp;
    int rc = plan_half(tensors, ntensors, wavelet_id, level, pct, flags, mode_id, true, hp);
    if (rc != WTP_OK) return rc;
    if (ntensors == 0) return WTP_OK;
    if (!ws || ws_bytes < hp.total)
        return fail(WTP_EWORKSPACE, -1, "workspace too small: need %zu bytes, got %zu", hp.total, ws_bytes);
    const hipStream_t s = (hipStream_t)stream;
    const H16Ws w{wsb<uint32_t>(ws, hp.hist1), wsb<uint32_t>(ws, hp.hist2), wsb<H16State>(ws, hp.st)};
    launch_h16_init(w.hist1, (int64_t)((hp.zero_end - hp.hist1) / sizeof(uint32_t)), results, ntensors, s);

    /* kind B: the float16 selection and mask, five launches per table */
    for (const H16Table& tab : make_tables(hp, hp.b_idx, tensors, ws, pct, false, false)) {
        launch_h16_hist1(tab, w, s);
        launch_h16_scan1(tab, w, s);
        launch_h16_hist2(tab, w, s);
        launch_h16_scan2(tab, w, results, s);
        launch_h16_mask(tab, w, results, s);
    }
    if ((rc = check_launch()) != WTP_OK) return rc;

    /* kind A: widen, the float32 path on the staging, narrow */
    if (!hp.a_idx.empty()) {
        for (const H16Table& tab : make_tables(hp, hp.a_idx, tensors, ws, pct, true, false)) launch_h16_widen(tab, s);
        for (size_t j = 0; j < hp.sub.size(); ++j) hp.sub[j].in = hp.sub[j].out = wsb<float>(ws, hp.stage[j]);
        wtp_result* subres = wsb<wtp_result>(ws, hp.subres);
        rc = wtp_prune_mode_f32(hp.sub.data(), (int)hp.sub.size(), wavelet_id, level, pct,
                                flags & (WTP_CARRY_LEVEL | WTP_NO_RESIDENT), mode_id, ws, hp.inner, subres, stream);
        if (rc != WTP_OK) {
            if (g_err_tensor >= 0 && g_err_tensor < (int)hp.a_idx.size()) g_err_tensor = hp.a_idx[g_err_tensor];
            return rc;
        }
        for (const H16Table& tab : make_tables(hp, hp.a_idx, tensors, ws, pct, true, true))
            launch_h16_narrow(tab, subres, results, s);
    }
    return check_launch();
}

}  // extern "C"

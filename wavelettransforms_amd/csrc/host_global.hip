/*
 * host_global.hip -- the global percentile (wtp_prune_global_f32): plan_tensors' plan, one forward
 * transform per tensor of EVERY launch group, then one selection of every percentile's order
 * statistics over the pool of all populations (global.hip), then per percentile the level-0 mask
 * or the inverse transform with the pool's threshold.  Workspace: [one SwState | the pass-1
 * histogram | the pass-2 and pass-3 slot histograms | the pool's npct float64 and float32
 * thresholds | the mask launch's threshold table (npct x ntensors) | a packed array per
 * transformed tensor | three level temps per launch-group slot].
 */
#include "wtp_host.h"

using namespace wtp;

namespace {

struct GlobalPlan {
    std::vector<TPlan> ps;
    uint64_t pool = 0; /* keys in the pool */
    size_t st = 0, h1 = 0, h2 = 0, h3 = 0, zero_end = 0, thr64 = 0, thr = 0, thr_tab = 0, total = 0;
};

bool global_flags_ok(int flags) { return !(flags & ~(WTP_CARRY_LEVEL | WTP_SWEEP_THRESHOLDS_ONLY)); }
bool pct_bad(double p) { return !(p >= 0.0 && p <= 100.0); }

/* the plan of plan_tensors (validated with percentile `pct`), the pooled count and this entry's layout */
int plan_global(const wtp_tensor* ts, int n, int wid, int level, double pct, int npct, bool carry, GlobalPlan& gp) {
    const int rc = plan_tensors(ts, n, wid, level, pct, false, gp.ps, carry, false, WTP_MODE_PERIODIZATION);
    if (rc != WTP_OK) return rc;
    std::vector<int64_t> pops(n);
    for (int t = 0; t < n; ++t) pops[t] = gp.ps[t].pop;
    if (!gl_pool_count(pops.data(), n, &gp.pool))
        return fail(WTP_EARG, -1, "the pool of the %d tensors holds %llu keys: more than 2^32-1", n,
                    (unsigned long long)gp.pool);
    const Taps tp = taps_for(wid);
    size_t off = 0;
    gp.st = off;
    off = align_up(off + sizeof(SwState));
    gp.h1 = off;
    off = align_up(off + (size_t)SW_BINS1 * sizeof(uint32_t));
    gp.h2 = off;
    off = align_up(off + (size_t)SW_SLOT_WORDS * sizeof(uint32_t));
    gp.h3 = off;
    off = align_up(off + (size_t)SW_SLOT_WORDS * sizeof(uint32_t));
    gp.zero_end = off; /* k_sweep_init zeroes [st, zero_end) */
    gp.thr64 = off;
    off = align_up(off + (size_t)npct * sizeof(double));
    gp.thr = off;
    off = align_up(off + (size_t)npct * sizeof(float));
    gp.thr_tab = off;
    off = align_up(off + (size_t)npct * n * sizeof(float));
    for (auto& p : gp.ps) {
        if (!p.dwt) continue;
        p.p_off = off;
        off = align_up(off + (size_t)p.pop * sizeof(float));
    }
    /* level temps per launch-group slot: the groups' transforms run one after another on the stream */
    size_t slot_elems[SEG_PER_LAUNCH] = {};
    for (size_t t = 0; t < gp.ps.size(); ++t)
        if (gp.ps[t].dwt)
            slot_elems[t % SEG_PER_LAUNCH] = std::max(slot_elems[t % SEG_PER_LAUNCH], temp_elems(gp.ps[t], tp));
    size_t slot_off[SEG_PER_LAUNCH] = {};
    for (int j = 0; j < SEG_PER_LAUNCH; ++j) {
        if (!slot_elems[j]) continue;
        slot_off[j] = off;
        off = align_up(off + 3 * align_up(slot_elems[j] * sizeof(float)));
    }
    for (size_t t = 0; t < gp.ps.size(); ++t) {
        if (!gp.ps[t].dwt) continue;
        gp.ps[t].t_off = slot_off[t % SEG_PER_LAUNCH];
        gp.ps[t].t_elems = slot_elems[t % SEG_PER_LAUNCH];
    }
    gp.total = off;
    return WTP_OK;
}

}  // namespace

extern "C" {

size_t wtp_global_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int npct,
                                 int flags) {
    if (ntensors < 0 || (ntensors > 0 && !tensors) || !global_flags_ok(flags) || npct < 1 || npct > WTP_SWEEP_MAX_PCT)
        return 0;
    GlobalPlan gp;
    if (plan_global(tensors, ntensors, wavelet_id, level, 50.0, npct, (flags & WTP_CARRY_LEVEL) != 0, gp) != WTP_OK)
        return 0;
    return gp.total;
}

int wtp_prune_global_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, const double* pcts,
                         int npct, int flags, float* const* outs, void* ws, size_t ws_bytes, wtp_result* results,
                         wtp_stream_t stream) {
    clear_error();
    if (ntensors < 0 || (ntensors > 0 && (!tensors || !results))) return fail(WTP_EARG, -1, "bad arguments");
    if (!global_flags_ok(flags)) return fail(WTP_EARG, -1, "bad flags 0x%x", flags);
    if (npct < 1 || npct > WTP_SWEEP_MAX_PCT || !pcts)
        return fail(WTP_EARG, -1, "a global call takes 1 to %d percentiles", WTP_SWEEP_MAX_PCT);
    const bool thr_only = (flags & WTP_SWEEP_THRESHOLDS_ONLY) != 0;
    const int n = ntensors;
    /* a bad percentile among good ones: plan_tensors reports it where the reference would */
    double vpct = pcts[0];
    for (int k = npct - 1; k >= 0; --k)
        if (pct_bad(pcts[k])) vpct = pcts[k];
    if (n == 0) return pct_bad(vpct) ? fail(WTP_EBADPCT, -1, "Percentiles must be in the range [0, 100]") : WTP_OK;
    GlobalPlan gp;
    int rc = plan_global(tensors, n, wavelet_id, level, vpct, npct, (flags & WTP_CARRY_LEVEL) != 0, gp);
    if (rc != WTP_OK) return rc;
    if (!thr_only && !outs) return fail(WTP_EARG, -1, "outs is NULL without WTP_SWEEP_THRESHOLDS_ONLY");
    for (int t = 0; t < n; ++t) {
        if (!tensors[t].in) return fail(WTP_EARG, t, "tensor %d: null pointer", t);
        if (thr_only) continue;
        rc = check_sweep_outs(outs, npct, n, t);
        if (rc != WTP_OK) return rc;
    }
    if (!ws || ws_bytes < gp.total)
        return fail(WTP_EWORKSPACE, -1, "workspace too small: need %zu bytes, got %zu", gp.total, ws_bytes);

    const hipStream_t s = (hipStream_t)stream;
    const Taps tp = taps_for(wavelet_id);
    const GlWs w{wsb<SwState>(ws, gp.st), wsb<uint32_t>(ws, gp.h1),  wsb<uint32_t>(ws, gp.h2), wsb<uint32_t>(ws, gp.h3),
                 wsb<float>(ws, gp.thr),  wsb<double>(ws, gp.thr64), wsb<float>(ws, gp.thr_tab)};
    /* the state and histograms every pass launch adds into: zeroed by a kernel, as in the sweep */
    launch_sweep_init(wsb<uint32_t>(ws, gp.st), (int64_t)((gp.zero_end - gp.st) / sizeof(uint32_t)), s);

    const int ngroups = (n + SEG_PER_LAUNCH - 1) / SEG_PER_LAUNCH;
    /* 1. the pool: pywt.wavedec2 + coeffs_to_array of the transformed tensors of EVERY group first */
    std::vector<char> has_dwt(ngroups, 0);
    for (int gi = 0; gi < ngroups; ++gi) {
        const int g0 = gi * SEG_PER_LAUNCH, g1 = std::min(n, g0 + SEG_PER_LAUNCH);
        std::vector<Chain> fwd;
        for (int t = g0; t < g1; ++t) {
            const TPlan& p = gp.ps[t];
            if (!p.dwt) continue;
            float* P = wsb<float>(ws, p.p_off);
            if (!p.tight) launch_abs_zero(P, p.pop, s);
            fwd.push_back(make_chain(p, tensors[t].in, nullptr, P, wsb(ws, p.t_off), align_up(p.t_elems * sizeof(float)),
                                     nullptr, nullptr));
        }
        has_dwt[gi] = !fwd.empty();
        if (!fwd.empty()) forward_chains(fwd, tp, s);
    }
    /* 2. the selection: per pass one launch per group into the pool's histograms, then ONE scan;
     * the ranks are those of the pooled count */
    GlRanks rk;
    memset(&rk, 0, sizeof rk);
    rk.npct = npct;
    for (int k = 0; k < npct; ++k) {
        SegDesc sd;
        memset(&sd, 0, sizeof sd);
        seg_ranks((int64_t)gp.pool, pcts[k], sd);
        rk.r0[k] = (uint32_t)sd.r0;
        rk.gamma[k] = sd.gamma;
        if (sd.above) rk.above |= 1u << k;
    }
    std::vector<GlTable> tabs(ngroups);
    for (int gi = 0; gi < ngroups; ++gi) {
        const int g0 = gi * SEG_PER_LAUNCH, g1 = std::min(n, g0 + SEG_PER_LAUNCH);
        GlTable& tab = tabs[gi];
        memset(&tab, 0, sizeof tab);
        int64_t chunks = 0;
        for (int t = g0; t < g1; ++t) chunks += (gp.ps[t].pop + SW_CHUNK - 1) / SW_CHUNK;
        tab.cpb = (int32_t)std::max<int64_t>(1, (chunks + SW_MAX_BLOCKS - 1) / SW_MAX_BLOCKS);
        for (int t = g0; t < g1; ++t) {
            const TPlan& p = gp.ps[t];
            GlSeg& sg = tab.s[tab.nseg];
            sg.data = p.dwt ? wsb<const float>(ws, p.p_off) : tensors[t].in;
            sg.n = p.pop;
            tab.blk_begin[tab.nseg++] = tab.nblk;
            const int64_t nch = (p.pop + SW_CHUNK - 1) / SW_CHUNK;
            tab.nblk += (int32_t)((nch + tab.cpb - 1) / tab.cpb);
        }
        for (int i = tab.nseg; i < SEG_PER_LAUNCH; ++i) tab.blk_begin[i] = INT32_MAX;
    }
    for (int pass = 1; pass <= 3; ++pass) {
        for (int gi = 0; gi < ngroups; ++gi) launch_global_pass(tabs[gi], pass, w, s);
        launch_global_scan(rk, pass, w, s);
    }
    /* the records, and the thresholds laid out as k_sweep_mask reads them */
    for (int gi = 0; gi < ngroups; ++gi) {
        const int g0 = gi * SEG_PER_LAUNCH, g1 = std::min(n, g0 + SEG_PER_LAUNCH);
        GlRecTable rt;
        memset(&rt, 0, sizeof rt);
        rt.t0 = g0;
        rt.ntensors = n;
        rt.npct = npct;
        for (int t = g0; t < g1; ++t) {
            const TPlan& p = gp.ps[t];
            GlRecSeg& sg = rt.s[rt.nseg++];
            sg.numel = p.numel;
            sg.coeff_numel = p.pop;
            sg.eff_level = p.L;
        }
        launch_global_records(rt, w, results, s);
    }
    if (thr_only) return check_launch();
    /* 3. the outputs, group by group: level-0 and ndim < 2 tensors in one mask launch for all
     * percentiles (sweep.hip's k_sweep_mask over thr_tab) ... */
    for (int gi = 0; gi < ngroups; ++gi) {
        const int g0 = gi * SEG_PER_LAUNCH, g1 = std::min(n, g0 + SEG_PER_LAUNCH);
        SwMaskTable mt;
        memset(&mt, 0, sizeof mt);
        mt.npct = npct;
        mt.ntensors = n;
        for (int t = g0; t < g1; ++t) {
            const TPlan& p = gp.ps[t];
            if (p.dwt) continue;
            SwMaskSeg& mg = mt.s[mt.nseg];
            mg.data = tensors[t].in;
            mg.n = p.numel;
            mg.t = t;
            uintptr_t bits = reinterpret_cast<uintptr_t>(tensors[t].in);
            for (int k = 0; k < npct; ++k) {
                mg.out[k] = outs[(size_t)k * n + t];
                bits |= reinterpret_cast<uintptr_t>(mg.out[k]);
            }
            mg.aligned = (bits & 15) == 0;
            mt.blk_begin[mt.nseg++] = mt.nblk;
            mt.nblk += (int32_t)((p.numel + SW_CHUNK - 1) / SW_CHUNK);
        }
        for (int i = mt.nseg; i < SEG_PER_LAUNCH; ++i) mt.blk_begin[i] = INT32_MAX;
        if (mt.nseg) launch_sweep_mask(mt, w.thr_tab, results, s);
        /* ... the others by waverec2 of the same packed array, once per percentile, with the
         * pool's threshold word of that percentile and the record's zero counter */
        if (!has_dwt[gi]) continue;
        for (int k = 0; k < npct; ++k) {
            std::vector<Chain> inv;
            for (int t = g0; t < g1; ++t) {
                const TPlan& p = gp.ps[t];
                if (!p.dwt) continue;
                const size_t ri = gl_record_index(k, n, t);
                inv.push_back(make_chain(p, tensors[t].in, outs[ri], wsb<float>(ws, p.p_off), wsb(ws, p.t_off),
                                         align_up(p.t_elems * sizeof(float)), w.thr + k,
                                         reinterpret_cast<unsigned long long*>(&results[ri].zero_count)));
            }
            inverse_chains(inv, tp, s);
        }
    }
    return check_launch();
}

}  // extern "C"

/*
 * host_prune.hip -- the percentile path: one multi_resolution_analysis call (ResNet/dwt_pruning.py:
 * 35-95) as plan, layout, the one-launch small path, then per launch group forward, selection and
 * inverse, with the selection on a side stream when the call has several groups.  Also the
 * entries of that path, their workspace queries and the process-wide switches prune_impl reads.
 */
#include <atomic>
#include <map>
#include <mutex>

#include "wtp_host.h"
#include "small_geom.h"

using namespace wtp;

static thread_local hipEvent_t g_stage_ev[8];
static thread_local int g_stage_n = 0;
static std::atomic<int> g_resident{1}; /* wtp_set_resident */
static std::atomic<int> g_pipeline{1}; /* wtp_set_pipeline */
static std::atomic<int> g_fused{1};    /* wtp_set_fused_select */

static inline void stage(int i, hipStream_t s) {
    if (i < g_stage_n && g_stage_ev[i]) (void)hipEventRecord(g_stage_ev[i], s);
}

/* ---- the one-launch small path (small.hip) ---- */
constexpr int64_t SM_POP_MAX = 1 << 20; /* population of a whole call taken by k_small */
constexpr int SM_TILES_MAX = SM_SEG_WG_MAX; /* workgroups per tensor */
constexpr int64_t SM_TILE_COST = 64;         /* tiling choice: LDS words a workgroup is worth */

/* Tile sizes (TR x TC at level L) for one tensor: every tile's forward and inverse arena must
 * fit; among those, the least per-workgroup level-0 window plus a charge per workgroup. */
static bool small_tiling(const TPlan& p, int F, int budget, int words, SmallSeg& sg) {
    const int L = p.L;
    int32_t Rn[SM_LMAX + 1], Cn[SM_LMAX + 1];
    for (int k = 0; k <= L; ++k) { Rn[k] = (int32_t)p.g.R[k]; Cn[k] = (int32_t)p.g.C[k]; }
    const int RL = Rn[L], CL = Cn[L];
    int64_t best = INT64_MAX;
    std::vector<SmAxis> ar, ac;
    for (int TR = RL;; TR = (TR + 1) / 2) {
        const int tR = (RL + TR - 1) / TR;
        ar.resize(tR);
        for (int i = 0; i < tR; ++i) sm_axis(i, TR, L, Rn, F, &ar[i]);
        for (int TC = CL;; TC = (TC + 1) / 2) {
            const int tC = (CL + TC - 1) / TC;
            const int64_t tiles = p.B * tR * tC;
            if (tiles <= budget && 2 * (L + 1) * (tR + tC) <= words) {
                ac.resize(tC);
                for (int j = 0; j < tC; ++j) sm_axis(j, TC, L, Cn, F, &ac[j]);
                int64_t worst = 0;
                bool fits = true;
                for (int i = 0; i < tR && fits; ++i)
                    for (int j = 0; j < tC && fits; ++j) {
                        const SmNeed nd = sm_need(ar[i], ac[j], L, F);
                        fits = sm_fwd_words(nd) <= SM_ARENA && sm_inv_words(nd) <= SM_ARENA;
                        worst = std::max<int64_t>(worst, (int64_t)ar[i].fw[0].len * ac[j].fw[0].len + nd.fkeys / 2);
                    }
                const int64_t cost = worst + SM_TILE_COST * tiles;
                if (fits && cost < best) {
                    best = cost;
                    sg.TR = TR;
                    sg.TC = TC;
                    sg.tilesR = tR;
                    sg.tilesC = tC;
                }
            }
            if (TC == 1) break;
        }
        if (TR == 1) break;
    }
    return best != INT64_MAX;
}

/* k_small takes the whole call when every tensor is a 2-D transform, the call is small and
 * every tensor finds a tiling inside the co-resident grid */
static bool plan_small(const std::vector<TPlan>& ps, const wtp_tensor* ts, int n, void* ws, double pct, const Taps& tp,
                       uint32_t* slots, SmallTable& t) {
    if (n > SM_MAX_SEG || (tp.F & 1) || tp.F < 2 || tp.F > SM_F_MAX) return false;
    const int cap = std::min(small_capacity(), RES_MAX_WG);
    int64_t tot = 0;
    for (const TPlan& p : ps) {
        if (!p.dwt || p.flat || p.mode || p.L > SM_LMAX || p.H > SM_LINE_MAX || p.W > SM_LINE_MAX) return false;
        tot += p.pop;
    }
    if (tot > SM_POP_MAX || cap < n) return false;
    memset(&t, 0, sizeof t);
    int wg = 0, words = 0;
    for (int i = 0; i < n; ++i) {
        const TPlan& p = ps[i];
        SmallSeg& sg = t.s[i];
        /* workgroups by share of the population, at least one per image */
        if (p.B > SM_SEG_WG_MAX) return false;
        const int budget = (int)std::max<int64_t>(p.B, std::min<int64_t>(std::min(SM_TILES_MAX, SM_SEG_WG_MAX),
                                                                         (int64_t)cap * p.pop / tot));
        if (!small_tiling(p, tp.F, budget, (SM_WIN_WORDS - words) / (n - i), sg)) return false;
        /* the windows of every tile row and tile column, packed (small_geom.h computes them) */
        {
            int32_t Rn[SM_LMAX + 1], Cn[SM_LMAX + 1];
            for (int k = 0; k <= p.L; ++k) { Rn[k] = (int32_t)p.g.R[k]; Cn[k] = (int32_t)p.g.C[k]; }
            sg.win_off = words;
            auto pack = [&](const SmAxis& a) {
                for (int k = 0; k <= p.L; ++k) {
                    t.win[words++] = (uint32_t)a.fw[k].s | ((uint32_t)a.fw[k].len << 16);
                    t.win[words++] = (uint32_t)a.sv[k].s | ((uint32_t)a.sv[k].len << 16);
                }
            };
            SmAxis a;
            for (int r = 0; r < sg.tilesR; ++r) { sm_axis(r, sg.TR, p.L, Rn, tp.F, &a); pack(a); }
            for (int c = 0; c < sg.tilesC; ++c) { sm_axis(c, sg.TC, p.L, Cn, tp.F, &a); pack(a); }
        }
        sg.in = ts[i].in;
        sg.out = ts[i].out;
        sg.P = wsb<float>(ws, p.p_off);
        SegDesc sd;
        memset(&sd, 0, sizeof sd);
        seg_ranks(p.pop, pct, sd);
        sg.r0 = sd.r0;
        sg.gamma = sd.gamma;
        sg.above = sd.above;
        sg.numel = p.numel;
        sg.n = p.pop;
        sg.B = (int32_t)p.B;
        sg.L = p.L;
        sg.PR = (int32_t)p.g.PR;
        sg.PC = (int32_t)p.g.PC;
        for (int k = 0; k <= p.L; ++k) {
            sg.R[k] = (int32_t)p.g.R[k];
            sg.C[k] = (int32_t)p.g.C[k];
            sg.offR[k] = k ? (int32_t)p.g.offR[k] : 0;
            sg.offC[k] = k ? (int32_t)p.g.offC[k] : 0;
        }
        sg.npad = (int32_t)(p.pop - p.B * wtm_block_cells(&p.g, p.L));
        sg.res = i;
        sg.wg_begin = wg;
        sg.nwg = (int32_t)(p.B * sg.tilesR * sg.tilesC);
        t.wg_begin[i] = wg;
        wg += sg.nwg;
    }
    for (int i = n; i < SM_MAX_SEG; ++i) t.wg_begin[i] = INT32_MAX;
    if (wg > cap) return false;
    t.nseg = n;
    t.slots = slots;
    t.nblk = wg;
    t.tp.F = tp.F;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < SM_F_MAX; ++j) t.tp.f[i][j] = j < tp.F ? tp.f[i][j] : 0.0f;
    return true;
}

/* ---- the selection pipeline ----
 * The side stream (one per device and caller stream, non-blocking, created on first use and kept)
 * and its events: a call with several launch groups of DWT segments runs group g's forward levels
 * on the caller's stream and its selection (window / collect / mask-select: HBM-bound) on the side
 * stream, so it overlaps the next group's forward levels or the previous group's inverse levels
 * (VALU-bound); the caller's stream waits for every group's selection before that group's inverse,
 * which joins the side stream back (graph capture included).  Selections stay serialised on the
 * side stream (the SelHeader parity regions). */
struct SidePipe {
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev;
};
static std::mutex g_pipe_mu;
static std::map<std::pair<int, hipStream_t>, SidePipe> g_pipes;
static SidePipe* side_pipe(hipStream_t s, int nev) {
    /* the side stream must live on the caller's stream's device: when that is not the current
     * device (the caller set no device guard) the call keeps the single-stream form */
    int dev = 0, sdev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (hipStreamGetDevice(s, &sdev) != hipSuccess || sdev != dev) return nullptr;
    std::lock_guard<std::mutex> lk(g_pipe_mu);
    SidePipe& sp = g_pipes[{dev, s}];
    if (!sp.side && hipStreamCreateWithFlags(&sp.side, hipStreamNonBlocking) != hipSuccess) {
        sp.side = nullptr;
        return nullptr;
    }
    while ((int)sp.ev.size() < nev) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        sp.ev.push_back(e);
    }
    return &sp;
}

struct PruneOpts { /* the flags of the call, parsed once */
    bool carry, flat, no_resident;
    int mode;
};

/* One call of the percentile path: what its steps share. */
struct PruneCall {
    const wtp_tensor* ts;
    int n;
    double pct;
    void* ws;
    wtp_result* results;
    PruneOpts opt;
    Taps tp;
    std::vector<TPlan> ps;
    Layout lay;
    SelHeader* head;
    uint32_t* cand;
    float* thr_t;
    int ngroups;
    std::vector<std::vector<Chain>> gchains; /* per launch group: its 2-D transform chains */
    std::vector<char> fused;                 /* per launch group: fused selection */
    std::vector<FwinTable> fts;              /* ... and its window pass's table */
    hipStream_t s;                           /* the caller's stream */
    hipStream_t ss;                          /* the selection's stream: the side stream, or s */
    SidePipe* pipe = nullptr;                /* null: the single-stream form */
    bool forked = false;
};
static int group_begin(const PruneCall& c, int gi) { return gi * SEG_PER_LAUNCH; }
static int group_end(const PruneCall& c, int gi) { return std::min(c.n, (gi + 1) * SEG_PER_LAUNCH); }

/* the side pipe's events, by what they mark (3 ngroups + 2 of them) */
static int pipe_events(int ngroups) { return 3 * ngroups + 2; }
static hipEvent_t ev_forward_done(const PruneCall& c, int gi) { return c.pipe->ev[2 * gi]; }
static hipEvent_t ev_selection_done(const PruneCall& c, int gi) { return c.pipe->ev[2 * gi + 1]; }
static hipEvent_t ev_window_done(const PruneCall& c, int gi) { return c.pipe->ev[2 * c.ngroups + gi]; } /* fused group's k_fwin */
static hipEvent_t ev_call_start(const PruneCall& c) { return c.pipe->ev[3 * c.ngroups]; } /* on the caller's stream */
static hipEvent_t ev_join(const PruneCall& c) { return c.pipe->ev[3 * c.ngroups + 1]; }
/* an error after the first fork still joins the side stream back into the caller's (an unjoined
 * fork invalidates a capture, and eagerly the caller may free what it still reads) */
static int fail_joined(const PruneCall& c, int t, const char* msg) {
    if (c.forked) {
        (void)hipEventRecord(ev_join(c), c.ss);
        (void)hipStreamWaitEvent(c.s, ev_join(c), 0);
    }
    return fail(WTP_EHIP, t, "%s", msg);
}

/* The chains of group gi's 2-D transforms, with the packed arrays' padding zeroed; a flattened
 * tensor's forward runs here, in the tensors' order. */
static int build_group_chains(PruneCall& c, int gi) {
    for (int t = group_begin(c, gi); t < group_end(c, gi); ++t) {
        const TPlan& p = c.ps[t];
        if (!p.dwt) continue;
        const size_t stride = align_up(p.t_elems * sizeof(float));
        if (p.flat) {
            forward_flat(p, c.ts[t].in, wsb<float>(c.ws, p.p_off), wsb<float>(c.ws, p.t_off),
                         wsb<float>(c.ws, p.t_off + stride), c.tp, c.s);
            continue;
        }
        Chain ch = make_chain(p, c.ts[t].in, c.ts[t].out, wsb<float>(c.ws, p.p_off), wsb(c.ws, p.t_off), stride,
                              c.thr_t + t, reinterpret_cast<unsigned long long*>(&c.results[t].zero_count));
        if (p.f_slots) ch.fsl = wsb<uint32_t>(c.ws, p.f_off);
        c.gchains[gi].push_back(ch);
        if (p.mode) { /* the padding zeros by a kernel (a memset node misbehaved in a replayed graph:
                       * k_abs_init's note); k_mtiny_fwd writes whole packed images itself */
            if (!p.tight && p.tiny_lg < 0) launch_abs_zero(ch.P, p.pop, c.s);
        } else if (!p.tight && hipMemsetAsync(ch.P, 0, (size_t)p.pop * sizeof(float), c.s) != hipSuccess)
            return fail(WTP_EHIP, t, "hipMemsetAsync failed");
    }
    return WTP_OK;
}

/* fused selection per launch group: every tensor of the group qualifies with its real input
 * pointer and the current interior mode (fused_slot_count) */
static bool group_fused(const PruneCall& c, int gi) {
    for (int t = group_begin(c, gi); t < group_end(c, gi); ++t)
        if (!(c.ps[t].f_slots > 0 && fused_slot_count(c.ps[t], c.ts[t].in, c.tp, false) == c.ps[t].f_slots)) return false;
    return true;
}

/* a fused group's window pass (k_fwin): its table */
static void build_fwin_table(const PruneCall& c, int gi, FwinTable& ft) {
    memset(&ft, 0, sizeof ft);
    const int g0 = group_begin(c, gi), g1 = group_end(c, gi);
    ft.nseg = g1 - g0;
    ft.F = c.tp.F;
    ft.gh = wsb<uint32_t>(c.ws, c.lay.fwh);
    for (int j = 0; j < c.tp.F && j < FWIN_F_MAX; ++j) { ft.lo[j] = c.tp.f[0][j]; ft.hi[j] = c.tp.f[1][j]; }
    for (int t = g0; t < g1; ++t) {
        const TPlan& p = c.ps[t];
        FwinSeg& f = ft.s[t - g0];
        SegDesc sd;
        memset(&sd, 0, sizeof sd);
        seg_ranks(p.pop, c.pct, sd);
        bucket_plan(p.pop, &sd.nsub_log2, &sd.bucket_cap, true);
        f.in = c.ts[t].in;
        f.hdr = wsb<FslHeader>(c.ws, p.f_off);
        f.n = p.pop;
        f.r0 = sd.r0;
        f.above = sd.above;
        f.nsub_log2 = sd.nsub_log2;
        f.B = (int32_t)p.B;
        f.R = (int32_t)p.g.R[0];
        f.C = (int32_t)p.g.C[0];
        f.L = p.L;
    }
}

/* pipelined: fused group gi's window pass on the side stream (a group past the last, or one that is
 * not fused: nothing) */
static bool window_on_side(const PruneCall& c, int gi) {
    if (gi >= c.ngroups || !c.fused[gi]) return true;
    launch_fwin(c.fts[gi], c.head, c.ss);
    return hipEventRecord(ev_window_done(c, gi), c.ss) == hipSuccess;
}

/* one resident launch when every segment of the group is level-0 and the group's chunks fit the
 * co-resident grid; *rblk: the group's workgroups in that form */
static bool group_resident(const PruneCall& c, int gi, int64_t* rblk) {
    bool all0 = true;
    *rblk = 0;
    for (int t = group_begin(c, gi); t < group_end(c, gi); ++t) {
        all0 = all0 && !c.ps[t].dwt;
        *rblk += (c.ps[t].pop + RES_CHUNK - 1) / RES_CHUNK;
    }
    return !c.fused[gi] && all0 && !c.opt.no_resident && g_resident.load(std::memory_order_relaxed) &&
           *rblk <= RES_MAX_WG && *rblk <= resident_capacity();
}

/* the resident launch's late group: the smallest segments, together at most RES_LATE_PCT % of
 * the workgroups (at least one segment stays early) */
static void choose_late(const PruneCall& c, int gi, int64_t rblk, bool late[SEG_PER_LAUNCH]) {
    const int g0 = group_begin(c, gi), ng = group_end(c, gi) - g0;
    int by[SEG_PER_LAUNCH];
    for (int i = 0; i < ng; ++i) by[i] = g0 + i;
    std::stable_sort(by, by + ng, [&](int a, int b) { return c.ps[a].pop < c.ps[b].pop; });
    int64_t lb = 0;
    for (int i = 0; i + 1 < ng; ++i) {
        const int64_t w = (c.ps[by[i]].pop + RES_CHUNK - 1) / RES_CHUNK;
        if (100 * (lb + w) > (int64_t)RES_LATE_PCT * rblk) break;
        lb += w;
        late[by[i] - g0] = true;
    }
}

/* group gi's segment table, in the block units of the form that selects it */
static void build_seg_table(const PruneCall& c, int gi, bool resident, int64_t rblk, SegTable& tab) {
    memset(&tab, 0, sizeof tab);
    const bool fz = c.fused[gi] != 0;
    const int64_t chunk = resident ? RES_CHUNK : CHUNK;
    bool late[SEG_PER_LAUNCH] = {};
    if (resident) choose_late(c, gi, rblk, late);
    const int g0 = group_begin(c, gi);
    for (int t = g0; t < group_end(c, gi); ++t) {
        const TPlan& p = c.ps[t];
        /* k_fslot_collect: one block per FSC_SLOTS wave slots (seg_fsl / seg_fsl_n) */
        const int nblk = fz ? (int)((p.f_slots + FSC_SLOTS - 1) / FSC_SLOTS) : (int)((p.pop + chunk - 1) / chunk);
        SegDesc& sd = seg_add(tab, p, p.dwt ? wsb<const float>(c.ws, p.p_off) : c.ts[t].in, p.dwt ? nullptr : c.ts[t].out,
                              t, p.dwt ? 0 : SEG_MASK, nblk);
        seg_ranks(p.pop, c.pct, sd);
        if (resident) {
            sd.nsub_log2 = RES_NSUB_LOG2;
            if (p.pop > RES_MS) /* rounded up: floor(g * step_fx / 2^32) is then the exact floor of
                                   * g (n - 16) / 255 for every group g <= 255 (the error stays
                                   * below 255 / 2^32, under the 1/255 gap to the next integer) */
                sd.res_step_fx = (((uint64_t)(p.pop - SAMPLE_GROUP) << 32) + (uint64_t)(RES_MS / SAMPLE_GROUP - 2)) /
                                 (uint64_t)(RES_MS / SAMPLE_GROUP - 1);
        }
        if (late[t - g0]) sd.flags |= SEG_LATE;
        if (fz) {
            sd.out = wsb<float>(c.ws, p.f_off);
            sd.res_step_fx = (uint64_t)p.f_slots;
            sd.flags |= SEG_FUSED;
        }
    }
    seg_close(tab);
}

/* Ahead of group gi's selection: pipelined, its forward levels on the caller's stream and the
 * selection's stream behind them; else a fused group's window pass and forward (the other groups'
 * forwards already ran). */
static int forward_before_select(PruneCall& c, int gi) {
    const bool fz = c.fused[gi] != 0;
    if (c.pipe) {
        if (fz && hipStreamWaitEvent(c.s, ev_window_done(c, gi), 0) != hipSuccess)
            return fail_joined(c, -1, "hipStreamWaitEvent failed");
        forward_chains(c.gchains[gi], c.tp, c.s, fz);
        if (hipEventRecord(ev_forward_done(c, gi), c.s) != hipSuccess) return fail_joined(c, -1, "hipEventRecord failed");
        if (hipStreamWaitEvent(c.ss, ev_forward_done(c, gi), 0) != hipSuccess)
            return fail_joined(c, -1, "hipStreamWaitEvent failed");
        c.forked = true;
    } else if (fz) {
        launch_fwin(c.fts[gi], c.head, c.s);
        forward_chains(c.gchains[gi], c.tp, c.s, true);
    }
    return WTP_OK;
}

/* the fused form: the bucket pass over the forward's wave slots, the select, and the retry */
static int select_fused(PruneCall& c, int gi, const SegTable& tab, bool first) {
    if (first) { stage(1, c.ss); stage(2, c.ss); }
    launch_fslot_collect(tab, c.head, c.cand, c.results, c.ss);
    /* group g + 2's window pass next on the side stream: it needs only the slot areas this
     * bucket pass has read, not this group's select and retry */
    if (c.pipe && !window_on_side(c, gi + 2)) return fail_joined(c, -1, "hipEventRecord failed");
    if (first) stage(3, c.ss);
    launch_mask_select(tab, c.head, c.cand, c.results, c.thr_t, c.ss);
    /* a segment whose patch window missed the ranks: the unfused window / collect / select
     * over P, for it alone (the same table in k_collect's chunk units) */
    SegTable rt = tab;
    rt.retry = 1;
    int rb = 0;
    for (int i = 0; i < rt.nseg; ++i) {
        SegDesc& sd = rt.s[i];
        sd.flags &= ~SEG_FUSED;
        sd.out = nullptr;
        sd.res_step_fx = 0;
        sd.blk_begin = rt.blk_begin[i] = rb;
        rb += (int)((sd.n + CHUNK - 1) / CHUNK);
    }
    rt.nblk = rb;
    launch_fused_retry(rt, c.head, c.cand, c.results, c.thr_t, c.ss);
    return WTP_OK;
}

static void select_resident(PruneCall& c, const SegTable& tab, bool first) {
    if (first) stage(1, c.ss);
    if (first) { stage(2, c.ss); stage(3, c.ss); }
    launch_resident(tab, c.head, c.cand, c.results, c.thr_t, c.ss);
}

/* the three-launch form, and the in-place level-0 segments whose select took the full scan */
static void select_three(PruneCall& c, const SegTable& tab, bool first) {
    if (first) stage(1, c.ss);
    launch_window(tab, c.head, c.ss);
    if (first) stage(2, c.ss);
    launch_collect(tab, c.head, c.cand, c.results, c.ss);
    if (first) stage(3, c.ss);
    launch_mask_select(tab, c.head, c.cand, c.results, c.thr_t, c.ss);
    bool inplace = false;
    for (int i = 0; i < tab.nseg; ++i) inplace = inplace || (tab.s[i].out && tab.s[i].out == tab.s[i].data);
    if (inplace) launch_mask_inplace(tab, c.results, c.thr_t, c.ss);
}

/* exact percentile selection + level-0 mask of launch group gi */
static int select_group(PruneCall& c, int gi) {
    const bool fz = c.fused[gi] != 0, first = gi == 0;
    int64_t rblk = 0;
    const bool resident = group_resident(c, gi, &rblk);
    SegTable tab;
    build_seg_table(c, gi, resident, rblk, tab);
    int rc = forward_before_select(c, gi);
    if (rc != WTP_OK) return rc;
    if (fz) {
        if ((rc = select_fused(c, gi, tab, first)) != WTP_OK) return rc;
    } else if (resident) {
        select_resident(c, tab, first);
    } else {
        select_three(c, tab, first);
    }
    if (first) stage(4, c.ss);
    if (c.pipe && hipEventRecord(ev_selection_done(c, gi), c.ss) != hipSuccess) return fail_joined(c, -1, "hipEventRecord failed");
    if (c.pipe && !fz && !window_on_side(c, gi + 2)) return fail_joined(c, -1, "hipEventRecord failed");
    return WTP_OK;
}

/* inverse transforms of group gi with the threshold applied on load (array_to_coeffs + waverec2);
 * pipelined, behind the group's selection (which joins the side stream) */
static int inverse_group(PruneCall& c, int gi) {
    if (c.pipe && hipStreamWaitEvent(c.s, ev_selection_done(c, gi), 0) != hipSuccess)
        return fail_joined(c, -1, "hipStreamWaitEvent failed");
    inverse_chains(c.gchains[gi], c.tp, c.s);
    return WTP_OK;
}

/* Step 1 of the call: every group's chains; which groups select fused; the side pipe; then the
 * forwards that do not wait for a selection step -- single stream: every group that is not fused,
 * group by group (the groups share the level temps, make_layout); pipelined: none yet, only the
 * first two fused groups' window passes on the side stream.  The rest runs in select_group(). */
static int forward_groups(PruneCall& c) {
    const hipStream_t s = c.s;
    int rc;
    const int ngroups = c.ngroups = (c.n + SEG_PER_LAUNCH - 1) / SEG_PER_LAUNCH;
    c.gchains.resize(ngroups);
    for (int gi = 0; gi < ngroups; ++gi)
        if ((rc = build_group_chains(c, gi)) != WTP_OK) return rc;
    int dwt_groups = 0;
    for (const auto& gc : c.gchains) dwt_groups += !gc.empty();
    c.fused.assign(ngroups, 0);
    bool any_fused = false;
    if (g_fused.load(std::memory_order_relaxed))
        for (int gi = 0; gi < ngroups; ++gi) any_fused = (c.fused[gi] = group_fused(c, gi)) || any_fused;
    /* (Round 5's mode 2 -- each group's levels on a lane stream of its own -- measured slower and
     * was removed in round 6; its capture-crash bisection is kept in tools/lanes_capture_diag.py
     * and DESIGN.md.) */
    const int pmode = dwt_groups > 1 ? g_pipeline.load(std::memory_order_relaxed) : 0;
    c.pipe = pmode ? side_pipe(s, pipe_events(ngroups)) : nullptr;
    if (c.pipe) c.ss = c.pipe->side;
    /* the fused groups' window passes (k_fwin); their histograms start at zero */
    if (any_fused && hipMemsetAsync(wsb(c.ws, c.lay.fwh), 0, FWIN_HIST_BYTES, s) != hipSuccess)
        return fail(WTP_EHIP, -1, "hipMemsetAsync failed");
    c.fts.resize(ngroups);
    for (int gi = 0; gi < ngroups; ++gi)
        if (c.fused[gi]) build_fwin_table(c, gi, c.fts[gi]);
    if (!c.pipe) /* group by group: the groups share the level temps (make_layout); a fused group's
                  * forward runs behind its window pass (forward_before_select) */
        for (int gi = 0; gi < ngroups; ++gi)
            if (!c.fused[gi]) forward_chains(c.gchains[gi], c.tp, s);
    /* pipelined: the first two fused groups' window passes on the side stream ahead of their
     * forwards (it reads the inputs: it waits for the caller's stream first); group g + 2's
     * follows group g's selection there, which has read the slot areas g + 2 reuses */
    if (c.pipe && any_fused) {
        if (hipEventRecord(ev_call_start(c), s) != hipSuccess || hipStreamWaitEvent(c.ss, ev_call_start(c), 0) != hipSuccess)
            return fail_joined(c, -1, "hipEventRecord / hipStreamWaitEvent failed");
        c.forked = true;
        if (!window_on_side(c, 0) || !window_on_side(c, 1)) return fail_joined(c, -1, "hipEventRecord failed");
    }
    return WTP_OK;
}

static int prune_impl(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, int flags, int mode,
                      void* ws, size_t ws_bytes, wtp_result* results, wtp_stream_t stream) {
    clear_error();
    if (ntensors < 0 || (ntensors > 0 && (!tensors || !results))) return fail(WTP_EARG, -1, "bad arguments");
    if (ntensors == 0) return WTP_OK;
    PruneCall c;
    c.ts = tensors;
    c.n = ntensors;
    c.pct = pct;
    c.ws = ws;
    c.results = results;
    c.opt = PruneOpts{(flags & WTP_CARRY_LEVEL) != 0, (flags & WTP_FLATTEN) != 0, (flags & WTP_NO_RESIDENT) != 0, mode};
    int rc = plan_tensors(tensors, ntensors, wavelet_id, level, pct, true, c.ps, c.opt.carry, c.opt.flat, c.opt.mode);
    if (rc != WTP_OK) return rc;
    c.tp = taps_for(wavelet_id);
    c.lay = make_layout(c.ps, c.tp);
    if (!ws || ws_bytes < c.lay.total)
        return fail(WTP_EWORKSPACE, -1, "workspace too small: need %zu bytes, got %zu", c.lay.total, ws_bytes);
    const hipStream_t s = c.s = c.ss = (hipStream_t)stream;
    c.head = wsb<SelHeader>(ws, c.lay.sel);
    c.cand = wsb<uint32_t>(ws, c.lay.cand);
    c.thr_t = wsb<float>(ws, c.lay.thr);

    stage(0, s);
    if (!c.opt.no_resident && !c.opt.flat && g_resident.load(std::memory_order_relaxed)) {
        /* a small call: the whole path in one launch (small.hip) */
        SmallTable st;
        if (plan_small(c.ps, tensors, ntensors, ws, pct, c.tp, c.cand, st)) {
            for (int i = 1; i <= 4; ++i) stage(i, s);
            launch_small(st, c.head, results, s);
            stage(5, s);
            return check_launch();
        }
    }
    /* 1. forward transforms into the packed arrays (pywt.wavedec2 + coeffs_to_array) */
    if ((rc = forward_groups(c)) != WTP_OK) return rc;
    /* 2. exact percentile selection + level-0 mask, SEG_PER_LAUNCH segments per launch group */
    for (int gi = 0; gi < c.ngroups; ++gi)
        if ((rc = select_group(c, gi)) != WTP_OK) return rc;
    /* 3. inverse transforms, group by group, then the flattened tensors' */
    for (int gi = 0; gi < c.ngroups; ++gi)
        if ((rc = inverse_group(c, gi)) != WTP_OK) return rc;
    for (int t = 0; t < ntensors; ++t) {
        const TPlan& p = c.ps[t];
        if (!p.flat || !p.dwt) continue;
        inverse_flat(p, wsb<const float>(ws, p.p_off), tensors[t].out, wsb<float>(ws, p.t_off),
                     wsb<float>(ws, p.t_off + align_up(p.t_elems * sizeof(float))), c.tp, c.thr_t + t,
                     reinterpret_cast<unsigned long long*>(&results[t].zero_count), s);
    }
    stage(5, s);
    return check_launch();
}

extern "C" {

int wtp_set_stage_events(void* const* events, int n) {
    if (n < 0 || n > 8 || (n > 0 && !events)) return fail(WTP_EARG, -1, "bad stage events");
    for (int i = 0; i < 8; ++i) g_stage_ev[i] = (i < n) ? (hipEvent_t)events[i] : nullptr;
    g_stage_n = n;
    return WTP_OK;
}
int wtp_set_resident(int mode) {
    if (mode < 0 || mode > 1) return fail(WTP_EARG, -1, "bad resident mode %d", mode);
    return g_resident.exchange(mode);
}
int wtp_set_pipeline(int mode) {
    if (mode < 0 || mode > 1) return fail(WTP_EARG, -1, "bad pipeline mode %d", mode);
    return g_pipeline.exchange(mode);
}
int wtp_set_fused_select(int mode) {
    if (mode < 0 || mode > 1) return fail(WTP_EARG, -1, "bad fused-select mode %d", mode);
    return g_fused.exchange(mode);
}

size_t wtp_workspace_size_mode(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int flags,
                               int mode_id) {
    if (ntensors < 0 || (ntensors > 0 && !tensors) || mode_check(mode_id, flags) != WTP_OK) return 0;
    return layout_bytes(tensors, ntensors, wavelet_id, level, (flags & WTP_CARRY_LEVEL) != 0, (flags & WTP_FLATTEN) != 0,
                        mode_id);
}
size_t wtp_workspace_size_ex(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, int flags) {
    if (!flags_ok(flags)) return 0; /* without a message, unlike the mode query */
    return wtp_workspace_size_mode(tensors, ntensors, wavelet_id, level, flags, WTP_MODE_PERIODIZATION);
}
size_t wtp_workspace_size(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level) {
    if (ntensors < 0 || (ntensors > 0 && !tensors)) return 0;
    /* large enough for both wtp_prune_f32 (level carried) and wtp_prune_layers_f32 */
    const size_t carried = layout_bytes(tensors, ntensors, wavelet_id, level, true, false, WTP_MODE_PERIODIZATION);
    if (!carried) return 0;
    const size_t layers = layout_bytes(tensors, ntensors, wavelet_id, level, false, false, WTP_MODE_PERIODIZATION);
    return layers ? std::max(carried, layers) : 0;
}

int wtp_prune_mode_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, int flags,
                       int mode_id, void* ws, size_t ws_bytes, wtp_result* results, wtp_stream_t stream) {
    int rc = mode_check(mode_id, flags);
    if (rc != WTP_OK) return rc;
    return prune_impl(tensors, ntensors, wavelet_id, level, pct, flags, mode_id, ws, ws_bytes, results, stream);
}
int wtp_prune_ex_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, int flags,
                     void* ws, size_t ws_bytes, wtp_result* results, wtp_stream_t stream) {
    return wtp_prune_mode_f32(tensors, ntensors, wavelet_id, level, pct, flags, WTP_MODE_PERIODIZATION, ws, ws_bytes,
                              results, stream);
}
int wtp_prune_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, void* ws,
                  size_t ws_bytes, wtp_result* results, wtp_stream_t stream) {
    return prune_impl(tensors, ntensors, wavelet_id, level, pct, WTP_CARRY_LEVEL, WTP_MODE_PERIODIZATION, ws, ws_bytes,
                      results, stream);
}
int wtp_prune_layers_f32(const wtp_tensor* tensors, int ntensors, int wavelet_id, int level, double pct, void* ws,
                         size_t ws_bytes, wtp_result* results, wtp_stream_t stream) {
    return prune_impl(tensors, ntensors, wavelet_id, level, pct, 0, WTP_MODE_PERIODIZATION, ws, ws_bytes, results, stream);
}

/* percentile_based_thresholding: one 1-D tensor through the path (no wavelet lookup) */
int wtp_threshold_f32(const float* in, float* out, int64_t n, double pct, void* ws, size_t ws_bytes,
                      wtp_result* result, wtp_stream_t stream) {
    wtp_tensor t;
    memset(&t, 0, sizeof t);
    t.in = in;
    t.out = out;
    t.ndim = 1;
    t.shape[0] = n;
    return wtp_prune_f32(&t, 1, -1, 0, pct, ws, ws_bytes, result, stream);
}

}  // extern "C"

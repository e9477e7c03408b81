/*
 * fb_launch.inc -- the filter bank's host side: a call's items become kernel arguments, are grouped
 * by geometry, and each group runs the launches that fb_plan.h plans for its tile grid.  After
 * fb_fwd.inc and fb_inv.inc.
 */
#include <atomic>
#include <cstring>
#include <utility>
#include <vector>

namespace wtp {

/* the interior mode (fb_plan.h, fb_plan) */
static std::atomic<int> g_fb_interior{3};
int fb_set_interior(int mode) { return g_fb_interior.exchange(mode < 0 ? 0 : (mode > 3 ? 3 : mode)); }

bool fb_tiled_ok(int64_t B, int64_t R, int64_t C, const Taps& tp) { return fb_tiled_ok(B, R, C, (int)tp.F); }

/* the runtime filter length as a compile-time one: fn(std::integral_constant<int, FT>) with FT = F
 * for the specialised lengths (fb_plan.h, FB_SPEC_F), else FT = 0 */
template <class Fn, size_t... K>
static void by_filter(int F, const Fn& fn, std::index_sequence<K...>) {
    if (!((F == FB_SPEC_F[K] && (fn(std::integral_constant<int, FB_SPEC_F[K]>{}), true)) || ...))
        fn(std::integral_constant<int, 0>{});
}
template <class Fn>
static void by_filter(int F, const Fn& fn) { by_filter(F, fn, std::make_index_sequence<FB_N_SPEC>{}); }

template <int FT>
static TapsT<FT> taps_of(const Taps& tp) {
    if constexpr (FT == 0) {
        return tp;
    } else {
        SmallTaps t;
        memset(&t, 0, sizeof t);
        t.F = tp.F;
        for (int k = 0; k < 4; ++k)
            for (int j = 0; j < FT; ++j) t.f[k][j] = tp.f[k][j];
        return t;
    }
}
template <int FT>
static void fwd_go(const FwdGroup& g, int grid, const Taps& tp, hipStream_t s) {
    static_assert(FT <= SM_F_MAX, "SmallTaps holds the specialised filters");
    hipLaunchKernelGGL(k_fwd_level<FT>, dim3(grid), dim3(FB_THREADS), fwd_lds(tp.F, FT > 0), s, g, taps_of<FT>(tp));
}
template <int FT, bool EDGE>
static void fwd_int_go(const FwdGroup& g, int grid, const Taps& tp, const FwdSel& fs, hipStream_t s) {
    FwdIntTaps t;
    memset(&t, 0, sizeof t);
    for (int j = 0; j < FT; ++j) t.t[j] = f2{tp.f[0][j], tp.f[1][j]};
    hipLaunchKernelGGL((k_fwd_int<FT, EDGE>), dim3(grid), dim3(FB_THREADS), fwd_int_lds(tp.F), s, g, t, fs);
}
template <int FT>
static void inv_go(const InvGroup& g, int grid, const Taps& tp, hipStream_t s) {
    hipLaunchKernelGGL(k_inv_level<FT>, dim3(grid), dim3(FB_THREADS), inv_lds(tp.F, FT > 0), s, g, taps_of<FT>(tp));
}
template <int FT, bool EDGE>
static void inv_int_go(const InvGroup& g, int grid, const Taps& tp, hipStream_t s) {
    hipLaunchKernelGGL((k_inv_int<FT, EDGE>), dim3(grid), dim3(FB_THREADS), inv_lds(tp.F, true), s, g, taps_of<FT>(tp));
}

static FwdArgs fwd_args(const FwdItem& x) {
    FwdArgs a;
    memset(&a, 0, sizeof a);
    a.in = x.in;
    a.in_bs = x.R * x.C;
    a.R = (int)x.R;
    a.C = (int)x.C;
    a.Ro = (int)((x.R + 1) / 2);
    a.Co = (int)((x.C + 1) / 2);
    a.P = x.P;
    a.P_bs = x.PR * x.PC;
    a.PC = (int)x.PC;
    a.offR = (int)x.offR;
    a.offC = (int)x.offC;
    a.anext = x.anext;
    a.last = x.last;
    a.tilesC = fb_tiles(a.Co, FC);
    a.tilesR = fb_tiles(a.Ro, FR);
    a.al16 = (reinterpret_cast<uintptr_t>(x.in) % 16) == 0 && (x.C % 4) == 0;
    return a;
}

static InvArgs inv_args(const InvItem& x) {
    InvArgs a;
    memset(&a, 0, sizeof a);
    a.a = x.a_src ? x.a_src : x.P;
    a.a_bs = x.a_bs;
    a.lda = (int)x.lda;
    a.a_from_P = x.a_from_P;
    a.P = x.P;
    a.P_bs = x.PR * x.PC;
    a.PC = (int)x.PC;
    a.offR = (int)x.offR;
    a.offC = (int)x.offC;
    a.R = (int)x.R;
    a.C = (int)x.C;
    a.y = x.y;
    a.outH = (int)x.outH;
    a.outW = (int)x.outW;
    a.thr = x.thr;
    a.zc = x.zc;
    a.tilesC = fb_tiles(x.outW, IC);
    a.tilesR = fb_tiles(x.outH, IR);
    return a;
}

static_assert(sizeof(FwdGroup) + sizeof(Taps) <= 3840 && sizeof(InvGroup) + sizeof(Taps) <= 3840,
              "filter-bank kernel arguments (plus the hidden ones) stay under 4 KB");

/* the plan of a forward / inverse group's level: its grid, its interior rectangle, its edge predicate */
static FbPlan fwd_plan(const FwdArgs& a, int B, int n, int F, int mode) {
    FbRect q;
    const bool has = fwd_interior(a.R, a.C, a.Ro, a.Co, a.al16, a.P_bs, F, &q);
    return fb_plan(a.tilesR, a.tilesC, B, n, has ? &q : nullptr, true, fb_specialised(F), mode);
}
static FbPlan inv_plan(const InvArgs& a, int B, int n, int F, int mode) {
    FbRect q;
    const bool has = inv_interior(a.R, a.C, a.outH, a.outW, a.P_bs, a.a_from_P ? 0 : a.a_bs, F, &q);
    return fb_plan(a.tilesR, a.tilesC, B, n, has ? &q : nullptr, inv_frame_ok(a.R, a.C, F), fb_specialised(F), mode);
}
/* a group's argument for one launch of its plan */
template <class Group>
static Group group_of(const Group& g, const FbLaunch& l) {
    Group x = g;
    x.geo.tr0 = l.rect.r0; x.geo.nTR = l.rect.nr; x.geo.tc0 = l.rect.c0; x.geo.nTC = l.rect.nc;
    x.geo.frame = l.frame;
    x.tiles = l.tiles;
    x.dv_tiles = l.dv_tiles; x.dv_per = l.dv_per; x.dv_ntc = l.dv_ntc;
    x.dv_tc = l.dv_tc; x.dv_side = l.dv_side;
    return x;
}

/* fused selection: a level of (B, R, C) images runs only in k_fwd_int (the interior rectangle and
 * the edge form, interior mode 2 or 3; any_mode: as if the mode were 3), whose waves classify what
 * they write; the slots are one per wave of every tile */
bool fwd_level_fused_ok(const FwdItem& x, const Taps& tp, int64_t* slots, bool any_mode) {
    const int mode = any_mode ? 3 : g_fb_interior.load(std::memory_order_relaxed);
    if (mode < 2 || !fb_tiled_ok(x.B, x.R, x.C, tp)) return false;
    const FwdArgs a = fwd_args(x);
    const FbPlan p = fwd_plan(a, (int)x.B, 1, tp.F, mode);
    for (int k = 0; k < p.n; ++k)
        if (p.l[k].kind == FB_GENERAL) return false;
    *slots = (int64_t)a.tilesR * a.tilesC * x.B * (FB_THREADS / 64);
    return true;
}

void launch_fwd_levels(const FwdItem* it, int n, const Taps& tp, hipStream_t s, bool fused) {
    std::vector<FwdArgs> args(n);
    std::vector<int64_t> tiles(n);
    for (int i = 0; i < n; ++i) {
        args[i] = fwd_args(it[i]);
        tiles[i] = (int64_t)args[i].tilesC * args[i].tilesR * it[i].B;
    }
    auto same = [&](int i, int j) {
        const FwdArgs &x = args[i], &y = args[j];
        return x.in_bs == y.in_bs && x.R == y.R && x.C == y.C && x.Ro == y.Ro && x.Co == y.Co && x.P_bs == y.P_bs &&
               x.PC == y.PC && x.offR == y.offR && x.offC == y.offC && x.last == y.last && x.al16 == y.al16;
    };
    const int mode = g_fb_interior.load(std::memory_order_relaxed);
    for (const auto& grp : fb_groups(tiles, same, FB_UNI)) {
        FwdGroup g;
        memset(&g, 0, sizeof g);
        g.geo = args[grp[0]];
        g.n = (int)grp.size();
        for (int m = 0; m < g.n; ++m) {
            g.in[m] = args[grp[m]].in;
            g.anext[m] = args[grp[m]].anext;
            g.P[m] = args[grp[m]].P;
        }
        /* fused selection: the items' slots (a fused launch group holds at most SEG_PER_LAUNCH
         * chains, so at most that many items of one level) */
        const bool fsel = fused && it[grp[0]].fslot && g.n <= SEG_PER_LAUNCH;
        const FbPlan p = fwd_plan(g.geo, (int)it[grp[0]].B, g.n, tp.F, mode);
        for (int k = 0; k < p.n; ++k) {
            const FbLaunch& l = p.l[k];
            const FwdGroup gl = group_of(g, l);
            FwdSel fs;
            memset(&fs, 0, sizeof fs);
            fs.on = fsel;
            for (int m = 0; fsel && m < g.n; ++m) { /* a launch's slots follow those of the launches before it */
                fs.slots[m] = it[grp[m]].fslot + (int64_t)l.before * (FB_THREADS / 64) * FSL_WORDS;
                fs.hdr[m] = it[grp[m]].fhdr;
            }
            by_filter(tp.F, [&](auto ft) {
                constexpr int FT = decltype(ft)::value;
                if (l.kind == FB_GENERAL) fwd_go<FT>(gl, gl.n * gl.tiles, tp, s);
                else if constexpr (FT > 0) {
                    if (l.kind == FB_EDGE) fwd_int_go<FT, true>(gl, gl.n * gl.tiles, tp, fs, s);
                    else fwd_int_go<FT, false>(gl, gl.n * gl.tiles, tp, fs, s);
                }
            });
        }
    }
}

void launch_inv_levels(const InvItem* it, int n, const Taps& tp, hipStream_t s) {
    std::vector<InvArgs> args(n);
    std::vector<int64_t> tiles(n);
    for (int i = 0; i < n; ++i) {
        args[i] = inv_args(it[i]);
        tiles[i] = (int64_t)args[i].tilesC * args[i].tilesR * it[i].B;
    }
    /* one geometry, and the threshold / zero-count words at whole-element offsets from the
     * group's first ones (or absent in all of them) */
    auto off_ok = [](const void* p, const void* q, size_t elem) {
        if ((p == nullptr) != (q == nullptr)) return false;
        if (!p) return true;
        const intptr_t d = reinterpret_cast<intptr_t>(q) - reinterpret_cast<intptr_t>(p);
        return d % (intptr_t)elem == 0 && d / (intptr_t)elem >= INT16_MIN && d / (intptr_t)elem <= INT16_MAX;
    };
    auto same = [&](int i, int j) {
        const InvArgs &x = args[i], &y = args[j];
        return x.a_bs == y.a_bs && x.lda == y.lda && x.a_from_P == y.a_from_P && x.P_bs == y.P_bs && x.PC == y.PC &&
               x.offR == y.offR && x.offC == y.offC && x.R == y.R && x.C == y.C && x.outH == y.outH &&
               x.outW == y.outW && off_ok(x.thr, y.thr, sizeof(float)) &&
               off_ok(x.zc, y.zc, sizeof(unsigned long long));
    };
    const int mode = g_fb_interior.load(std::memory_order_relaxed);
    for (const auto& grp : fb_groups(tiles, same, FB_UNI)) {
        InvGroup g;
        memset(&g, 0, sizeof g);
        g.geo = args[grp[0]];
        g.n = (int)grp.size();
        for (int m = 0; m < g.n; ++m) {
            const InvArgs& x = args[grp[m]];
            g.a[m] = x.a;
            g.P[m] = x.P;
            g.y[m] = x.y;
            const int32_t to = x.thr ? (int32_t)(x.thr - g.geo.thr) : 0, zo = x.zc ? (int32_t)(x.zc - g.geo.zc) : 0;
            g.tz_off[m] = (int32_t)(((uint32_t)zo << 16) | ((uint32_t)to & 0xFFFFu)); /* off_ok: both within int16 */
        }
        const FbPlan p = inv_plan(g.geo, (int)it[grp[0]].B, g.n, tp.F, mode);
        for (int k = 0; k < p.n; ++k) {
            const FbLaunch& l = p.l[k];
            const InvGroup gl = group_of(g, l);
            by_filter(tp.F, [&](auto ft) {
                constexpr int FT = decltype(ft)::value;
                if (l.kind == FB_GENERAL) inv_go<FT>(gl, gl.n * gl.tiles, tp, s);
                else if constexpr (FT > 0) {
                    if (l.kind == FB_EDGE) inv_int_go<FT, true>(gl, gl.n * gl.tiles, tp, s);
                    else inv_int_go<FT, false>(gl, gl.n * gl.tiles, tp, s);
                }
            });
        }
    }
}

void launch_fwd_level(const float* in, int64_t B, int64_t R, int64_t C, const Taps& tp, float* anext, float* P,
                      int64_t PR, int64_t PC, int64_t offR, int64_t offC, int last, hipStream_t s) {
    const FwdItem x{in, B, R, C, anext, P, PR, PC, offR, offC, last};
    launch_fwd_levels(&x, 1, tp, s);
}

void launch_inv_level(const float* a_src, int64_t a_bs, int64_t lda, int a_from_P, const float* P, int64_t PR,
                      int64_t PC, int64_t offR, int64_t offC, int64_t B, int64_t R, int64_t C, const Taps& tp,
                      const float* thr, float* y, int64_t outH, int64_t outW, unsigned long long* zc,
                      hipStream_t s) {
    const InvItem x{a_src, a_bs, lda, a_from_P, P, PR, PC, offR, offC, B, R, C, thr, y, outH, outW, zc};
    launch_inv_levels(&x, 1, tp, s);
}

}  // namespace wtp

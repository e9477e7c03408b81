/* Tile geometry and launch plan of the filter bank (filterbank.hip), shared by its kernels, its
 * launchers (fb_launch.inc) and the host-compiled CPU check tests/native/fbplan.cpp: the tile sizes,
 * the forward tile's LDS layout and the inverse tile's coefficient window as functions of the filter
 * length, the dynamic LDS of every kernel, the interior rectangle of a level's tile grid, the
 * grouping of a call's items, and which kernel runs which tiles.  Integers only: no HIP, no pointers. */
#ifndef WT_FB_PLAN_H
#define WT_FB_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "fb_index.h"
#include "wt_dwt_core.h"

namespace wtp {

constexpr int FB_THREADS = 256;
/* forward output tile (per subband).  FC = 56: the axis -2 pass has 2 (2 FC + F - 2) column items,
 * <= 256 for F <= 18, so every thread of the workgroup takes exactly one (with FC = 64 and db8,
 * 284 items: wave 0 -- always on the same SIMD -- took a second one, doubling that SIMD's share
 * of the pass; cfg5 forward levels -5 %) */
constexpr int FR = 16, FC = 56;
constexpr int IR = 64, IC = 64;  /* inverse output tile */
constexpr int FB_UNI = 64;       /* items of one geometry a launch takes (FwdGroup / InvGroup) */
constexpr int FB_MAX_LDS = 64 * 1024;
/* the filter lengths with kernels of their own (FT = F); every other length runs FT = 0 */
constexpr int FB_SPEC_F[] = {2, 4, 6, 8, 10, 12, 16, 18};
constexpr int FB_N_SPEC = (int)(sizeof(FB_SPEC_F) / sizeof(FB_SPEC_F[0]));
constexpr bool fb_specialised(int F) {
    for (int k = 0; k < FB_N_SPEC; ++k)
        if (FB_SPEC_F[k] == F) return true;
    return false;
}

constexpr size_t fb_max(size_t a, size_t b) { return a > b ? a : b; }

/* ---- the forward tile: FR x FC outputs from (2 FR + F - 2) x (2 FC + F - 2) inputs ---- */
constexpr int fwd_nr(int F) { return 2 * FR + F - 2; }
constexpr int fwd_nc(int F) { return 2 * FC + F - 2; }
/* the input tile in LDS (specialised filters): row pitch fwd_tp floats, the tile's first column at
 * fwd_s0 -- so that its column 0 - fwd_s0 is 16-byte aligned in the image (a tile's first input
 * column is 2 FC tc - F/2 + 1) and interior rows load as whole float4s */
constexpr int fwd_s0(int F) { return ((1 - F / 2) % 4 + 4) % 4; }
constexpr int fwd_tp(int F) { return (fwd_s0(F) + fwd_nc(F) + 3) / 4 * 4; }
/* k_fwd_int's column-pass results in LDS: row o holds its even columns from o * 2 LHH, its odd ones
 * from o * 2 LHH + LHH (float2 units).  LHH = 8 (mod 16): a wave's float2 writes of consecutive
 * columns then put the even lanes on banks b .. b + 15 and the odd lanes on b + 16 .. b + 31 of
 * each 16-lane group (with LHH = (NC + 1) / 2 = 63 at db8 the two halves overlapped on 14 banks:
 * 0.69 bank-conflict cycles per LDS instruction, round-5 PMC); the row pass reads stay contiguous */
constexpr int fwd_lhh(int nc) { return (nc + 1) / 2 + ((8 - (nc + 1) / 2) % 16 + 16) % 16; }
/* ---- the inverse tile: IR x IC outputs; k_inv_int's coefficient window along either axis ---- */
static_assert(IR == IC, "one window serves both axes");
constexpr int inv_win(int F) { return IR / 2 + F / 2 - ((F / 2) & 1); }

/* dynamic LDS per workgroup; `alias`: the specialised kernels write their second-pass input over
 * their first-pass input (k_fwd_level: LH over T; k_inv_level and k_inv_int: LoHi over Aq/Dq).  The
 * aliased forward pitch is taken at the largest fwd_s0 (3), so it is >= fwd_tp: an over-estimate
 * the occupancy was tuned with */
constexpr size_t fwd_lds(int F, bool alias = false) {
    const size_t pitch = alias ? (size_t)(3 + fwd_nc(F) + 3) / 4 * 4 : (size_t)fwd_nc(F);
    /* lh: k_fwd_level's FR x NC float2 rows, or k_fwd_int's FR rows of 2 fwd_lhh(NC) float2 (the larger) */
    const size_t t = (size_t)fwd_nr(F) * pitch,
                 lh = 2 * (size_t)FR * fb_max((size_t)fwd_nc(F), 2 * (size_t)fwd_lhh(fwd_nc(F)));
    return sizeof(float) * (alias ? fb_max(t, lh) : t + lh);
}
/* k_fwd_int's exact dynamic LDS: its input tile at pitch fwd_tp, then its column results over it at
 * the fwd_lhh half pitch -- the occupancy is LDS-bound (db8: 46 x 128 floats = 23 KB, six
 * workgroups per CU) */
constexpr size_t fwd_int_lds(int F) {
    const size_t t = (size_t)fwd_nr(F) * (size_t)fwd_tp(F), lh = 2 * (size_t)FR * 2 * (size_t)fwd_lhh(fwd_nc(F));
    return sizeof(float) * fb_max(t, lh);
}
/* the tile bounds of k_inv_level (IR/2 + H rows, IC/2 + H columns): db8 40 x 40, 25.6 KB aliased --
 * six workgroups per CU instead of five */
constexpr size_t inv_lds(int F, bool alias = false) {
    const size_t nr = IR / 2 + F / 2, nc = IC / 2 + F / 2;
    return sizeof(float) * (alias ? fb_max(4 * nr * nc, 2 * nr * IC) : 4 * nr * nc + 2 * nr * IC);
}

constexpr int fb_tiles(int64_t out, int T) { return (int)((out + T - 1) / T); }

/* The tiled path needs an even filter, the LDS budget, and images large enough that a tile is
 * mostly useful work (tiny conv kernels keep the per-point kernels). */
static inline bool fb_tiled_ok(int64_t B, int64_t R, int64_t C, int F) {
    if ((F & 1) || fwd_lds(F) > FB_MAX_LDS || inv_lds(F) > FB_MAX_LDS) return false;
    if (R > (1 << 28) || C > (1 << 28) || B * R * C > ((int64_t)1 << 31)) return false;
    return R * C >= 512; /* at least a quarter of a forward tile of outputs */
}

/* ---- the interior rectangle of a level's tile grid ---- */
struct FbRect {
    int r0, nr, c0, nc; /* tile rows r0 .. r0 + nr - 1, tile columns c0 .. c0 + nc - 1 */
};

/* one axis of the forward grid: tile t is interior when the `span` input samples from
 * 2 T t - F/2 + 1 - lead lie inside the line of N and the tile is full (T outputs of `out`) */
static inline bool fwd_axis(int T, int lead, int span, int N, int out, int F, int* lo, int* cnt) {
    int a = -1, z = -2;
    for (int t = 0; t < fb_tiles(out, T); ++t) {
        const int st = 2 * T * t - F / 2 + 1 - lead;
        if (st >= 0 && st + span <= N && (t + 1) * T <= out) { if (a < 0) a = t; z = t; }
    }
    *lo = a;
    *cnt = z - a + 1;
    return a >= 0;
}
/* The interior rectangle of a forward level (k_fwd_int's tiles): a tile row is interior when its
 * input rows lie inside the image (no extension; then every output site of it is interior too,
 * i < R) and it is full; a tile column when its aligned float4 window [gc0 - S0, gc0 - S0 + TP)
 * lies inside the row and it is full.  Both conditions are intervals of the tile index.  False: no
 * interior tile (or offsets beyond the kernel's 32-bit buffer offsets) -- k_fwd_level takes the
 * whole grid.  al16: the input is 16-byte aligned and C % 4 == 0; P_bs: the packed image's elements. */
static inline bool fwd_interior(int R, int C, int Ro, int Co, int al16, int64_t P_bs, int F, FbRect* q) {
    if (!al16 || (int64_t)4 * P_bs > INT32_MAX || (int64_t)4 * Ro * Co > INT32_MAX) return false;
    if ((int64_t)4 * (2 * FR + F) * C > INT32_MAX) return false; /* k_fwd_int's tile loads: 32-bit offsets */
    return fwd_axis(FR, 0, fwd_nr(F), R, Ro, F, &q->r0, &q->nr) &&
           fwd_axis(FC, fwd_s0(F), fwd_tp(F), C, Co, F, &q->c0, &q->nc);
}

/* One axis of a synthesis level (k_inv_int's tiles): a tile is interior when it is full, holds no
 * special site (H even: outputs 0 and 2N - 1), its last site is below N and its first site's
 * window starts at or after 0 -- the sites grow with the output index, so the interior tiles are
 * an interval. */
static inline bool inv_axis(int T, int out, int N, int F, int* lo, int* cnt) {
    const int H = F / 2;
    int a = -1, z = -2;
    for (int t = 0; t < fb_tiles(out, T); ++t) {
        const int n0 = t * T, nl = n0 + T - 1;
        if (nl >= out) continue;
        const wt_syn_site s0 = wt_syn_locate(n0, N, F), s1 = wt_syn_locate(nl, N, F);
        if (s0.special || s1.special || (H % 2 == 0 && (n0 == 0 || nl >= 2 * N - 1))) continue;
        if (s1.i >= N || s0.i - H + 1 < 0) continue;
        if (a < 0) a = t;
        z = t;
    }
    *lo = a;
    *cnt = z - a + 1;
    return a >= 0;
}
/* a_bs: the approximation's batch stride when it is not read from the packed image, else 0 */
static inline bool inv_interior(int R, int C, int outH, int outW, int64_t P_bs, int64_t a_bs, int F, FbRect* q) {
    if ((int64_t)4 * P_bs > INT32_MAX || (int64_t)4 * outH * outW > INT32_MAX || (int64_t)4 * a_bs > INT32_MAX)
        return false;
    return inv_axis(IR, outH, R, F, &q->r0, &q->nr) && inv_axis(IC, outW, C, F, &q->c0, &q->nc);
}
/* k_inv_int's EDGE form wraps a window coordinate once: the level spans a whole window */
static inline bool inv_frame_ok(int R, int C, int F) { return R >= inv_win(F) && C >= inv_win(F); }

/* ---- which kernels run a level's tiles ---- */
/* Interior mode: 3 (default) as 2, except that a level of at most FB_ONE_LAUNCH_TILES tiles (all
 * items of the launch) runs every tile in ONE launch of the EDGE form; 2 the interior rectangle in
 * k_fwd_int / k_inv_int and the frame around it in their EDGE forms (two launches); 1 the frame in
 * the general k_fwd_level / k_inv_level; 0 every tile in the general kernels (A/B and parity
 * cross-checks) */
constexpr int64_t FB_ONE_LAUNCH_TILES = 8192;
enum FbKind { FB_GENERAL = 0, FB_INTERIOR = 1, FB_EDGE = 2 };
struct FbLaunch {
    int kind;
    int tiles;      /* per item: the rectangle's, the frame's or the grid's, times B */
    FbRect rect;    /* geo.tr0 / nTR / tc0 / nTC */
    int frame;      /* geo.frame: the tiles AROUND rect */
    FastDiv dv_tiles, dv_per, dv_ntc; /* k_*_int: by tiles, by the rectangle's (or frame's) tiles, by nTC */
    FastDiv dv_tc, dv_side;           /* the frame's decode: by tilesC, by tilesC - nTC */
    int before;     /* tiles per item that the plan's earlier launches ran (fused selection: slots) */
};
struct FbPlan {
    int n;
    FbLaunch l[2];
};
static inline FbLaunch fb_launch(int kind, int per, int B, int tilesC, const FbRect& q, int frame, int before) {
    FbLaunch l;
    l.kind = kind;
    l.tiles = per * B;
    l.rect = q;
    l.frame = frame;
    l.dv_tiles = make_fastdiv((uint32_t)l.tiles);
    l.dv_per = make_fastdiv((uint32_t)per);
    l.dv_ntc = make_fastdiv((uint32_t)(q.nc > 1 ? q.nc : 1));
    l.dv_tc = make_fastdiv((uint32_t)tilesC);
    l.dv_side = make_fastdiv((uint32_t)(tilesC - q.nc > 1 ? tilesC - q.nc : 1));
    l.before = before;
    return l;
}
/* The launches of one level of n items of B images on a tilesR x tilesC grid.  rect: the interior
 * rectangle, or null; edge_ok: the EDGE form may run (the inverse: inv_frame_ok); spec: the filter
 * has kernels of its own.  The interior tiles run first, then the frame around them (measured in
 * round 4: the frame on a stream of its own beside the interior launch gained nothing -- both
 * launches fill every CU, so the work only moved). */
static inline FbPlan fb_plan(int tilesR, int tilesC, int B, int n, const FbRect* rect, bool edge_ok, bool spec, int mode) {
    const FbRect none = {0, 0, 0, 0};
    const int grid = tilesR * tilesC;
    FbPlan p;
    p.n = 1;
    if (!mode || !spec || !rect) {
        p.l[0] = fb_launch(FB_GENERAL, grid, B, tilesC, none, 0, 0);
        return p;
    }
    const int in = rect->nr * rect->nc, fr = grid - in;
    if (mode == 3 && fr > 0 && edge_ok && (int64_t)n * grid * B <= FB_ONE_LAUNCH_TILES) {
        /* a small level: every tile in ONE launch of the edge form (its decode with an empty
         * rectangle walks the whole grid row-major; interior tiles take its interior paths), where
         * the interior and the frame as two launches were latency cliffs (round 4: the frame's
         * launch as long as the interior's at levels 3-5) */
        p.l[0] = fb_launch(FB_EDGE, grid, B, tilesC, none, 0, 0);
        return p;
    }
    p.l[0] = fb_launch(FB_INTERIOR, in, B, tilesC, *rect, 0, 0);
    if (fr > 0) p.l[p.n++] = fb_launch(mode >= 2 && edge_ok ? FB_EDGE : FB_GENERAL, fr, B, tilesC, *rect, 1, in * B);
    return p;
}

/* Items are grouped by geometry (their order does not matter: every item is independent); each
 * launch takes up to `cap` items of one geometry whose tiles sum below 2^31 (fb_tiled_ok bounds
 * every item's B * R * C below 2^31 elements, hence its tiles far below).  same(i, j): items i and j
 * may share a launch; the first item of a group stands for its geometry. */
template <class Same>
static inline std::vector<std::vector<int>> fb_groups(const std::vector<int64_t>& tiles, const Same& same, int cap) {
    std::vector<std::vector<int>> groups;
    for (int i = 0; i < (int)tiles.size(); ++i) {
        int gi = -1;
        for (int j = 0; j < (int)groups.size() && gi < 0; ++j) {
            const int r = groups[j][0];
            if ((int)groups[j].size() < cap && tiles[r] == tiles[i] && same(r, i) &&
                tiles[i] * (int64_t)(groups[j].size() + 1) <= INT32_MAX)
                gi = j;
        }
        if (gi < 0) {
            groups.emplace_back();
            gi = (int)groups.size() - 1;
        }
        groups[gi].push_back(i);
    }
    return groups;
}

}  // namespace wtp

#endif

/* csrc/fb_plan.h compiled for the host (no HIP header): the filter bank's tile constants, LDS sizes,
 * interior intervals and launch plan as the library computes them, for tests/test_fb_plan.py and
 * tests/test_interior_algebra.py.  Built as a shared library for ctypes; with FBPLAN_MAIN it is the
 * stand-alone sanitizer driver of tests/test_sanitizers.py, which walks the grid of levels below. */
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../wavelettransforms_amd/csrc/fb_plan.h"

using namespace wtp;

/* FB_THREADS, FR, FC, IR, IC, FB_UNI, FB_MAX_LDS, FB_ONE_LAUNCH_TILES, then the specialised lengths */
extern "C" int fbp_consts(int64_t* out) {
    const int64_t c[] = {FB_THREADS, FR, FC, IR, IC, FB_UNI, FB_MAX_LDS, FB_ONE_LAUNCH_TILES};
    int k = 0;
    for (int64_t v : c) out[k++] = v;
    for (int f : FB_SPEC_F) out[k++] = f;
    return k;
}

/* fwd_lds, fwd_lds aliased, fwd_int_lds, inv_lds, inv_lds aliased, fb_specialised, fwd_s0, fwd_tp,
 * fwd_lhh of the tile's columns, inv_win */
extern "C" void fbp_filter(int F, int64_t* out) {
    const int64_t v[] = {(int64_t)fwd_lds(F), (int64_t)fwd_lds(F, true), (int64_t)fwd_int_lds(F), (int64_t)inv_lds(F),
                         (int64_t)inv_lds(F, true), fb_specialised(F), fwd_s0(F), fwd_tp(F), fwd_lhh(fwd_nc(F)),
                         inv_win(F)};
    int k = 0;
    for (int64_t x : v) out[k++] = x;
}

extern "C" int fbp_tiled_ok(int64_t B, int64_t R, int64_t C, int F) { return fb_tiled_ok(B, R, C, F); }

/* q = r0, nr, c0, nc */
extern "C" int fbp_fwd_interior(int R, int C, int al16, int64_t P_bs, int F, int* q) {
    FbRect r = {0, 0, 0, 0};
    const bool ok = fwd_interior(R, C, (R + 1) / 2, (C + 1) / 2, al16, P_bs, F, &r);
    q[0] = r.r0; q[1] = r.nr; q[2] = r.c0; q[3] = r.nc;
    return ok;
}
extern "C" int fbp_inv_axis(int T, int out, int N, int F, int* lo, int* cnt) { return inv_axis(T, out, N, F, lo, cnt); }
extern "C" int fbp_inv_interior(int R, int C, int outH, int outW, int64_t P_bs, int64_t a_bs, int F, int* q) {
    FbRect r = {0, 0, 0, 0};
    const bool ok = inv_interior(R, C, outH, outW, P_bs, a_bs, F, &r);
    q[0] = r.r0; q[1] = r.nr; q[2] = r.c0; q[3] = r.nc;
    return ok;
}
extern "C" int fbp_inv_frame_ok(int R, int C, int F) { return inv_frame_ok(R, C, F); }

/* One launch as the fixture records it: kind, tiles per item, r0, nr, c0, nc, frame, before, then
 * (m, sh) of dv_tiles, dv_per, dv_ntc, dv_tc, dv_side: FBP_LW numbers. */
enum { FBP_LW = 18 };
static void put_launch(const FbLaunch& l, int64_t* o) {
    const int64_t v[FBP_LW] = {l.kind, l.tiles, l.rect.r0, l.rect.nr, l.rect.c0, l.rect.nc, l.frame, l.before,
                               l.dv_tiles.m, l.dv_tiles.sh, l.dv_per.m, l.dv_per.sh, l.dv_ntc.m, l.dv_ntc.sh,
                               l.dv_tc.m, l.dv_tc.sh, l.dv_side.m, l.dv_side.sh};
    for (int k = 0; k < FBP_LW; ++k) o[k] = v[k];
}
extern "C" int fbp_plan(int tilesR, int tilesC, int B, int n, const int* rect, int edge_ok, int spec, int mode,
                        int64_t* out) {
    FbRect q = {0, 0, 0, 0};
    if (rect) q = FbRect{rect[0], rect[1], rect[2], rect[3]};
    const FbPlan p = fb_plan(tilesR, tilesC, B, n, rect ? &q : nullptr, edge_ok != 0, spec != 0, mode);
    for (int k = 0; k < p.n; ++k) put_launch(p.l[k], out + k * FBP_LW);
    return p.n;
}

/* The tiles of one item that a plan's launches run, decoded as the kernels decode them (k_*_int by
 * the launch's FastDivs, the general kernels by division): returns how many (image, tile) pairs
 * of the B x tilesR x tilesC grid are not run exactly once, plus the decodes outside the grid. */
extern "C" int fbp_cover(int tilesR, int tilesC, int B, int n, const int* rect, int edge_ok, int spec, int mode) {
    FbRect q = {0, 0, 0, 0};
    if (rect) q = FbRect{rect[0], rect[1], rect[2], rect[3]};
    const FbPlan p = fb_plan(tilesR, tilesC, B, n, rect ? &q : nullptr, edge_ok != 0, spec != 0, mode);
    std::vector<int> seen((size_t)B * tilesR * tilesC, 0);
    int bad = 0;
    for (int k = 0; k < p.n; ++k) {
        const FbLaunch& l = p.l[k];
        const FbRect& r = l.rect;
        for (int tile = 0; tile < l.tiles; ++tile) {
            int b, tr, tc;
            if (l.kind == FB_INTERIOR) {
                const int per = r.nr * r.nc;
                b = fdiv(tile, l.dv_per);
                const int t2 = tile - b * per, trr = fdiv(t2, l.dv_ntc);
                tr = r.r0 + trr;
                tc = r.c0 + t2 - trr * r.nc;
            } else if (l.kind == FB_EDGE) {
                const int per = tilesR * tilesC - r.nr * r.nc;
                b = fdiv(tile, l.dv_per);
                frame_tile_fd(tile - b * per, tilesC, r.r0, r.nr, r.c0, r.nc, l.dv_tc, l.dv_side, &tr, &tc);
            } else if (l.frame) {
                const int per = tilesR * tilesC - r.nr * r.nc;
                b = tile / per;
                frame_tile(tile - b * per, tilesC, r.r0, r.nr, r.c0, r.nc, &tr, &tc);
            } else {
                tc = tile % tilesC;
                tr = (tile / tilesC) % tilesR;
                b = tile / (tilesC * tilesR);
            }
            if (b < 0 || b >= B || tr < 0 || tr >= tilesR || tc < 0 || tc >= tilesC) { ++bad; continue; }
            ++seen[((size_t)b * tilesR + tr) * tilesC + tc];
        }
    }
    for (int s : seen) bad += s != 1;
    return bad;
}

/* A whole level: n items (dir 0: B, R, C, misalignment of the input; dir 1: B, R, C, outH, outW,
 * a_from_P -- the items of tools/gen_golden_fb_plan.py, packed images of 2 Ro x 2 Co) grouped and
 * planned as launch_fwd_levels / launch_inv_levels do it.  Per launch: n items, FBP_LW numbers,
 * then the items' indices.  Returns the launches, or -1 when `cap` numbers do not hold them. */
extern "C" int fbp_level(int dir, int F, int mode, int n, const int64_t* items, int64_t* out, int cap) {
    const int W = dir ? 6 : 4;
    std::vector<int64_t> tiles(n);
    auto it = [&](int i, int k) { return items[i * W + k]; };
    auto rows = [&](int i) { return dir ? fb_tiles(it(i, 3), IR) : fb_tiles((it(i, 1) + 1) / 2, FR); };
    auto cols = [&](int i) { return dir ? fb_tiles(it(i, 4), IC) : fb_tiles((it(i, 2) + 1) / 2, FC); };
    for (int i = 0; i < n; ++i) tiles[i] = (int64_t)rows(i) * cols(i) * it(i, 0);
    auto al16 = [&](int i) { return it(i, 3) % 16 == 0 && it(i, 2) % 4 == 0; };
    auto same = [&](int i, int j) {
        for (int k = 1; k < W; ++k)
            if (dir ? it(i, k) != it(j, k) : (k < 3 && it(i, k) != it(j, k))) return false;
        return dir || al16(i) == al16(j);
    };
    int launches = 0, used = 0;
    for (const auto& grp : fb_groups(tiles, same, FB_UNI)) {
        const int i = grp[0], B = (int)it(i, 0), R = (int)it(i, 1), C = (int)it(i, 2);
        FbRect q;
        bool has, edge_ok = true;
        if (dir) {
            has = inv_interior(R, C, (int)it(i, 3), (int)it(i, 4), (int64_t)4 * R * C, it(i, 5) ? 0 : (int64_t)R * C, F, &q);
            edge_ok = inv_frame_ok(R, C, F);
        } else {
            const int Ro = (R + 1) / 2, Co = (C + 1) / 2;
            has = fwd_interior(R, C, Ro, Co, al16(i), (int64_t)4 * Ro * Co, F, &q);
        }
        const FbPlan p = fb_plan(rows(i), cols(i), B, (int)grp.size(), has ? &q : nullptr, edge_ok, fb_specialised(F), mode);
        for (int k = 0; k < p.n; ++k) {
            if (used + 1 + FBP_LW + (int)grp.size() > cap) return -1;
            out[used++] = (int64_t)grp.size();
            put_launch(p.l[k], out + used);
            used += FBP_LW;
            for (int m : grp) out[used++] = m;
            ++launches;
        }
    }
    return launches;
}

#ifdef FBPLAN_MAIN
/* every even filter length to 20, every mode, levels of 1 .. 3 tiles and a bit along each axis
 * (odd and even extents, aligned and not), 1 and 65 items, both directions; each frame decoded */
int main(int argc, char** argv) {
    long cases = 0, launches = 0;
    std::vector<int64_t> out(1 << 16);
    /* argv[1]: the fixture's grid as text, "dir F mode n" then the n items' numbers */
    if (FILE* fh = argc > 1 ? std::fopen(argv[1], "r") : nullptr) {
        int dir, F, mode, n;
        while (std::fscanf(fh, "%d %d %d %d", &dir, &F, &mode, &n) == 4) {
            std::vector<int64_t> items((size_t)n * (dir ? 6 : 4));
            for (int64_t& v : items) {
                long long x;
                if (std::fscanf(fh, "%lld", &x) != 1) return 3;
                v = x;
            }
            const int nl = fbp_level(dir, F, mode, n, items.data(), out.data(), (int)out.size());
            if (nl < 0) return 1;
            launches += nl;
            ++cases;
        }
        std::fclose(fh);
    }
    for (int F = 2; F <= 20; F += 2)
        for (int mode = 0; mode <= 3; ++mode)
            for (int R = 1; R <= 2 * FR * 3 + 9; R += 7)
                for (int C = 1; C <= 2 * FC * 3 + 9; C += 13)
                    for (int n : {1, 65})
                        for (int dir = 0; dir < 2; ++dir) {
                            std::vector<int64_t> items;
                            for (int i = 0; i < n; ++i) {
                                if (dir) items.insert(items.end(), {2, R, C, 2 * R - (R & 1), 2 * C - (C & 1), i & 1});
                                else items.insert(items.end(), {2, 2 * R - (R & 1), 2 * C, 4 * (i % 3 == 2)});
                            }
                            const int nl = fbp_level(dir, F, mode, n, items.data(), out.data(), (int)out.size());
                            if (nl < 0) return 1;
                            int64_t* o = out.data();
                            for (int k = 0; k < nl; ++k) {
                                const int gn = (int)o[0];
                                const int64_t* l = o + 1;
                                if (l[6]) { /* a frame: decode its tiles */
                                    const int tilesC = dir ? fb_tiles(2 * C - (C & 1), IC) : fb_tiles(C, FC);
                                    const int per = (int)(l[1] / 2);
                                    for (int f = 0; f < per; ++f) {
                                        int tr, tc;
                                        frame_tile(f, tilesC, (int)l[2], (int)l[3], (int)l[4], (int)l[5], &tr, &tc);
                                        if (tr < 0 || tc < 0 || tc >= tilesC) return 2;
                                    }
                                }
                                o += 1 + FBP_LW + gn;
                                ++launches;
                            }
                            ++cases;
                        }
    std::printf("fbplan: %ld cases clean (%ld launches)\n", cases, launches);
    return 0;
}
#endif

"""Record the filter bank's host decisions: tests/golden/fb_plan.json.

Which kernel runs which tiles of a level (csrc/filterbank.hip's launchers) is host arithmetic, so it
can be recorded without a GPU: the generator copies a revision's csrc/ and include/, replaces the
four hipLaunchKernelGGL statements of fwd_go, fwd_int_go, inv_go and inv_int_go by a call that
prints the launch, compiles that copy for the host only (hipcc --offload-host-only) with a small
main, and runs the grid of cases() through launch_fwd_levels / launch_inv_levels with pointers that
are never dereferenced.  Per case the fixture keeps fb_tiled_ok, the interior rectangle, the
inverse's edge predicate, fwd_level_fused_ok's two answers and every launch: the *_go it went
through, FT, EDGE, grid, LDS bytes, the rectangle and frame flag of geo, the items and their order,
tiles per item, the five FastDivs and the fused-selection slot shift.  The header keeps the tile
constants and the LDS bytes of every filter length.

The fixture pins what a refactor of the launchers must keep, so it is generated from the sources of
the commit BEFORE the change (one whose filterbank.hip still holds the four launch statements) and
left alone afterwards; tests/test_fb_plan.py replays the grid through csrc/fb_plan.h:

    git worktree add <dir> <commit>
    python tools/gen_golden_fb_plan.py <dir> --commit <commit>
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fb_plan.json")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

FILTERS = list(range(2, 21, 2))  # 14 and 20 are not specialised (FT = 0)
MODES = [0, 1, 2, 3]
# (B, R, C) images: tests/test_gpu_large_levels.py's shapes, then levels with no interior tile
SHAPES = [(1, 130, 1001), (2, 255, 520), (3, 301, 777), (1, 512, 1024), (1, 999, 600), (2, 700, 1100),
          (1, 1031, 515), (1, 800, 1600), (2, 333, 4100), (1, 170, 180), (1, 680, 700), (1, 40, 48), (1, 64, 64)]
CROSSED = [(2, 700, 1100), (1, 40, 48)]  # these meet every filter in every mode


def levels(shape, depth=3):
    """The analysis inputs of `depth` levels of a shape (fb_tiled_ok's size bound applied)."""
    B, R, C = shape
    out = []
    for _ in range(depth):
        if R * C < 512:
            break
        out.append((B, R, C))
        R, C = (R + 1) // 2, (C + 1) // 2
    return out


def inv_win(F):  # the coefficient window of an inverse interior tile (IR = IC = 64)
    H = F // 2
    return 32 + H - (H & 1)


def fwd_item(g, mis=0):
    return [g[0], g[1], g[2], mis]


def inv_item(g, from_p=0):
    """The synthesis level that undoes the analysis of a (B, R, C) image."""
    B, R, C = g
    return [B, (R + 1) // 2, (C + 1) // 2, R, C, from_p]


def cases():
    """[dir, F, mode, fused, items]; dir 0: forward, items [B, R, C, input misalignment in bytes];
    dir 1: inverse, items [B, R, C, outH, outW, a_from_P].  The grid, thinned: the CROSSED shapes
    meet every filter in every mode, every other level meets every filter and every mode along one
    axis, and the special cases below are crossed with the modes."""
    out = []
    item = (fwd_item, inv_item)
    geos = [g for s in SHAPES for g in levels(s)]
    for d in (0, 1):
        for s in CROSSED:
            for F in FILTERS:
                for mode in MODES:
                    out.append([d, F, mode, int(d == 0 and mode >= 2), [item[d](s)]])
        for i, g in enumerate(geos):
            out.append([d, FILTERS[i % len(FILTERS)], 3, 0, [item[d](g)]])
            out.append([d, 16, MODES[i % 4], int(d == 0), [item[d](g)]])
            out.append([d, (4, 8, 18)[i % 3], MODES[(i + 2) % 4], 0, [item[d](g, i & 1)] if d else [item[d](g)]])
    for mode in MODES:
        # al16 = 0: C % 4 != 0, and an aligned pitch behind a pointer off by 4 bytes
        out.append([0, 8, mode, 1, [fwd_item((1, 512, 1022))]])
        out.append([0, 8, mode, 1, [fwd_item((1, 512, 1024), 4)]])
        # haar on whole tiles: every tile is interior, no frame
        out.append([0, 2, mode, 1, [fwd_item((1, 64, 224))]])
        out.append([0, 2, mode, 0, [fwd_item((2, 96, 336))]])
        out.append([1, 2, mode, 0, [inv_item((2, 128, 256))]])
        # both sides of n * tiles == FB_ONE_LAUNCH_TILES: 64 x 128 tiles, one tile row more, and
        # 64 items of 128 and of 144 tiles
        out.append([0, 16, mode, 0, [fwd_item((1, 2048, 14336))]])
        out.append([0, 16, mode, 0, [fwd_item((1, 2050, 14336))]])
        out.append([1, 16, mode, 0, [inv_item((1, 4096, 8192))]])
        out.append([1, 16, mode, 0, [inv_item((1, 4098, 8192))]])
        # 32-bit offsets: the packed image of one item past 2^31 bytes takes the general kernels
        out.append([0, 8, mode, 1, [fwd_item((1, 24000, 24000))]])
        out.append([1, 8, mode, 0, [inv_item((1, 24000, 24000))]])
        # items of one geometry (FB_UNI = 64 a launch) and the fused selection's item cap
        for n in (1, 3, 25, 64, 65):
            if n in (3, 65) or mode == 3:
                out.append([0, 16, mode, int(n < 64), [fwd_item((1, 256, 1792))] * n])
                out.append([1, 8, mode, 0, [inv_item((1, 256, 1792), n & 1)] * n])
        out.append([0, 4, mode, 0, [fwd_item((1, 288, 1792))] * 64])
        # mixed geometries: the grouping order
        mixed = [(1, 170, 180), (2, 700, 1100), (1, 170, 180), (1, 40, 48), (2, 700, 1100), (1, 170, 180)]
        out.append([0, 12, mode, 1, [fwd_item(g, 4 * (i == 2)) for i, g in enumerate(mixed)]])
        out.append([1, 12, mode, 0, [inv_item(g, int(i == 2)) for i, g in enumerate(mixed)]])
    # both sides of the inverse's edge predicate: R or C at inv_win(F) - 1 and inv_win(F)
    for F in FILTERS:
        w = inv_win(F)
        for R, C in ((w - 1, 400), (w, 400), (400, w - 1), (400, w), (w, w)):
            out.append([1, F, 3 - (R + C + F // 2) % 2, 0, [[1, R, C, 2 * R, 2 * C, 0]]])
    # too small for the tiled path: only the predicates are recorded
    out.append([0, 8, 3, 1, [fwd_item((1, 16, 16))]])
    out.append([0, 8, 3, 1, [fwd_item((1, 16, 32))]])
    return out


PRELUDE = r"""
namespace wtp {
template <class G, class S>
static void fbrec(int go, int FT, int EDGE, int grid, size_t lds, const G& g, const S* fs);
}
"""

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include "filterbank.hip"

namespace wtp {
static const uintptr_t BASE_IN = 0x100000000ull, BASE_P = 0x4000000000ull, BASE_A = 0x8000000000ull,
                       BASE_Y = 0xC000000000ull, BASE_S = 0x10000000000ull, STEP = 0x40000000ull;
static bool g_first;
static void dv(const FastDiv& f) { printf(",%u,%u", f.m, f.sh); }
template <class G, class S>
static void fbrec(int go, int FT, int EDGE, int grid, size_t lds, const G& g, const S* fs) {
    printf("%s[%d,%d,%d,%d,%zu,%d,%d,%d,%d,%d,%d,%d", g_first ? "" : ",", go, FT, EDGE, grid, lds, g.geo.tr0,
           g.geo.nTR, g.geo.tc0, g.geo.nTC, g.geo.frame, g.n, g.tiles);
    g_first = false;
    dv(g.dv_tiles); dv(g.dv_per); dv(g.dv_ntc); dv(g.dv_tc); dv(g.dv_side);
    printf(",%d,[", fs ? (int)fs->on : 0);
    for (int m = 0; m < g.n; ++m) {
        uintptr_t p;
        if constexpr (std::is_same<G, FwdGroup>::value) p = reinterpret_cast<uintptr_t>(g.P[m]) - BASE_P;
        else p = reinterpret_cast<uintptr_t>(g.y[m]) - BASE_Y;
        printf("%s%d", m ? "," : "", (int)(p / STEP));
    }
    printf("],[");
    for (int m = 0; fs && fs->on && m < g.n; ++m) {
        uintptr_t p;
        if constexpr (std::is_same<G, FwdGroup>::value) p = reinterpret_cast<uintptr_t>(g.P[m]) - BASE_P;
        else p = 0;
        const uintptr_t base = BASE_S + (p / STEP) * STEP;
        printf("%s%" PRId64, m ? "," : "", (int64_t)((reinterpret_cast<uintptr_t>(fs->slots[m]) - base) / 4));
    }
    printf("]]");
}
}  // namespace wtp

using namespace wtp;

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "consts")) {
        printf("{\"FB_THREADS\":%d,\"FR\":%d,\"FC\":%d,\"IR\":%d,\"IC\":%d,\"FB_UNI\":%d,\"FB_MAX_LDS\":%d,"
               "\"FB_ONE_LAUNCH_TILES\":%d,\"lds\":{", FB_THREADS, FR, FC, IR, IC, FB_UNI, FB_MAX_LDS,
               (int)FB_ONE_LAUNCH_TILES);
        for (int F = 2; F <= 20; F += 2)
            printf("%s\"%d\":[%zu,%zu,%zu,%zu,%zu,%d]", F > 2 ? "," : "", F, fwd_lds(F), fwd_lds(F, true),
                   fwd_int_lds(F), inv_lds(F), inv_lds(F, true), (int)fwd_int_filter(F));
        printf("}}\n");
        return 0;
    }
    int d, F, mode, fused, n;
    while (scanf("%d %d %d %d %d", &d, &F, &mode, &fused, &n) == 5) {
        Taps tp;
        memset(&tp, 0, sizeof tp);
        tp.F = F;
        fb_set_interior(mode);
        g_first = true;
        if (d == 0) {
            std::vector<FwdItem> it(n);
            for (int i = 0; i < n; ++i) {
                long long B, R, C, mis;
                if (scanf("%lld %lld %lld %lld", &B, &R, &C, &mis) != 4) return 2;
                FwdItem& x = it[i];
                x.in = reinterpret_cast<const float*>(BASE_IN + i * STEP + mis);
                x.B = B; x.R = R; x.C = C;
                x.anext = reinterpret_cast<float*>(BASE_A + i * STEP);
                x.P = reinterpret_cast<float*>(BASE_P + i * STEP);
                x.offR = (R + 1) / 2; x.offC = (C + 1) / 2;
                x.PR = 2 * x.offR; x.PC = 2 * x.offC;
                x.last = 0;
                x.fslot = fused ? reinterpret_cast<uint32_t*>(BASE_S + i * STEP) : nullptr;
                x.fhdr = fused ? reinterpret_cast<FslHeader*>(BASE_S + i * STEP + STEP / 2) : nullptr;
            }
            const FwdArgs a = fwd_args(it[0]);
            int q[4] = {0, 0, 0, 0};
            const int has = fwd_interior(a, F, q, q + 1, q + 2, q + 3);
            int64_t s0 = 0, s1 = 0;
            const int ok0 = fwd_level_fused_ok(it[0], tp, &s0, false), ok1 = fwd_level_fused_ok(it[0], tp, &s1, true);
            const int tiled = fb_tiled_ok(it[0].B, it[0].R, it[0].C, tp);
            printf("{\"tiled\":%d,\"int\":[%d,%d,%d,%d,%d],\"edge_ok\":1,\"fused_ok\":[%d,%lld,%d,%lld],\"L\":[", tiled,
                   has, q[0], q[1], q[2], q[3], ok0, (long long)s0, ok1, (long long)s1);
            if (tiled) launch_fwd_levels(it.data(), n, tp, nullptr, fused != 0);
        } else {
            std::vector<InvItem> it(n);
            for (int i = 0; i < n; ++i) {
                long long B, R, C, oh, ow, fp;
                if (scanf("%lld %lld %lld %lld %lld %lld", &B, &R, &C, &oh, &ow, &fp) != 6) return 2;
                InvItem& x = it[i];
                x.a_src = fp ? nullptr : reinterpret_cast<const float*>(BASE_A + i * STEP);
                x.a_bs = R * C; x.lda = C; x.a_from_P = (int)fp;
                x.P = reinterpret_cast<const float*>(BASE_P + i * STEP);
                x.PR = 2 * R; x.PC = 2 * C; x.offR = R; x.offC = C;
                x.B = B; x.R = R; x.C = C;
                x.thr = reinterpret_cast<const float*>(BASE_S) + i;
                x.y = reinterpret_cast<float*>(BASE_Y + i * STEP);
                x.outH = oh; x.outW = ow;
                x.zc = reinterpret_cast<unsigned long long*>(BASE_S + STEP) + i;
            }
            const InvArgs a = inv_args(it[0]);
            int q[4] = {0, 0, 0, 0};
            const int has = inv_interior(a, F, q, q + 1, q + 2, q + 3);
            const int tiled = fb_tiled_ok(it[0].B, it[0].outH, it[0].outW, tp);
            printf("{\"tiled\":%d,\"int\":[%d,%d,%d,%d,%d],\"edge_ok\":%d,\"fused_ok\":[0,0,0,0],\"L\":[", tiled, has,
                   q[0], q[1], q[2], q[3], (int)inv_frame_ok(a, F));
            if (tiled) launch_inv_levels(it.data(), n, tp, nullptr);
        }
        printf("]}\n");
    }
    return 0;
}
"""


def build_recorder(src_root, work):
    """Copy <src_root>'s csrc/ and include/ (layout kept), patch the four launches, compile."""
    csrc = os.path.join(work, "wavelettransforms_amd", "csrc")
    shutil.copytree(os.path.join(src_root, "wavelettransforms_amd", "csrc"), csrc)
    shutil.copytree(os.path.join(src_root, "include"), os.path.join(work, "include"))
    path = os.path.join(csrc, "filterbank.hip")
    with open(path) as fh:
        text = fh.read()
    n = 0
    for go, (kernel, fs) in enumerate([("k_fwd_level<FT>", "(const FwdSel*)nullptr"),
                                       ("(k_fwd_int<FT, EDGE>)", "&fs"),
                                       ("k_inv_level<FT>", "(const FwdSel*)nullptr"),
                                       ("(k_inv_int<FT, EDGE>)", "(const FwdSel*)nullptr")]):
        pat = re.compile(r"hipLaunchKernelGGL\(" + re.escape(kernel) +
                         r", dim3\(grid\), dim3\(FB_THREADS\), (.+?), s, g, [^;]*\);")
        edge = "EDGE" if "EDGE" in kernel else "0"
        text, k = pat.subn(lambda m: "fbrec(%d, FT, %s, grid, %s, g, %s);" % (go, edge, m.group(1), fs), text)
        n += k
    if n != 4 or "hipLaunchKernelGGL" in text:
        sys.exit("expected the four launch statements of fwd_go, fwd_int_go, inv_go and inv_int_go in " + path)
    text = text.replace("#pragma clang fp contract(off)", PRELUDE + "#pragma clang fp contract(off)", 1)
    with open(path, "w") as fh:
        fh.write(text)
    main = os.path.join(csrc, "fbrec_main.hip")
    with open(main, "w") as fh:
        fh.write(MAIN)
    exe = os.path.join(work, "fbrec")
    subprocess.check_call([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-Wno-unused-function", "-I" + csrc,
                           "-I" + os.path.join(work, "include"), "-o", exe, main])
    return exe


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src", help="a checkout of the commit to record (holds wavelettransforms_amd/csrc and include)")
    ap.add_argument("--commit", required=True, help="hash of that commit")
    a = ap.parse_args()
    if len(a.commit) != 40:
        sys.exit("--commit takes the full 40-character hash")
    cs = cases()
    with tempfile.TemporaryDirectory() as work:
        exe = build_recorder(os.path.abspath(a.src), work)
        consts = json.loads(subprocess.check_output([exe, "consts"], text=True))
        feed = "".join("%d %d %d %d %d\n%s\n" % (c[0], c[1], c[2], c[3], len(c[4]),
                                                  "\n".join(" ".join(map(str, it)) for it in c[4])) for c in cs)
        lines = subprocess.check_output([exe], input=feed, text=True).splitlines()
    if len(lines) != len(cs):
        sys.exit("%d records for %d cases" % (len(lines), len(cs)))
    dump = lambda x: json.dumps(x, separators=(",", ":"))
    rows = []
    for c, line in zip(cs, lines):
        r = json.loads(line)
        rows.append(dump([c, r["tiled"], r["int"], r["edge_ok"], r["fused_ok"], r["L"]]))
    with open(OUT, "w") as fh:
        fh.write('{"commit":%s,\n"consts":%s,\n"cases":[\n%s\n]}\n' % (dump(a.commit), dump(consts), ",\n".join(rows)))
    print("%s: %d cases, %d launches, %d bytes" % (OUT, len(cs), sum(len(json.loads(l)["L"]) for l in lines),
                                                   os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

"""The filter bank's host decisions (csrc/fb_plan.h, compiled for the host by tests/native/fbplan.cpp)
against tests/golden/fb_plan.json, the record tools/gen_golden_fb_plan.py made from the launchers of
the commit named in the fixture: for every case fb_tiled_ok, the interior rectangle, the inverse's
edge predicate, fwd_level_fused_ok's answer and slot count, and every launch -- which kernel, FT,
EDGE, grid, LDS bytes, the rectangle and frame flag, items and their order, tiles per item, the
FastDivs and the fused selection's slot shift.  Exact equality on every field the launched kernel
reads: k_*_int decode a tile by dv_tiles, dv_per and dv_ntc, their EDGE forms by dv_tiles, dv_per,
dv_tc and dv_side; the general kernels divide and read no dv_* field, so those are not compared
there (the recorded launchers left them zero or stale, the plan fills them).  CPU only."""
import ctypes
import importlib.util
import json
import os

import pytest

from tests.fbplan_shim import (EDGE, FIXTURE, FSL_WORDS, GENERAL, INTERIOR, ROOT, SEG_PER_LAUNCH, consts, level,
                               load_shim, per_filter)


@pytest.fixture(scope="module")
def fb():
    return load_shim()


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_golden_fb_plan", os.path.join(ROOT, "tools", "gen_golden_fb_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_covers_the_generators_grid(gen, fixture):
    """The committed record is the generator's grid, case for case, and the grid holds what it must."""
    cases = gen.cases()
    assert [c[0] for c in fixture["cases"]] == cases and len(cases) > 400
    assert len(fixture["commit"]) == 40
    assert os.path.getsize(FIXTURE) < 256 << 10
    assert {c[1] for c in cases} == set(range(2, 21, 2)) and {c[2] for c in cases} == {0, 1, 2, 3}
    assert {len(c[4]) for c in cases} >= {1, 3, 64, 65}
    assert {c[3] for c in cases} == {0, 1} and {c[0] for c in cases} == {0, 1}
    launches = [l for c in fixture["cases"] for l in c[5]]
    assert {(l[0], l[2]) for l in launches} == {(0, 0), (1, 0), (1, 1), (2, 0), (3, 0), (3, 1)}  # every *_go, both forms
    assert any(l[9] and l[0] in (0, 2) for l in launches) and any(l[9] and l[2] for l in launches)  # both frames
    assert any(l[22] and l[24] and l[24][0] for l in launches)  # a shifted fused slot
    one = fixture["consts"]["FB_ONE_LAUNCH_TILES"]
    assert any(l[3] == one and l[2] == 1 for l in launches) and any(l[3] > one for l in launches)
    assert {c[3] for c in fixture["cases"] if c[0][0] == 1} == {0, 1}  # both sides of the inverse's edge predicate
    assert any(not c[1] for c in fixture["cases"]) and any(not c[2][0] for c in fixture["cases"])


def test_constants_and_lds_match_the_record(fb, fixture):
    """Tile sizes, the specialised lengths and every kernel's dynamic LDS: LDS bytes set the occupancy."""
    c, want = consts(fb), fixture["consts"]
    for k in ("FB_THREADS", "FR", "FC", "IR", "IC", "FB_UNI", "FB_MAX_LDS", "FB_ONE_LAUNCH_TILES"):
        assert c[k] == want[k], k
    for F in range(2, 21, 2):
        f = per_filter(fb, F)
        got = [f["fwd_lds"], f["fwd_lds_alias"], f["fwd_int_lds"], f["inv_lds"], f["inv_lds_alias"], f["spec"]]
        assert got == want["lds"][str(F)], F
        assert (F in c["spec"]) == bool(f["spec"])
        assert max(got[:5]) <= c["FB_MAX_LDS"]
        # the aliased forward bytes are taken at the largest first column: never below k_fwd_int's exact ones
        assert f["fwd_lds_alias"] >= f["fwd_int_lds"] and f["tp"] % 4 == 0 and 0 <= f["s0"] < 4
        assert f["lhh"] % 16 == 8 and 2 * f["lhh"] >= 2 * c["FC"] + F - 2


def test_plan_matches_the_record(fb, fixture):
    c = consts(fb)
    waves = c["FB_THREADS"] // 64
    bad, n_launch = [], 0
    for case in fixture["cases"]:
        (d, F, mode, fused, items), tiled, interior, edge_ok, fused_ok, want = case
        f = per_filter(fb, F)
        B, R, C = items[0][:3]
        q = (ctypes.c_int * 4)()
        if d == 0:
            Ro, Co = (R + 1) // 2, (C + 1) // 2
            got_tiled = fb.fbp_tiled_ok(B, R, C, F)
            has = fb.fbp_fwd_interior(R, C, int(items[0][3] % 16 == 0 and C % 4 == 0), 4 * Ro * Co, F, q)
            got_edge = 1
            tilesR, tilesC = -(-Ro // c["FR"]), -(-Co // c["FC"])
        else:
            oh, ow, from_p = items[0][3:]
            got_tiled = fb.fbp_tiled_ok(B, oh, ow, F)
            has = fb.fbp_inv_interior(R, C, oh, ow, 4 * R * C, 0 if from_p else R * C, F, q)
            got_edge = fb.fbp_inv_frame_ok(R, C, F)
            tilesR, tilesC = -(-oh // c["IR"]), -(-ow // c["IC"])
        rect = list(q) if has else interior[1:]  # without an interior the rectangle is not defined
        if [got_tiled, [has] + rect, got_edge] != [tiled, interior, edge_ok]:
            bad.append((case[0], "predicates", [got_tiled, [has] + rect, got_edge]))
        if d == 0:
            # fwd_level_fused_ok: interior mode 2 or 3 (any_mode: as if 3), and no launch of the
            # first item's own plan in the general kernel; the slots are one per wave of every tile
            got = []
            for m in (mode, 3):
                p = level(fb, 0, F, m, items[:1])
                ok = int(bool(got_tiled) and m >= 2 and all(l[0] != GENERAL for _, l, _ in p))
                got += [ok, ok * waves * sum(l[1] for _, l, _ in p)]
                assert sum(l[1] for _, l, _ in p) == tilesR * tilesC * B
            if got != fused_ok:
                bad.append((case[0], "fused_ok", got))
        if not tiled:
            assert want == []
            continue
        got = level(fb, d, F, mode, items)
        if len(got) != len(want):
            bad.append((case[0], "launches", len(got)))
            continue
        for (n, l, order), w in zip(got, want):
            n_launch += 1
            kind, tiles, r0, nr, c0, nc, frame, before = l[:8]
            dv = {k: l[8 + 2 * i:10 + 2 * i] for i, k in enumerate(["tiles", "per", "ntc", "tc", "side"])}
            wdv = {k: w[12 + 2 * i:14 + 2 * i] for i, k in enumerate(["tiles", "per", "ntc", "tc", "side"])}
            ft = F if f["spec"] else 0
            go = 2 * d + (kind != GENERAL)
            lds = [f["fwd_lds_alias"] if ft else f["fwd_lds"], f["fwd_int_lds"],
                   f["inv_lds_alias"] if ft else f["inv_lds"], f["inv_lds_alias"]][go]
            assert lds <= c["FB_MAX_LDS"]
            on = int(bool(fused) and kind != GENERAL and n <= SEG_PER_LAUNCH)
            rec = [go, ft, int(kind == EDGE), n * tiles, lds, r0, nr, c0, nc, frame, n, tiles]
            read = {GENERAL: [], INTERIOR: ["tiles", "per", "ntc"], EDGE: ["tiles", "per", "tc", "side"]}[kind]
            shift = [before * waves * FSL_WORDS] * n if on else []
            if (rec != w[:12] or any(dv[k] != wdv[k] for k in read) or on != w[22] or order != w[23] or shift != w[24]):
                bad.append((case[0], "launch", rec, dv, on, order, shift, w))
        # together the launches run every tile of every item
        assert sum(l[1] * n for n, l, _ in got) == sum(-(-((it[1] + 1) // 2) // c["FR"]) * -(-((it[2] + 1) // 2) // c["FC"]) * it[0]
                                                      if d == 0 else -(-it[3] // c["IR"]) * -(-it[4] // c["IC"]) * it[0]
                                                      for it in items), case[0]
    assert n_launch > 500
    assert not bad, "%d records differ; first: %r" % (len(bad), bad[:3])


def test_every_plan_runs_every_tile_once(fb, fixture):
    """A rectangle plus its frame, decoded as the kernels decode them (frame_tile and the plan's
    FastDivs), lists every tile of every image once: over the fixture's grids in every mode, and
    over every rectangle of small grids."""
    c = consts(fb)
    seen = set()
    for case in fixture["cases"]:
        (d, F, mode, _, items), _, interior, edge_ok = case[:4]
        B, R, C = items[0][:3]
        if d == 0:
            tr, tc = -(-((R + 1) // 2) // c["FR"]), -(-((C + 1) // 2) // c["FC"])
        else:
            tr, tc = -(-items[0][3] // c["IR"]), -(-items[0][4] // c["IC"])
        key = (tr, tc, B, tuple(interior), edge_ok)
        if key in seen or tr * tc * B > 20000:
            continue
        seen.add(key)
        rect = (ctypes.c_int * 4)(*interior[1:]) if interior[0] else None
        for m in range(4):
            for n in (1, 40):
                assert fb.fbp_cover(tr, tc, B, n, rect, edge_ok, 1, m) == 0, (key, m, n)
    assert len(seen) > 40
    for tr in range(1, 6):
        for tc in range(1, 6):
            for r0 in range(tr):
                for nr in range(1, tr - r0 + 1):
                    for c0 in range(tc):
                        for nc in range(1, tc - c0 + 1):
                            rect = (ctypes.c_int * 4)(r0, nr, c0, nc)
                            for m in range(4):
                                for edge in (0, 1):
                                    assert fb.fbp_cover(tr, tc, 3, 2, rect, edge, 1, m) == 0, (tr, tc, r0, nr, c0, nc, m, edge)

"""CPU check of the extension modes' shared core (csrc/wt_modes_core.h, compiled into the
stand-alone program tests/native/modescore.cpp) against PyWavelets goldens
(tools/gen_golden_modes.py): one level of dwt / idwt of a line bit for bit, the packed geometry,
the whole wavedec2 -> threshold -> waverec2 -> crop of the golden cases level by level, and the
tiny-image kernels' per-image routines (wtm_tiny_fwd / wtm_tiny_inv in a wave's arena, record 5)
word for word against that per-level path."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.modes_ref import MODE_ID, MODES, build as _build, lanes_log2, run as _run
from wavelettransforms_amd import workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "modes_manifest.json")) as fh:
        man = json.load(fh)
    return man, np.load(os.path.join(HERE, "golden", "modes_cases.npz"))


def _i(*v):
    return np.array(v, np.int32)


def _kat_records(man):
    words, keys = [], sorted(man["kat"])
    for key in keys:
        k = man["kat"][key]
        taps = O.filters(k["wavelet"])
        x = W.synth_numpy((k["n"],), *k["synth"])
        words += [_i(1, MODE_ID[k["mode"]], taps.shape[1], k["n"]), taps, x]
    return words, keys


def _check_kat(out, man, arrs, keys):
    pos = 0
    for key in keys:
        a, d, y = arrs[key + "/a"], arrs[key + "/d"], arrs[key + "/y"]
        m = int(out[pos])
        assert m == a.size == d.size, key
        assert np.array_equal(out[pos + 1:pos + 1 + m], a.view(np.uint32)), key
        assert np.array_equal(out[pos + 1 + m:pos + 1 + 2 * m], d.view(np.uint32)), key
        pos += 1 + 2 * m
        n = int(out[pos])
        assert n == y.size, key
        assert np.array_equal(out[pos + 1:pos + 1 + n], y.view(np.uint32)), key
        pos += 1 + n
    assert pos == out.size


def test_fixture_covers_the_grid(golden):
    man, _ = golden
    want = {"kat/%s/%s/%d" % (m, w, n) for m in MODES for w in ("haar", "db2", "bior3.3", "rbio2.2", "db8")
            for n in (1, 2, 3, 4, 5, 7, 8, 9, 16, 33)}
    # pywt 1.1.1 does not return from reflect of a one-sample line: no golden exists
    want -= {"kat/reflect/%s/1" % w for w in ("haar", "db2", "bior3.3", "rbio2.2", "db8")}
    assert set(man["kat"]) == want


def test_line_dwt_idwt_bit_equal(golden):
    man, arrs = golden
    words, keys = _kat_records(man)
    _check_kat(_run(_build("modescore", ["-O2"]), words, "kat"), man, arrs, keys)


def _geom_records(man):
    words = []
    for g in man["geom"]:
        words.append(_i(2, MODE_ID[g["mode"]], O.dec_len(g["wavelet"]), g["shape"][0], g["shape"][1], g["level"]))
    return words


def _check_geom(out, man):
    out = out.view(np.int32)
    pos = 0
    seen = set()
    for g in man["geom"]:
        L = g["level"]
        R, C = out[pos:pos + L + 1], out[pos + L + 1:pos + 2 * L + 2]
        PR, PC, oH, oW = out[pos + 2 * L + 2:pos + 2 * L + 6]
        pos += 2 * L + 6
        # pywt's list: cA_L, then the details of level L .. 1
        want = [g["shape"]] + g["levels"][1:][::-1] if L else [g["shape"]]
        assert [[int(r), int(c)] for r, c in zip(R, C)] == want, g
        if L:
            assert g["levels"][0] == [int(R[L]), int(C[L])], g
        assert [int(PR), int(PC)] == g["packed_shape"], g
        assert [int(oH), int(oW)] == g["rec_shape"], g
        seen.add((tuple(g["shape"]), L))
    assert pos == out.size
    assert seen >= {(s, L) for s in ((3, 3), (7, 7), (5, 8), (10, 128), (96, 100)) for L in range(4)}


def test_geometry_matches_coeffs_to_array(golden):
    man, _ = golden
    _check_geom(_run(_build("modescore", ["-O2"]), _geom_records(man), "geom"), man)


def _canon_hash(a):
    a = np.array(a, dtype=np.float32, copy=True).reshape(-1)
    a[a == 0] = 0
    return hashlib.sha256(a.tobytes()).hexdigest()


def _image_records(man, names, nl=None):
    """record 3 of every transformed tensor of the named cases; with nl (a function of H, W, L, F
    giving the lane stride, or None for a tensor that is not a tiny one): record 5 of the tiny ones"""
    words, metas = [], []
    for name in names:
        c = man["cases"][name]
        taps = O.filters(c["wavelet"])
        for ti, t in enumerate(c["tensors"]):
            if len(t["shape"]) < 2 or t["eff_level"] == 0:
                continue
            H, Wd = t["shape"][-2:]
            B = int(np.prod(t["shape"][:-2], dtype=np.int64))
            head = (MODE_ID[c["mode"]], taps.shape[1], B, H, Wd, t["eff_level"])
            if nl is not None:
                stride = nl(H, Wd, t["eff_level"], taps.shape[1])
                if stride is None:
                    continue
                head = (5,) + head + (stride,)
            else:
                head = (3,) + head
            x = W.synth_numpy(tuple(t["shape"]), *t["synth"])
            words += [_i(*head), np.array([t["thr32_bits"]], np.uint32), taps, x]
            metas.append((name, ti, t, B, H, Wd))
    return words, metas


def _check_images(out, arrs, metas):
    pos = 0
    for name, ti, t, B, H, Wd in metas:
        PR, PC = int(out[pos]), int(out[pos + 1])
        assert [PR, PC] == t["packed_shape"][-2:], name
        n = B * PR * PC
        assert n == t["coeff_numel"], name
        packed = out[pos + 2:pos + 2 + n].view(np.float32)
        assert _canon_hash(packed) == t["packed_hash"], name
        res = out[pos + 2 + n:pos + 2 + n + B * H * Wd].view(np.float32).reshape(t["shape"])
        ref = arrs["case/%s/%d/out" % (name, ti)]
        assert _canon_hash(res) == t["out_hash"] and np.array_equal(res, ref), name
        assert int((res == 0).sum()) == t["zero_count"], name
        pos += 2 + n + B * H * Wd
    assert pos == out.size


def test_whole_transform_of_the_golden_cases(golden):
    """wavedec2 + coeffs_to_array, the float32 compare against the golden threshold, waverec2 with
    its inter-level crop and the final crop, from the shared header's points and geometry alone"""
    man, arrs = golden
    words, metas = _image_records(man, sorted(man["cases"]))
    assert len(metas) >= 40
    _check_images(_run(_build("modescore", ["-O2"]), words, "img"), arrs, metas)


# ---- the tiny-image routines (record 5) ----
TINY_THR = np.float32(0.5)  # of standard normal samples: most cases have coefficients on both sides of it


def _levels_ok(n, L, F, mode):
    """wtm_levels_ok along one axis: reflect cannot extend a one-sample line"""
    for _ in range(L):
        if mode == "reflect" and n == 1:
            return False
        n = (n + F - 1) // 2
    return True


def _tiny_sweep():
    """every (mode, wavelet, H, W, L) of the sweep that the modes can transform"""
    return [(m, w, h, wd, L) for m in MODES for w in ("haar", "db2") for L in range(1, 5)
            for h in range(1, 9) for wd in range(1, 9)
            if _levels_ok(h, L, O.dec_len(w), m) and _levels_ok(wd, L, O.dec_len(w), m)]


def _tiny_words(sweep, kind, nl=None, B=5):
    rng = np.random.default_rng(20)
    words = []
    for m, w, h, wd, L in sweep:
        taps = O.filters(w)
        x = rng.standard_normal((B, h, wd)).astype(np.float32)
        head = (kind, MODE_ID[m], taps.shape[1], B, h, wd, L) + (() if nl is None else (nl,))
        words += [_i(*head), np.array([TINY_THR], np.float32), taps, x]
    return words


@pytest.fixture(scope="module")
def tiny_sweep():
    """the sweep and record 3 (the per-level path the PyWavelets goldens anchor) over it, once"""
    sweep = _tiny_sweep()
    return sweep, _run(_build("modescore", ["-O2"]), _tiny_words(sweep, 3), "tiny_ref")


def test_tiny_sweep_is_the_one_asked_for(tiny_sweep):
    """Of 5 modes x 2 wavelets x 4 levels x 64 shapes = 2560, reflect loses the shapes that meet a
    one-sample line: under haar (n -> ceil(n / 2)) a side needs n >= 2, 3, 5 at levels 1, 2, 3 and
    none reaches level 4, 49 + 36 + 16 shapes; under db2 (n -> (n + 3) // 2 >= 2) only n = 1 fails,
    49 shapes a level.  2048 + 101 + 196 = 2345, and every one is a tiny tensor (record 4)."""
    sweep, _ = tiny_sweep
    assert len(sweep) == len(set(sweep)) == 2345
    lanes = _run(_build("modescore", ["-O2"]), [_i(4, h, wd, L, O.dec_len(w)) for _, w, h, wd, L in sweep], "tiny_lanes")
    assert lanes.size == len(sweep) and (lanes.view(np.int32) >= 0).all()
    have = set(sweep)
    for m in MODES:
        for w in ("haar", "db2"):
            for shape in ((1, 1), (1, 8), (8, 1), (2, 3), (3, 3), (7, 7), (8, 8)):
                ok = [L for L in range(1, 5) if all(_levels_ok(n, L, O.dec_len(w), m) for n in shape)]
                assert (m != "reflect") <= (len(ok) == 4), (m, w, shape)
                if shape == (1, 1):
                    assert bool(ok) == (m != "reflect")
                if ok:
                    assert (m, w) + shape + (max(ok),) in have
            assert (m, w, 8, 8, 4) in have or (m, w) == ("reflect", "haar")


@pytest.mark.parametrize("nl", [1, 4])
def test_tiny_routines_equal_the_per_level_path(tiny_sweep, nl):
    """wtm_tiny_fwd / wtm_tiny_inv in an arena of lane stride nl (B = 5: a partial last group), the
    packed images and the outputs word for word those of record 3"""
    sweep, ref = tiny_sweep
    out = _run(_build("modescore", ["-O2"]), _tiny_words(sweep, 5, nl), "tiny_nl%d" % nl)
    assert out.size == ref.size
    pos = both = 0
    bad = []
    for m, w, h, wd, L in sweep:
        n = 2 + 5 * int(ref[pos]) * int(ref[pos + 1]) + 5 * h * wd
        if not np.array_equal(out[pos:pos + n], ref[pos:pos + n]):
            bad.append((m, w, h, wd, L))
        packed = ref[pos + 2:pos + n - 5 * h * wd].view(np.float32)
        both += bool((np.abs(packed) >= TINY_THR).any() and (np.abs(packed[packed != 0]) < TINY_THR).any())
        pos += n
    assert pos == ref.size
    assert both > len(sweep) // 2, "the threshold cuts through the coefficients of most geometries"
    assert not bad, "%d of %d geometries differ, first %s" % (len(bad), len(sweep), bad[:5])


def test_tiny_geometry_equals_wtm_geom(tiny_sweep):
    """wtm_tiny_geometry (R, C, offR, offC, PR, PC in small ints) against wtm_geom, and the C
    wtm_levels_ok against this file's restatement of it, over the sweep and the shapes it left out"""
    sweep, _ = tiny_sweep
    have = set(sweep)
    every = [(m, w, h, wd, L) for m in MODES for w in ("haar", "db2") for L in range(1, 5)
             for h in range(1, 9) for wd in range(1, 9)]
    out = _run(_build("modescore", ["-O2"]), [_i(6, MODE_ID[m], O.dec_len(w), h, wd, L) for m, w, h, wd, L in every],
               "tiny_geom").view(np.int32)
    pos = 0
    for key in every:
        n = 4 * key[4] + 4
        assert bool(out[pos]) == (key in have), key
        assert np.array_equal(out[pos + 1:pos + 1 + n], out[pos + 1 + n:pos + 1 + 2 * n]), key
        pos += 1 + 2 * n
    assert pos == out.size and len(every) == 2560


def _tiny_stride(H, Wd, L, F):
    """the lane stride the planner gives a tiny tensor (record 4), None for any other"""
    if H > 8 or Wd > 8 or F > 4 or not 1 <= L <= 4:
        return None
    return 1 << lanes_log2(H, Wd, L, F)


def _tiny_golden(man):
    return _image_records(man, sorted(man["cases"]), nl=_tiny_stride)


def test_tiny_routines_on_the_golden_cases(golden):
    """the tiny-eligible tensors of the PyWavelets cases (the c3x3 and c7x7 families, every mode)
    through record 5 at the planner's lane stride: packed_hash, out_hash, out and zero_count"""
    man, arrs = golden
    words, metas = _tiny_golden(man)
    assert {m[0] for m in metas} >= {"%s/%s" % (f, m) for f in ("c3x3", "c7x7") for m in MODES}
    _check_images(_run(_build("modescore", ["-O2"]), words, "tiny_img"), arrs, metas)


def test_core_asan_ubsan(golden):
    """the same program under AddressSanitizer and UBSan, once: every line record, every geometry
    record, the small image cases, and the tiny-image routines (record 5, whose arena is exactly the
    words the area functions report) on the golden tiny cases and over the sweep at lane stride 4"""
    man, arrs = golden
    exe = _build("modescore_san", SAN)
    kw, keys = _kat_records(man)
    small = [n for n in sorted(man["cases"]) if n.split("/")[0] in ("c3x3", "c7x7", "c9x9", "mixed", "c33x17")]
    iw, metas = _image_records(man, small)
    out = _run(exe, kw, "san_kat")
    _check_kat(out, man, arrs, keys)
    _check_geom(_run(exe, _geom_records(man), "san_geom"), man)
    _check_images(_run(exe, iw, "san_img"), arrs, metas)
    tw, tmetas = _tiny_golden(man)
    _check_images(_run(exe, tw, "san_tiny_img"), arrs, tmetas)
    sweep = _tiny_sweep()
    assert np.array_equal(_run(exe, _tiny_words(sweep, 5, 4), "san_tiny"), _run(exe, _tiny_words(sweep, 3), "san_tiny_ref"))

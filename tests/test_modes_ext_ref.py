"""CPU checks of the extension modes' reference chain (tests/modes_ref.py) and of the fixture it
generates (tools/gen_golden_modes_ext.py -> tests/golden/modes_ext_*):
  (a) the chain reproduces every transformed tensor of the PyWavelets goldens (modes_manifest.json)
      bit for bit -- the anchor of everything tests/test_gpu_modes_ext.py compares against;
  (b) the generator, run in memory, gives the committed fixture;
  (c) the fixture holds the cases it was written for: tiny tensors over several waves, thresholds
      on and just past the zero plateau, long filters, lines shorter than the filter."""
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import golden_io as G
from tests import modes_ref as R
from wavelettransforms_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = R.MODES


def _load(stem):
    with open(os.path.join(G.GOLDEN, stem + "_manifest.json")) as fh:
        return json.load(fh), np.load(os.path.join(G.GOLDEN, stem + "_cases.npz"))


@pytest.fixture(scope="module")
def ext():
    return _load("modes_ext")


def test_chain_reproduces_the_pywt_goldens():
    man, arrs = _load("modes")
    seen = 0
    for name in sorted(man["cases"]):
        c = man["cases"][name]
        lvl = c["level"]
        for ti, t in enumerate(c["tensors"]):
            if len(t["shape"]) < 2:
                continue
            x = W.synth_numpy(tuple(t["shape"]), *t["synth"])
            packed, thr64, thr32, max_abs, out, eff = R.chain(x, c["wavelet"], lvl, c["mode"], c["pct"])
            lvl = eff  # a list case carries the clamped level on
            tag = (name, ti)
            assert eff == t["eff_level"], tag
            if eff == 0:
                continue
            seen += 1
            assert list(packed.shape) == t["packed_shape"] and packed.size == t["coeff_numel"], tag
            assert G.canon_hash(packed) == t["packed_hash"], tag
            assert float(thr64).hex() == t["thr64_hex"], tag
            assert G.f32_bits(thr32) == t["thr32_bits"] and G.f32_bits(max_abs) == t["max_abs_bits"], tag
            assert G.mask_hash(np.abs(packed) < thr32) == t["mask_hash"], tag
            ref = arrs["case/%s/%d/out" % (name, ti)]
            assert out.dtype == ref.dtype and np.array_equal(out, ref) and G.canon_hash(out) == t["out_hash"], tag
            assert int((out == 0).sum()) == t["zero_count"], tag
    assert seen == 55


def test_generator_gives_the_committed_fixture(ext):
    man, arrs = ext
    spec = importlib.util.spec_from_file_location("gen_golden_modes_ext",
                                                  os.path.join(ROOT, "tools", "gen_golden_modes_ext.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    man2, arrs2 = gen.generate()
    assert json.loads(json.dumps(man2, sort_keys=True)) == man
    assert sorted(arrs2) == sorted(arrs.files)
    for k in arrs.files:
        assert arrs2[k].dtype == arrs[k].dtype and arrs2[k].shape == arrs[k].shape, k
        assert arrs2[k].tobytes() == arrs[k].tobytes(), k
    size = sum(os.path.getsize(os.path.join(G.GOLDEN, f)) for f in ("modes_ext_manifest.json", "modes_ext_cases.npz"))
    assert size < 1000000


def _group(man, group):
    return {n: c for n, c in man["cases"].items() if c["group"] == group}


def test_tiny_cases_span_several_waves(ext):
    man, arrs = ext
    tiny = _group(man, "tiny")
    assert sorted(tiny) == sorted("%s/%s" % (n, m) for n in ("tiny_haar", "tiny_db2") for m in MODES)
    for mode in MODES:
        h, d = tiny["tiny_haar/" + mode]["tensors"], tiny["tiny_db2/" + mode]["tensors"]
        assert [(t["shape"], t["eff_level"]) for t in h] == [([70, 3, 3, 3], 1), ([9, 5, 7, 7], 2), ([5, 13, 8, 6], 2),
                                                             ([2, 2, 9, 9], 2), ([4, 4, 1, 5], 0)]
        assert [(t["shape"], t["eff_level"]) for t in d] == [([11, 7, 8, 8], 1), ([3, 43, 6, 8], 1), ([4, 3, 3, 3], 0)]
        assert h[0]["lanes_log2"] == 6 and h[0]["waves"] == [64, 64, 64, 18]
        assert h[1]["lanes_log2"] == 5 and h[1]["waves"] == [32, 13]
        assert d[0]["lanes_log2"] == 5 and d[0]["waves"] == [32, 32, 13]
        assert "lanes_log2" not in h[3] and "lanes_log2" not in h[4] and "lanes_log2" not in d[2]
        # a multi-wave segment with tiny segments after it (the wave_begin search), per-level kernels between
        assert len(h[0]["waves"]) > 1 and "waves" in h[2] and len(d[0]["waves"]) > 1 and "waves" in d[1]
    recs = [t for c in tiny.values() for t in c["tensors"] if "waves" in t]
    for t in recs:
        B, nl = int(np.prod(t["shape"][:-2])), 1 << t["lanes_log2"]
        assert sum(t["waves"]) == B and all(w == nl for w in t["waves"][:-1]) and 0 < t["waves"][-1] <= nl
    for c in (tiny["tiny_haar/zero"], tiny["tiny_db2/zero"]):  # the rule itself, from the shared header
        for t in c["tensors"]:
            lg = R.lanes_log2(t["shape"][-2], t["shape"][-1], t["eff_level"], O.dec_len(c["wavelet"]))
            assert lg == t.get("lanes_log2", -1), t["shape"]
    assert any(len(t["waves"]) >= 3 for t in recs)
    assert any(len(t["waves"]) >= 2 and t["waves"][-1] < t["waves"][0] for t in recs)  # B % NL != 0 after a full wave
    assert {t["lanes_log2"] for t in recs} == {5, 6}
    for name in ("tiny_haar", "tiny_db2"):  # the same input in every mode: the zero counts tell the modes apart
        for ts, tz in zip(tiny[name + "/symmetric"]["tensors"], tiny[name + "/zero"]["tensors"]):
            assert ts["synth"] == tz["synth"]
            if "waves" in ts:
                assert ts["zero_count"] != tz["zero_count"], (name, ts["shape"])
    for n, c in tiny.items():
        for ti in range(len(c["tensors"])):
            assert "case/%s/%d/out" % (n, ti) in arrs.files


def test_launch_group_case(ext):
    man, _ = ext
    grp = _group(man, "group")
    assert sorted(grp) == ["group_haar/periodic", "group_haar/symmetric"]
    for c in grp.values():
        ts = c["tensors"]
        assert len(ts) > 24  # SEG_PER_LAUNCH
        assert len(ts[24]["waves"]) >= 3 and ts[24]["waves"][-1] < ts[24]["waves"][0]
        assert any("waves" in t for t in ts[:24]) and sum("waves" in t for t in ts[25:]) >= 2
        assert any("waves" not in t and t["eff_level"] > 0 for t in ts[25:])


def test_percentile_cases_sit_on_the_plateau(ext):
    man, _ = ext
    pct = _group(man, "pct")
    below = 0
    for name, shape, wavelet, level in (("p96x100", [96, 100], "bior3.3", 3), ("p3x3", [70, 3, 3, 3], "haar", 1),
                                        ("p8x6", [5, 13, 8, 6], "haar", 2)):
        flat = 0
        for mode in MODES:
            cs = [pct[k] for k in sorted(pct) if k.startswith("%s/%s/" % (name, mode))]
            t0 = cs[0]["tensors"][0]
            z, n = t0["zeros_packed"], t0["coeff_numel"]
            assert t0["shape"] == shape and t0["eff_level"] == level and cs[0]["wavelet"] == wavelet
            want = {0.0, 5.0, 50.0, 99.9, 100.0} | ({100.0 * (z - 1) / (n - 1), 100.0 * (z - 0.5) / (n - 1)} if z else set())
            assert {c["pct"] for c in cs} == want, (name, mode)
            for c in cs:
                t = c["tensors"][0]
                thr64, thr32 = float.fromhex(t["thr64_hex"]), np.array(t["thr32_bits"], np.uint32).view(np.float32)[()]
                small = np.array(t["min_nonzero_bits"], np.uint32).view(np.float32)[()]
                if thr64 == 0.0:
                    assert t["out_hash"] == t["rt_hash"], (name, mode, c["pct"])
                    flat += 1
                if z and c["pct"] == 100.0 * (z - 1) / (n - 1):
                    assert thr64 == 0.0, (name, mode)
                if z and c["pct"] == 100.0 * (z - 0.5) / (n - 1):
                    assert 0 < thr32 < small and t["out_hash"] == t["rt_hash"], (name, mode)
                    below += 1
                if c["pct"] == 100.0:
                    assert thr32 == np.array(t["max_abs_bits"], np.uint32).view(np.float32)[()]
                    assert 2 * t["zero_count"] > int(np.prod(shape)), (name, mode)
        assert flat >= 1, name
    assert below >= 1
    zero = pct["p96x100/zero/0"]["tensors"][0]
    assert (zero["zeros_packed"], zero["coeff_numel"]) == (2573, 13804)
    assert pct["p3x3/symmetric/0"]["tensors"][0]["zeros_packed"] == 1470


def test_long_filter_and_component_cases(ext):
    man, arrs = ext
    want = {"db8_30x33": ("db8", 16, 1, [2, 3, 30, 33]), "db8_64x70": ("db8", 16, 2, [2, 2, 64, 70]),
            "bior33_14x17": ("bior3.3", 8, 1, [2, 2, 14, 17]), "sym3_12x10": ("sym3", 6, 1, [2, 5, 12, 10]),
            "coif1_10x12": ("coif1", 6, 1, [2, 2, 10, 12]), "bior13_10x11": ("bior1.3", 6, 1, [2, 2, 10, 11]),
            "dmey_124x130": ("dmey", 62, 1, [1, 2, 124, 130])}
    lng = _group(man, "long")
    assert sorted(lng) == sorted("%s/%s" % (n, m) for n in want for m in MODES)
    for n, c in lng.items():
        wavelet, F, level, shape = want[n.split("/")[0]]
        t = c["tensors"][0]
        assert (c["wavelet"], t["eff_level"], t["shape"]) == (wavelet, level, shape) and "waves" not in t
        assert O.filters(wavelet).shape == (4, F)
    t = lng["db8_64x70/zero"]["tensors"][0]
    R1, C1 = (64 + 15) // 2, (70 + 15) // 2
    R2, C2 = (R1 + 15) // 2, (C1 + 15) // 2
    assert t["packed_shape"][-2:] == [R2 + R2 + R1, C2 + C2 + C1]
    assert t["coeff_numel"] - 4 * (4 * R2 * C2 + 3 * R1 * C1) == 4704  # non-tight: padding zeros in the population
    comps = man["components"]
    assert sorted(comps) == sorted("%s/%s" % (n, m) for n in ("db8_3x3", "bior33_2x5", "haar_1x7") for m in MODES)
    assert [k for k in sorted(comps) if comps[k]["error"]] == ["haar_1x7/reflect"]
    for k, c in comps.items():
        assert min(c["shape"][-2:]) < O.dec_len(c["wavelet"]) or c["wavelet"] == "haar"
        assert c["level"] > O.dwt_max_level(min(c["shape"][-2:]), O.dec_len(c["wavelet"]))  # past the clamp
        if not c["error"]:
            y0, y1 = arrs["comp/%s/out0" % k], arrs["comp/%s/out1" % k]
            assert np.array(c["thr32_bits"], np.uint32).view(np.float32)[()] > 0 and not np.array_equal(y0, y1)

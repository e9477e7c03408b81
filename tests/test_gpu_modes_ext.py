"""GPU parity of the extension modes beyond the PyWavelets grid of tests/test_gpu_modes.py, against
the fixture of tools/gen_golden_modes_ext.py (the reference chain of tests/modes_ref.py, anchored to
pywt by tests/test_modes_ext_ref.py).  Everything bit for bit: outputs (the stored array where the
fixture holds one, the hash always), thr64, thr32, max |c|, coeff_numel, eff_level, the zero count,
and the packed array's hash through the component entry where the level is at least 1.
  tiny    k_mtiny_fwd / k_mtiny_inv over several waves of a segment, several such segments a table
  group   a list longer than one launch group whose second group starts with a multi-wave tensor
  pct     percentiles on, at the end of and past a plateau of exact zeros in the packed array
  long    db8, bior3.3, sym3, coif1, bior1.3 and dmey in the per-level kernels
  comp    the component entries at unclamped levels: lines shorter than the filter"""
import json
import os

import numpy as np
import pytest
import torch

from tests import golden_io as G
from wavelettransforms_amd import workloads as W

pytestmark = pytest.mark.gpu

MAN = json.load(open(os.path.join(G.GOLDEN, "modes_ext_manifest.json")))
ARR = np.load(os.path.join(G.GOLDEN, "modes_ext_cases.npz"))
MODES = ["zero", "constant", "symmetric", "reflect", "periodic"]
LONG = ["db8_30x33", "db8_64x70", "bior33_14x17", "sym3_12x10", "coif1_10x12", "bior13_10x11", "dmey_124x130"]
PCT = ["p96x100", "p3x3", "p8x6"]
COMP = ["db8_3x3", "bior33_2x5", "haar_1x7"]


@pytest.fixture(scope="module")
def eng():
    from wavelettransforms_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


def _inputs(case):
    return [W.synth_numpy(tuple(t["shape"]), *t["synth"]) for t in case["tensors"]]


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)[()]


def _check(case, name, outs, recs):
    assert len(outs) == len(recs) == len(case["tensors"]), name
    for ti, (t, o, r) in enumerate(zip(case["tensors"], outs, recs)):
        tag = (name, ti)
        out = o.cpu().numpy()
        key = "case/%s/%d/out" % (name, ti)
        assert list(out.shape) == t["shape"], tag
        if key in ARR.files:
            assert np.array_equal(out, ARR[key]), tag
        assert G.canon_hash(out) == t["out_hash"], tag
        assert np.float64(r["thr64"]).tobytes() == np.float64(float.fromhex(t["thr64_hex"])).tobytes(), tag
        assert r["thr32_bits"] == t["thr32_bits"] and r["max_abs_bits"] == t["max_abs_bits"], tag
        assert r["coeff_numel"] == t["coeff_numel"], tag
        assert r["eff_level"] == t["eff_level"], tag
        assert r["zero_count"] == t["zero_count"] and r["numel"] == out.size, tag


def _check_packed(eng, case, name, xs):
    """the packed array itself (padding zeros included) through the component entry, and back"""
    for ti, (t, x) in enumerate(zip(case["tensors"], xs)):
        if len(t["shape"]) < 2 or t["eff_level"] == 0:
            continue
        P = eng.wavedec2_packed_mode(x, case["wavelet"], t["eff_level"], case["mode"])
        assert list(P.shape) == t["packed_shape"], (name, ti)
        assert G.canon_hash(P.cpu().numpy()) == t["packed_hash"], (name, ti)
        y = eng.waverec2_packed_mode(P, x.shape, case["wavelet"], t["eff_level"], case["mode"],
                                     thr32=float(_f32(t["thr32_bits"])))
        assert G.canon_hash(y.cpu().numpy()) == t["out_hash"], (name, ti)


def _run_case(eng, name, packed=True, in_place=False):
    case = MAN["cases"][name]
    xs_np = _inputs(case)
    xs = [torch.from_numpy(x).cuda() for x in xs_np]
    outs, recs = eng.prune(xs, case["wavelet"], case["level"], case["pct"], outs=xs if in_place else None,
                           carry_level=False, mode=case["mode"])
    _check(case, name, outs, recs)
    if in_place:
        assert all(a is b for a, b in zip(outs, xs))
        return
    for x, x_np in zip(xs, xs_np):
        assert np.array_equal(x.cpu().numpy(), x_np), "out of place: the input is untouched"
    if packed:
        _check_packed(eng, case, name, xs)


@pytest.mark.parametrize("mode", MODES)
def test_tiny_images_over_several_waves(eng, mode):
    """waves of 64/64/64/18 and 32/13 images, 65 and 129 images of non-square kernels, a tensor of the
    per-level kernels and one at level 0 between them: one call per wavelet"""
    for lst in ("tiny_haar", "tiny_db2"):
        name = "%s/%s" % (lst, mode)
        ts = MAN["cases"][name]["tensors"]
        assert sum(len(t.get("waves", ())) >= 3 for t in ts) >= 1  # (tests/test_modes_ext_ref.py holds the rest)
        _run_case(eng, name)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("mode", ["symmetric", "periodic"])
def test_second_launch_group_starts_with_a_multi_wave_tensor(eng, mode, in_place):
    name = "group_haar/%s" % mode
    ts = MAN["cases"][name]["tensors"]
    assert len(ts) > 24 and len(ts[24]["waves"]) >= 3
    _run_case(eng, name, packed=False, in_place=in_place)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tensor", PCT)
def test_percentiles_over_a_zero_plateau(eng, tensor, mode):
    """pct 0, 5, the last rank on the plateau of exact zeros, half way to the smallest non-zero,
    50, 99.9 and 100 over a packed array with padding zeros and exact-zero coefficients"""
    names = sorted(n for n in MAN["cases"] if n.startswith("%s/%s/" % (tensor, mode)))
    t0 = MAN["cases"][names[0]]["tensors"][0]
    assert len(names) == (7 if t0["zeros_packed"] else 5)
    for i, name in enumerate(names):
        _run_case(eng, name, packed=i == 0)


@pytest.mark.parametrize("mode", MODES)
def test_long_and_unfamiliar_filters(eng, mode):
    from wavelettransforms_amd import _native as N
    assert N.lib().wtp_dec_len(eng.wavelet_id("dmey")) == 62
    for cname in LONG:
        _run_case(eng, "%s/%s" % (cname, mode))


@pytest.mark.parametrize("mode", MODES)
def test_component_entries_at_unclamped_levels(eng, mode):
    """lines shorter than the filter (the extension wraps more than once) reach the kernels only
    through the component entries, which take the level as given"""
    for cname in COMP:
        key = "%s/%s" % (cname, mode)
        c = MAN["components"][key]
        x = torch.from_numpy(W.synth_numpy(tuple(c["shape"]), *c["synth"])).cuda()
        if c["error"]:  # some level would analyse a one-sample line under reflect: undefined
            with pytest.raises(ValueError, match="bad packed-shape request"):
                eng.wavedec2_packed_mode(x, c["wavelet"], c["level"], mode)
            with pytest.raises(RuntimeError, match="cannot extend"):
                eng.waverec2_packed_mode(torch.zeros(3, 8, device="cuda"), x.shape, c["wavelet"], c["level"], mode)
            continue
        P = eng.wavedec2_packed_mode(x, c["wavelet"], c["level"], mode)
        ref = ARR["comp/%s/packed" % key]
        assert list(P.shape) == c["packed_shape"] == list(ref.shape), key
        assert np.array_equal(P.cpu().numpy(), ref) and G.canon_hash(P.cpu().numpy()) == c["packed_hash"], key
        for thr32, tag in ((None, "out0"), (float(_f32(c["thr32_bits"])), "out1")):
            y = eng.waverec2_packed_mode(P, x.shape, c["wavelet"], c["level"], mode, thr32=thr32).cpu().numpy()
            assert np.array_equal(y, ARR["comp/%s/%s" % (key, tag)]), (key, tag)
            assert G.canon_hash(y) == c[tag + "_hash"], (key, tag)

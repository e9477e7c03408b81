"""GPU parity of the percentile sweep (wtp_prune_sweep_f32; engine.prune_sweep): every percentile's
outputs and records against the PyWavelets + NumPy goldens and the C oracle, bit for bit -- the
record's path apart, which reads 5.  Every expected value comes from the oracle or the goldens,
never from the library under test (where a test compares two library calls, both are also held
against the oracle)."""
import math
import os
import json
import warnings

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import golden_io as G
from tests.test_sweep_core import REF_PCTS, boundary_array

pytestmark = pytest.mark.gpu

SWEEP = 5
FIELDS = ("numel", "zero_count", "coeff_numel", "thr64", "thr32_bits", "max_abs_bits", "eff_level")
E05 = G.W.sigma_exponent(0.05)


@pytest.fixture(scope="module")
def eng():
    from wavelettransforms_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_f32(bits, value):
    """bit for bit, NaN == NaN (x86's inf - inf is -nan, the GPU's +nan; either prunes nothing)"""
    got = np.array(bits, np.uint32).view(np.float32)[()]
    return (math.isnan(got) and math.isnan(value)) or int(bits) == G.f32_bits(value)


def _levels(xs, wavelet, level, carry):
    """the level every tensor is called with (dwt_pruning.py:64-65: the clamp carries over)"""
    out, cur = [], level
    F = O.dec_len(wavelet) if O.wavelet_id(wavelet) >= 0 else 2
    for x in xs:
        if not carry:
            cur = level
        if x.ndim >= 2:
            cur = min(cur, O.dwt_max_level(min(x.shape[-2:]), F))
        out.append(cur)
    return out


def _check_rec(r, ref, tag, zero_count=True):
    assert r["path"] == SWEEP, tag
    assert r["numel"] == ref["numel"] and r["coeff_numel"] == ref["coeff_numel"], tag
    assert r["eff_level"] == ref["eff_level"], tag
    assert G.f64_bits_equal(r["thr64"], ref["thr64"]), (tag, r["thr64"], ref["thr64"])
    if not math.isnan(ref["thr64"]):
        assert np.float64(r["thr64"]).tobytes() == np.float64(ref["thr64"]).tobytes(), tag
    assert _same_f32(r["thr32_bits"], ref["thr32"]), tag
    assert _same_f32(r["max_abs_bits"], ref["max_abs"]), tag
    assert r["zero_count"] == (ref["zero_count"] if zero_count else 0), tag


def _sweep_vs_oracle(eng, xs_np, wavelet, level, pcts, carry=True, xs=None, outs=None, tag=""):
    """One sweep of the list against one oracle call per tensor and percentile."""
    if xs is None:
        xs = [torch.from_numpy(x).cuda() for x in xs_np]
    got, recs = eng.prune_sweep(xs, wavelet, level, pcts, outs=outs, carry_level=carry)
    lv = _levels(xs_np, wavelet, level, carry)
    assert len(got) == len(recs) == len(pcts)
    for k, p in enumerate(pcts):
        assert len(got[k]) == len(recs[k]) == len(xs_np)
        for t, x in enumerate(xs_np):
            ref, rr = O.prune_tensor(x, wavelet, lv[t], p)
            o = got[k][t].cpu().numpy()
            assert o.shape == x.shape, (tag, k, t)
            assert np.array_equal(_bits(o), _bits(ref)), (tag, k, t, x.shape, p)
            _check_rec(recs[k][t], rr, (tag, k, t, x.shape, p))
    return got, recs


VALID = sorted(n for n, r in G.manifest()["cases"].items() if "error" not in r)


@pytest.mark.parametrize("name", VALID)
def test_golden_cases(eng, name):
    """its own percentile against the golden, 0 / 23.6 / 50 / 100 against the oracle"""
    rec = G.manifest()["cases"][name]
    x = G.case_input(name)
    pcts = [rec["pct"], 0.0, 23.599999999999998, 50.0, 100.0]
    got, recs = _sweep_vs_oracle(eng, [x], rec["wavelet"], rec["level_in"], pcts, tag=name)
    out, r = got[0][0].cpu().numpy(), recs[0][0]
    assert G.canon_hash(out) == rec["out_hash"]
    if name + "/out" in G.arrays():
        assert np.array_equal(out, G.arrays()[name + "/out"], equal_nan=True)
    assert r["path"] == SWEEP and r["eff_level"] == rec["eff_level"] and r["numel"] == x.size
    assert G.f64_bits_equal(r["thr64"], rec["thr64"])
    assert _same_f32(r["thr32_bits"], np.array(rec["thr32_bits"], np.uint32).view(np.float32)[()])
    assert _same_f32(r["max_abs_bits"], np.array(rec["max_abs_bits"], np.uint32).view(np.float32)[()])
    assert r["zero_count"] == rec["zero_count"] and r["coeff_numel"] == rec["coeff_numel"]


def test_one_percentile_equals_prune(eng):
    """one call per wavelet, the transformed tensor first so that the carry leaves it its level:
    haar level 2 of (9, 5, 7, 7), bior3.3 level 3 of (96, 100) (not tight: padding zeros in the
    population), each beside a 1-D tensor and a 4-D tensor the clamp takes to level 0"""
    for wavelet, level, shapes in (("haar", 2, [(9, 5, 7, 7), (301,), (16, 4, 1, 1)]),
                                   ("bior3.3", 3, [(96, 100), (301,), (16, 4, 3, 3)])):
        xs_np = [G.W.synth_numpy(s, 82, i, E05) for i, s in enumerate(shapes)]
        assert _levels(xs_np, wavelet, level, True) == [level, level, 0]
        xs = [torch.from_numpy(x).cuda() for x in xs_np]
        for carry in (True, False):
            a_outs, a_recs = eng.prune(xs, wavelet, level, 61.8, carry_level=carry)
            (b_outs,), (b_recs,) = _sweep_vs_oracle(eng, xs_np, wavelet, level, [61.8], carry=carry, xs=xs)
            for a, b, ra, rb in zip(a_outs, b_outs, a_recs, b_recs):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
                assert all(ra[f] == rb[f] for f in FIELDS), (ra, rb)
                assert rb["path"] == SWEEP != ra["path"]
    pr, pc = O.packed_shape(96, 100, 3)
    assert b_recs[0]["coeff_numel"] == pr * pc > xs_np[0].size, "padding zeros are in the population"


@pytest.mark.parametrize("carry", [True, False], ids=["carry", "layers"])
def test_reference_percentiles_mixed_list(eng, carry):
    shapes = [(64, 64, 3, 3), (33, 7, 3, 3), (50000,), (4099,), (5,), (1,)]
    xs_np = [G.W.synth_numpy(s, 83, i, E05) for i, s in enumerate(shapes)]
    _sweep_vs_oracle(eng, xs_np, "bior3.3", 5, REF_PCTS, carry=carry, tag="bior3.3")
    haar = [G.W.synth_numpy((2, 3, 8, 8), 83, 9, E05)] + xs_np[1:]  # level 2, then the 3 x 3 clamp to 1
    _sweep_vs_oracle(eng, haar, "haar", 2, REF_PCTS, carry=carry, tag="haar")


def _special_arrays():
    rng = np.random.default_rng(8)
    four = np.array([0.01, -0.02, 0.5, -3.0], np.float32)[rng.integers(0, 4, 30011)]
    sparse = (rng.standard_normal(20000) * 0.05).astype(np.float32)
    sparse[rng.random(20000) < 0.7] = 0.0
    odd = (rng.standard_normal(5000) * 0.05).astype(np.float32)
    odd[:50] = -0.0
    odd[50:100] = np.float32(1e-42)
    odd[100:110] = np.float32(-3e-45)
    odd[110:113] = np.inf
    odd[113] = -np.inf
    return {"equal": np.full(40000, 0.0371, np.float32), "four": four, "sparse": sparse, "odd": odd,
            "top_digit": boundary_array(False), "second_digit": boundary_array(True)}


def test_ties_and_special_values(eng):
    arrs = _special_arrays()
    pcts = [0.0, 10.0, 50.0, 90.0, 100.0]
    _sweep_vs_oracle(eng, list(arrs.values()), "haar", 1, pcts, tag="specials")
    # the same values as 2-D tensors under a transform at level 0 and at level 1
    _sweep_vs_oracle(eng, [arrs["four"][:30000].reshape(100, 300), arrs["sparse"].reshape(8, 50, 50)], "haar", 1, pcts,
                     carry=False, tag="specials 2-D")


def test_one_nan_keeps_everything(eng):
    x = _special_arrays()["odd"].copy()
    x[777] = np.nan
    got, recs = eng.prune_sweep([torch.from_numpy(x).cuda()], "haar", 1, [0.0, 10.0, 50.0, 90.0, 100.0])
    for k, p in enumerate([0.0, 10.0, 50.0, 90.0, 100.0]):
        ref, rr = O.prune_tensor(x, "haar", 1, p)
        assert math.isnan(rr["thr64"]) and math.isnan(recs[k][0]["thr64"]) and math.isnan(recs[k][0]["thr32"])
        assert np.array_equal(_bits(got[k][0].cpu().numpy()), _bits(x)) and np.array_equal(_bits(ref), _bits(x))
        _check_rec(recs[k][0], rr, ("nan", p))


def test_two_launch_groups(eng):
    man = json.load(open(os.path.join(G.GOLDEN, "modes_ext_manifest.json")))
    group = [tuple(t["shape"]) for t in man["cases"]["group_haar/symmetric"]["tensors"]]
    shapes = group[:26]
    for at, s in ((3, (17,)), (11, (4099,)), (24, (301,)), (29, (5,))):
        shapes.insert(at, s)
    assert len(shapes) == 30 and sum(len(s) == 1 for s in shapes) == 4
    xs_np = [G.W.synth_numpy(s, 84, i, E05) for i, s in enumerate(shapes)]
    lv = _levels(xs_np, "haar", 2, False)
    assert {0, 1, 2} <= set(l for x, l in zip(xs_np, lv) if x.ndim >= 2)
    pcts = [78.6, 10.0, 78.6]
    got, recs = _sweep_vs_oracle(eng, xs_np, "haar", 2, pcts, carry=False, tag="30 tensors")
    for a, b in zip(got[0], got[2]):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert recs[0] == recs[2]


def test_unaligned_input(eng):
    for n in (4099, 16384, 40000):
        buf = torch.from_numpy(G.W.synth_numpy((n + 1,), 85, n % 5, E05)).cuda()
        x = buf[1:]
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        outbuf = [torch.zeros(n + 3, device="cuda") for _ in range(3)]
        outs = [[outbuf[0][3:3 + n]], [outbuf[1][:n]], [outbuf[2][2:2 + n]]]
        _sweep_vs_oracle(eng, [x.cpu().numpy()], "haar", 1, [10.0, 50.0, 90.0], xs=[x], outs=outs, tag=n)
        assert float(outbuf[0][:3].abs().sum()) == 0 and float(outbuf[1][n:].abs().sum()) == 0


@pytest.mark.parametrize("shape,wavelet,level", [((20, 16, 3, 3), "bior3.3", 5), ((40000,), "haar", 1), ((6, 4, 10, 12), "haar", 1)])
def test_in_place_second_output(eng, shape, wavelet, level):
    x_np = G.W.synth_numpy(shape, 86, 1, E05)
    pcts = [23.6, 61.8, 90.0]
    ref_outs, ref_recs = _sweep_vs_oracle(eng, [x_np], wavelet, level, pcts, tag="out of place")
    x = torch.from_numpy(x_np).cuda()
    outs = [[torch.empty_like(x)], [x], [torch.empty_like(x)]]
    got, recs = _sweep_vs_oracle(eng, [x_np], wavelet, level, pcts, xs=[x], outs=outs, tag="in place")
    assert got[1][0] is x and recs == ref_recs
    for k in range(3):
        assert torch.equal(got[k][0].view(torch.int32), ref_outs[k][0].view(torch.int32))


def test_thresholds_only(eng):
    shapes = [(64, 64, 3, 3), (4099,), (2, 3, 8, 8), (96, 100)]
    xs_np = [G.W.synth_numpy(s, 87, i, E05) for i, s in enumerate(shapes)]
    xs = [torch.from_numpy(x).cuda() for x in xs_np]
    pcts = [10.0, 50.0, 100.0]
    _, full = _sweep_vs_oracle(eng, xs_np, "haar", 2, pcts, xs=xs)
    canary = [[torch.full_like(x, -7.25) for x in xs] for _ in pcts]
    for outs in (canary, None):
        got, recs = eng.prune_sweep(xs, "haar", 2, pcts, outs=outs, thresholds_only=True)
        assert got is None
        lv = _levels(xs_np, "haar", 2, True)
        for k, p in enumerate(pcts):
            for t, x in enumerate(xs_np):
                _check_rec(recs[k][t], O.prune_tensor(x, "haar", lv[t], p)[1], (k, t), zero_count=False)
                assert all(recs[k][t][f] == full[k][t][f] for f in FIELDS if f != "zero_count")
    torch.cuda.synchronize()
    assert all(bool((c == -7.25).all()) for cs in canary for c in cs), "no output is written"
    for x, x_np in zip(xs, xs_np):
        assert np.array_equal(x.cpu().numpy(), x_np)


def test_graph_capture_replays_on_refreshed_inputs(eng):
    shapes = [(33, 7, 3, 3), (4099,), (2, 3, 8, 8), (96, 100), (5,)]
    a_np = [G.W.synth_numpy(s, 88, i, E05) for i, s in enumerate(shapes)]
    b_np = [G.W.synth_numpy(s, 89, i, E05 + 1) for i, s in enumerate(shapes)]
    pcts = [38.2, 90.0, 10.0]
    lv = _levels(a_np, "bior3.3", 3, False)
    assert lv == [0, 3, 0, 3, 3]  # level-0 4-D tensors, 1-D tensors, a transformed one
    xs = [torch.from_numpy(x).cuda() for x in a_np]
    outs = [[torch.empty_like(x) for x in xs] for _ in pcts]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up: the workspace exists before the capture
        eng.launch_sweep(xs, "bior3.3", 3, pcts, outs=outs, carry_level=False, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.cuda.graph(g, stream=s):
            _, resd = eng.launch_sweep(xs, "bior3.3", 3, pcts, outs=outs, carry_level=False)
    n = len(xs)
    for inputs in (b_np, a_np):
        for x, v in zip(xs, inputs):
            x.copy_(torch.from_numpy(v))
        for os_ in outs:
            for o in os_:
                o.zero_()
        g.replay()
        torch.cuda.synchronize()
        blocks = resd.view(len(pcts), -1)
        for k, p in enumerate(pcts):
            recs = eng.decode(blocks[k], n)
            for t, v in enumerate(inputs):
                ref, rr = O.prune_tensor(v, "bior3.3", lv[t], p)
                assert np.array_equal(_bits(outs[k][t].cpu().numpy()), _bits(ref)), (k, t)
                _check_rec(recs[t], rr, ("replay", k, t))


def test_percentile_calls_around_a_sweep(eng):
    """each entry has its workspace kind: the selection state of the percentile entries survives"""
    dev = torch.device("cuda", torch.cuda.current_device())
    conv_np = [G.W.synth_numpy(s, 90, i, E05) for i, s in enumerate([(64, 64, 3, 3), (128, 64, 1, 1), (1000,)])]
    big_np = [G.W.synth_numpy((200, 300), 90, 7, E05)]

    def percentile_round():
        for xs_np, wavelet, level, pct in ((conv_np, "bior3.3", 5, 50.0), (big_np, "db4", 3, 61.8)):
            outs, res = eng.prune([torch.from_numpy(x).cuda() for x in xs_np], wavelet, level, pct, carry_level=False)
            for x, o, r in zip(xs_np, outs, res):
                ref, rr = O.prune_tensor(x, wavelet, level, pct)
                assert np.array_equal(_bits(o.cpu().numpy()), _bits(ref)), (x.shape, wavelet)
                assert r["zero_count"] == rr["zero_count"] and G.f64_bits_equal(r["thr64"], rr["thr64"])

    percentile_round()
    ws = eng.workspace(dev, 256)
    _sweep_vs_oracle(eng, conv_np + big_np, "db4", 3, [10.0, 61.8, 100.0], carry=False, tag="between")
    assert eng.workspace(dev, 256) is ws
    assert eng.workspace(dev, 256, kind="sweep").data_ptr() != ws.data_ptr()
    percentile_round()


def test_mirror(eng, capsys):
    from wavelettransforms_amd import dwt_pruning as D
    shapes = [(16, 8, 3, 3), (6, 4, 10, 12), (77,)]
    ws_np = [G.W.synth_numpy(s, 91, i, E05) for i, s in enumerate(shapes)]
    pcts = [10.0, 50.0, 78.6]
    for to_dev in (lambda t: t, lambda t: t.cuda()):
        weights = [to_dev(torch.from_numpy(x)) for x in ws_np]
        capsys.readouterr()
        swept = D.multi_resolution_analysis_sweep(weights, "haar", 1, pcts)
        assert "Percentile" not in capsys.readouterr().out
        assert len(swept) == len(pcts)
        lv = _levels(ws_np, "haar", 1, True)
        for p, (outs, total) in zip(pcts, swept):
            one_outs, one_total = D.multi_resolution_analysis(weights, "haar", 1, p, verbose=False)
            assert total == one_total and isinstance(total, int)
            want = 0
            for w, o, o1, x, l in zip(weights, outs, one_outs, ws_np, lv):
                assert o.device == w.device and o.dtype == w.dtype and o.shape == w.shape
                ref, rr = O.prune_tensor(x, "haar", l, p)
                assert np.array_equal(_bits(o.cpu().numpy()), _bits(ref)) and torch.equal(o.cpu(), o1.cpu())
                want += rr["zero_count"]
            assert total == want

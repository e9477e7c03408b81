"""GPU parity of the global percentile (wtp_prune_global_f32; engine.prune_global): ONE threshold per
percentile over the pool of every tensor's coefficients.  Every expected value comes from the
unchanged oracle, bit for bit: the coefficients and eff_level of a tensor from O.prune_tensor(...,
want_coeffs=True), thr64 and the maximum from O.percentile_abs of the concatenated pool, the outputs
from O.waverec2_packed(coeffs, ..., float32(thr64)) or np.where(|x| < thr32, 0, x).  Where a test
compares two library calls, both are also held against the oracle."""
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import golden_io as G
from tests.ref_helpers import np_ranks
from tests.test_gpu_sweep import _bits, _levels, _same_f32, _special_arrays
from tests.test_sweep_core import REF_PCTS

pytestmark = pytest.mark.gpu

GLOBAL, SWEEP = 7, 5
FIELDS = ("numel", "zero_count", "coeff_numel", "thr64", "thr32_bits", "max_abs_bits", "eff_level")
E05 = G.W.sigma_exponent(0.05)


@pytest.fixture(scope="module")
def eng():
    from wavelettransforms_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


class Ref:
    """The oracle's side of one list: every tensor's level, coefficients and the pool, computed once;
    per percentile the pool's threshold and every tensor's output."""

    def __init__(self, xs_np, wavelet, level, carry):
        self.xs, self.wavelet = xs_np, wavelet
        self.lv = _levels(xs_np, wavelet, level, carry)
        self.coeffs, self.eff = [], []
        for x, l in zip(xs_np, self.lv):
            _, rr, c = O.prune_tensor(x, wavelet, l, 50.0, want_coeffs=True)
            self.eff.append(rr["eff_level"])
            # a transformed tensor contributes its whole packed array, every other its raw values
            self.coeffs.append(c if (x.ndim >= 2 and rr["eff_level"] >= 1) else x)
        self.pool = np.concatenate([np.asarray(c, np.float32).ravel() for c in self.coeffs])
        self._at = {}

    def at(self, p):
        if p not in self._at:
            thr64, mx = O.percentile_abs(self.pool, p)
            thr32 = np.float32(thr64)
            outs = []
            for x, c, e in zip(self.xs, self.coeffs, self.eff):
                if x.ndim >= 2 and e >= 1:
                    outs.append(O.waverec2_packed(c, x.shape, self.wavelet, e, thr32))
                else:
                    with np.errstate(invalid="ignore"):
                        outs.append(np.where(np.abs(x) < thr32, np.float32(0), x))
            self._at[p] = (thr64, thr32, mx, outs)
        return self._at[p]


def _check_rec(r, ref, p, t, tag, zero_count=True):
    thr64, thr32, mx, outs = ref.at(p)
    x = ref.xs[t]
    assert r["path"] == GLOBAL, tag
    assert r["numel"] == x.size and r["coeff_numel"] == np.asarray(ref.coeffs[t]).size, tag   # the tensor's own
    assert r["eff_level"] == ref.eff[t], tag
    assert G.f64_bits_equal(r["thr64"], thr64), (tag, r["thr64"], thr64)                      # the pool's
    if not math.isnan(thr64):
        assert np.float64(r["thr64"]).tobytes() == np.float64(thr64).tobytes(), tag
    assert _same_f32(r["thr32_bits"], thr32), tag
    assert _same_f32(r["max_abs_bits"], mx), tag
    assert r["zero_count"] == (int((outs[t] == 0).sum()) if zero_count else 0), tag


def _global_vs_oracle(eng, xs_np, wavelet, level, pcts, carry=True, xs=None, outs=None, tag="", ref=None):
    """One global call of the list against the oracle's pool."""
    if xs is None:
        xs = [torch.from_numpy(x).cuda() for x in xs_np]
    if ref is None:
        ref = Ref(xs_np, wavelet, level, carry)
    got, recs = eng.prune_global(xs, wavelet, level, pcts, outs=outs, carry_level=carry)
    assert len(got) == len(recs) == len(pcts)
    for k, p in enumerate(pcts):
        assert len(got[k]) == len(recs[k]) == len(xs_np)
        want = ref.at(p)[3]
        for t, x in enumerate(xs_np):
            o = got[k][t].cpu().numpy()
            assert o.shape == x.shape, (tag, k, t)
            assert np.array_equal(_bits(o), _bits(want[t])), (tag, k, t, x.shape, p)
            _check_rec(recs[k][t], ref, p, t, (tag, k, t, x.shape, p))
    return got, recs, ref


def _sweep_held_to_oracle(eng, xs_np, xs, wavelet, level, pcts, carry):
    got, recs = eng.prune_sweep(xs, wavelet, level, pcts, carry_level=carry)
    lv = _levels(xs_np, wavelet, level, carry)
    for k, p in enumerate(pcts):
        for t, x in enumerate(xs_np):
            ref, rr = O.prune_tensor(x, wavelet, lv[t], p)
            assert np.array_equal(_bits(got[k][t].cpu().numpy()), _bits(ref)), (k, t)
            assert G.f64_bits_equal(recs[k][t]["thr64"], rr["thr64"]) and recs[k][t]["zero_count"] == rr["zero_count"]
    return got, recs


@pytest.mark.parametrize("shape,wavelet,level", [((9, 5, 7, 7), "haar", 2), ((96, 100), "bior3.3", 3), ((4099,), "haar", 1)])
def test_one_tensor_is_the_sweep(eng, shape, wavelet, level):
    """a pool of one tensor is that tensor's population: outputs and record fields are the sweep's"""
    x_np = G.W.synth_numpy(shape, 92, 1, E05)
    xs = [torch.from_numpy(x_np).cuda()]
    pcts = [23.6, 50.0, 100.0]
    a_outs, a_recs = _sweep_held_to_oracle(eng, [x_np], xs, wavelet, level, pcts, True)
    b_outs, b_recs, ref = _global_vs_oracle(eng, [x_np], wavelet, level, pcts, xs=xs, tag=shape)
    for k in range(len(pcts)):
        assert torch.equal(a_outs[k][0].view(torch.int32), b_outs[k][0].view(torch.int32))
        ra, rb = a_recs[k][0], b_recs[k][0]
        assert all(ra[f] == rb[f] for f in FIELDS), (ra, rb)
        assert (ra["path"], rb["path"]) == (SWEEP, GLOBAL)
    if shape == (96, 100):
        pr, pc = O.packed_shape(96, 100, 3)
        assert b_recs[0][0]["coeff_numel"] == pr * pc > x_np.size, "padding zeros are in the pool"


MIXED = [(64, 64, 3, 3), (33, 7, 3, 3), (2, 3, 8, 8), (50000,), (4099,), (5,), (1,)]


@pytest.mark.parametrize("carry", [True, False], ids=["carry", "layers"])
@pytest.mark.parametrize("wavelet,level", [("bior3.3", 5), ("haar", 2)])
def test_mixed_list_at_the_reference_percentiles(eng, wavelet, level, carry):
    # layers of different scales, as a model's are: the pool's threshold is then no tensor's own
    xs_np = [G.W.synth_numpy(s, 93, i, E05 - (i % 3)) for i, s in enumerate(MIXED)]
    xs = [torch.from_numpy(x).cuda() for x in xs_np]
    lv = _levels(xs_np, wavelet, level, carry)
    if wavelet == "haar":
        assert max(lv) >= 1, "some tensor is transformed"
    first, rest = [0.0] + REF_PCTS[:7], [REF_PCTS[7], 100.0, 0.0]  # ten percentiles: two calls
    assert REF_PCTS[7] == 100.0
    ref = Ref(xs_np, wavelet, level, carry)
    for pcts in (first, rest):
        got, recs, _ = _global_vs_oracle(eng, xs_np, wavelet, level, pcts, carry=carry, xs=xs, tag=wavelet, ref=ref)
        for k in range(len(pcts)):  # the pool's values are the same in every record of a percentile
            assert len({(r["thr32_bits"], r["max_abs_bits"], np.float64(r["thr64"]).tobytes()) for r in recs[k]}) == 1
        swept, _ = _sweep_held_to_oracle(eng, xs_np, xs, wavelet, level, pcts, carry)
        for k, p in enumerate(pcts):
            if 0.0 < p < 100.0:  # a per-tensor implementation would pass everything above
                assert any(not torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[k], swept[k])), p


def test_the_rank_pair_straddles_two_tensors(eng):
    rng = np.random.default_rng(11)
    a = (rng.uniform(0.001, 0.01, 1000) * rng.choice([-1.0, 1.0], 1000)).astype(np.float32)
    b = (rng.uniform(0.02, 0.5, 1001) * rng.choice([-1.0, 1.0], 1001)).astype(np.float32)
    assert np.abs(a).max() < np.abs(b).min()
    n = a.size + b.size
    p = 100.0 * 999.5 / (n - 1)
    r0, above, gamma = np_ranks(n, p)
    srt = np.sort(np.abs(np.concatenate([a, b])))
    assert (r0, above) == (999, 0) and 0.0 < gamma < 1.0
    assert srt[r0] == np.abs(a).max() and srt[r0 + 1] == np.abs(b).min(), "rank r0 ends the first tensor"
    thr = []
    for xs_np in ([a, b], [b, a]):
        _, recs, ref = _global_vs_oracle(eng, xs_np, "haar", 1, [p, 50.0], tag="straddle")
        assert np.abs(a).max() < ref.at(p)[0] < np.abs(b).min()
        thr.append(np.float64(recs[0][0]["thr64"]).tobytes())
    assert thr[0] == thr[1]


def test_ties_across_tensors_and_special_values(eng):
    arrs = list(_special_arrays().values())
    pcts = [0.0, 10.0, 50.0, 90.0, 100.0]
    _, recs, _ = _global_vs_oracle(eng, arrs, "haar", 1, pcts, tag="specials")
    assert recs[4][0]["max_abs_bits"] == 0x7F800000  # the pool's maximum (inf, from `odd`) in `equal`'s record
    # one NaN in one tensor: every threshold is NaN and every output keeps its input's bits
    arrs = [a.copy() for a in arrs]
    arrs[3][777] = np.nan
    got, recs, ref = _global_vs_oracle(eng, arrs, "haar", 1, pcts, tag="one NaN")
    for k, p in enumerate(pcts):
        assert math.isnan(ref.at(p)[0])
        for t, x in enumerate(arrs):
            assert math.isnan(recs[k][t]["thr64"]) and math.isnan(recs[k][t]["thr32"])
            assert np.array_equal(_bits(got[k][t].cpu().numpy()), _bits(x))


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
    got, recs, _ = _global_vs_oracle(eng, xs_np, "haar", 2, pcts, carry=False, tag="30 tensors")
    for a, b in zip(got[0], got[2]):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert recs[0] == recs[2]


def test_more_than_one_chunk_a_workgroup(eng):
    """4 300 000 values are 263 chunks, more than a pass launches workgroups: two chunks each"""
    xs_np = [G.W.synth_numpy((4300000,), 94, 0, E05), G.W.synth_numpy((20, 16, 3, 3), 94, 1, E05 + 1)]
    assert -(-xs_np[0].size // 16384) == 263 > 256
    _global_vs_oracle(eng, xs_np, "haar", 1, [10.0, 61.8, 99.0], tag="263 chunks")


def test_unaligned_inputs_and_outputs(eng):
    ns = (4099, 16384, 40000)
    bufs = [torch.from_numpy(G.W.synth_numpy((n + 1,), 85, n % 5, E05)).cuda() for n in ns]
    xs = [b[1:] for b in bufs]
    assert all(x.data_ptr() % 16 == 4 and x.is_contiguous() for x in xs)
    outbuf = [[torch.zeros(n + 3, device="cuda") for n in ns] for _ in range(3)]
    outs = [[outbuf[0][i][3:3 + n] for i, n in enumerate(ns)], [outbuf[1][i][:n] for i, n in enumerate(ns)],
            [outbuf[2][i][2:2 + n] for i, n in enumerate(ns)]]
    _global_vs_oracle(eng, [x.cpu().numpy() for x in xs], "haar", 1, [10.0, 50.0, 90.0], xs=xs, outs=outs, tag="unaligned")
    for i, n in enumerate(ns):  # the guard words
        assert float(outbuf[0][i][:3].abs().sum()) == 0 and float(outbuf[1][i][n:].abs().sum()) == 0
        assert float(outbuf[2][i][:2].abs().sum()) == 0 and float(outbuf[2][i][2 + n:].abs().sum()) == 0


@pytest.mark.parametrize("shape,wavelet,level", [((20, 16, 3, 3), "bior3.3", 5), ((40000,), "haar", 1), ((6, 4, 10, 12), "haar", 1)])
def test_in_place_second_output(eng, shape, wavelet, level):
    xs_np = [G.W.synth_numpy(shape, 86, 1, E05), G.W.synth_numpy((777,), 86, 2, E05 - 1)]
    pcts = [23.6, 61.8, 90.0]
    ref_outs, ref_recs, ref = _global_vs_oracle(eng, xs_np, wavelet, level, pcts, tag="out of place")
    xs = [torch.from_numpy(x).cuda() for x in xs_np]
    outs = [[torch.empty_like(x) for x in xs], list(xs), [torch.empty_like(x) for x in xs]]
    got, recs, _ = _global_vs_oracle(eng, xs_np, wavelet, level, pcts, xs=xs, outs=outs, tag="in place", ref=ref)
    assert got[1][0] is xs[0] and got[1][1] is xs[1] and recs == ref_recs
    for k in range(3):
        for a, b in zip(got[k], ref_outs[k]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_thresholds_only(eng):
    shapes = [(64, 64, 3, 3), (4099,), (2, 3, 8, 8), (96, 100)]
    xs_np = [G.W.synth_numpy(s, 87, i, E05) for i, s in enumerate(shapes)]
    xs = [torch.from_numpy(x).cuda() for x in xs_np]
    pcts = [10.0, 50.0, 100.0]
    _, full, ref = _global_vs_oracle(eng, xs_np, "haar", 2, pcts, xs=xs)
    canary = [[torch.full_like(x, -7.25) for x in xs] for _ in pcts]
    for outs in (canary, None):
        got, recs = eng.prune_global(xs, "haar", 2, pcts, outs=outs, thresholds_only=True)
        assert got is None
        for k, p in enumerate(pcts):
            for t in range(len(xs_np)):
                _check_rec(recs[k][t], ref, p, t, (k, t), zero_count=False)
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
    assert _levels(a_np, "bior3.3", 3, False) == [0, 3, 0, 3, 3]
    xs = [torch.from_numpy(x).cuda() for x in a_np]
    outs = [[torch.empty_like(x) for x in xs] for _ in pcts]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up: the workspace exists before the capture
        eng.launch_global(xs, "bior3.3", 3, pcts, outs=outs, carry_level=False, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.cuda.graph(g, stream=s):  # a single captured stream
            _, resd = eng.launch_global(xs, "bior3.3", 3, pcts, outs=outs, carry_level=False)
    n = len(xs)
    for inputs in (b_np, a_np):
        ref = Ref(inputs, "bior3.3", 3, False)
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
            for t in range(n):
                assert np.array_equal(_bits(outs[k][t].cpu().numpy()), _bits(ref.at(p)[3][t])), (k, t)
                _check_rec(recs[t], ref, p, t, ("replay", k, t))


def test_per_tensor_calls_around_a_global_call(eng):
    """the entry has its own workspace kind: the persistent selection state at the start of the
    float32 entries' workspace survives a global call"""
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
    head = ws[:4096].clone()
    _global_vs_oracle(eng, conv_np + big_np, "db4", 3, [10.0, 61.8, 100.0], carry=False, tag="between")
    assert eng.workspace(dev, 256) is ws and torch.equal(ws[:4096], head)
    assert eng.workspace(dev, 256, kind="global").data_ptr() != ws.data_ptr()
    assert eng.workspace(dev, 256, kind="global").data_ptr() != eng.workspace(dev, 256, kind="sweep").data_ptr()
    percentile_round()


def test_dtypes_other_than_float32(eng):
    f = torch.zeros(8, 8, device="cuda")
    for bad in ([f.half()], [f.bfloat16()], [f.double()], [f, f.half()], [f.half(), f]):
        with pytest.raises(TypeError):
            eng.launch_global(bad, "haar", 1, [50.0])
        with pytest.raises(TypeError):
            eng.prune_global(bad, "haar", 1, [50.0])


def test_mirror(eng, capsys):
    from wavelettransforms_amd import dwt_pruning as D
    shapes = [(16, 8, 3, 3), (6, 4, 10, 12), (77,)]
    ws_np = [G.W.synth_numpy(s, 91, i, E05 - (i % 2)) for i, s in enumerate(shapes)]
    pcts = [10.0, 50.0, 78.6, 0.0, 23.6, 38.2, 61.8, 90.0, 100.0, 50.0, 99.0, 1.0]
    ref = Ref(ws_np, "haar", 1, True)
    calls = []
    real = eng.prune_global

    def counted(tensors, wavelet, level, p, **kw):
        calls.append(len(list(p)))
        return real(tensors, wavelet, level, p, **kw)

    for to_dev in (lambda t: t, lambda t: t.cuda()):
        weights = [to_dev(torch.from_numpy(x)) for x in ws_np]
        del calls[:]
        capsys.readouterr()
        eng.prune_global = counted
        try:
            pruned = D.multi_resolution_analysis_global(weights, "haar", 1, pcts)
        finally:
            eng.prune_global = real
        printed = capsys.readouterr().out
        assert calls == [8, 4], "twelve percentiles are two calls"
        assert "Percentile" not in printed
        # (16, 8, 3, 3) is transformed with odd sides: the reference's warning, once per percentile
        assert printed.count("Warning: Shape mismatch occurred in 1 weights") == len(pcts)
        assert len(pruned) == len(pcts)
        for p, (outs, total) in zip(pcts, pruned):
            want = ref.at(p)[3]
            assert isinstance(total, int) and total == sum(int((o == 0).sum()) for o in want)
            for w, o, r in zip(weights, outs, want):
                assert o.device == w.device and o.dtype == w.dtype and o.shape == w.shape
                assert np.array_equal(_bits(o.cpu().numpy()), _bits(r))
    # the totals are the sums of the records' zero counts
    _, recs = eng.prune_global([torch.from_numpy(x).cuda() for x in ws_np], "haar", 1, pcts[:8])
    for k, (outs, total) in enumerate(pruned[:8]):
        assert total == sum(r["zero_count"] for r in recs[k])

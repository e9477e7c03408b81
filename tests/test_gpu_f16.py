"""GPU parity of float16 weights (wtp_prune_f16, csrc/half.hip) against the PyWavelets 1.1.1 +
NumPy 1.26.4 fixtures of tools/gen_golden_f16.py, bit for bit: output words, thr64, the value the
compare used, the maximum, zero counts and levels.  Tensors that get no transform (kind B) stay in
float16 with NumPy's float16 percentile and compare; tensors that get one (kind A) run the float32
path and are narrowed once.  Shapes: 1, 2 and 37 weights, conv kernels the clamp leaves at level 0,
all zeros, half of the values tied, 41 145 weights (odd, three blocks of vectors), populations over
many binades, the transformed shapes of the modes fixtures, a result that underflows in the
narrowing, and a mixed list with and without the level carry.  The last section feeds +-inf and
NaN to the tensors that get no transform and holds them to the same NumPy rule restated in scalar
steps (half_ref.kind_b_ref), which tests/test_half_core.py ties to the fixtures."""
import contextlib
import io
import warnings

import numpy as np
import pytest
import torch

from tests import half_ref as H
from tests import special_values as SV
from wavelettransforms_amd import workloads as W

pytestmark = pytest.mark.gpu

CALL_NAMES = sorted({c["name"] for c in H.manifest()["calls"].values()})


@pytest.fixture(scope="module")
def eng():
    from wavelettransforms_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


def _inputs(call):
    return [H.make_input(t, W.synth_numpy) for t in call["tensors"]]


def _cuda(xs):
    return [torch.from_numpy(x).cuda() for x in xs]


def _words(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)


def _check(key, call, outs, recs, eng):
    for ti, (t, o, r) in enumerate(zip(call["tensors"], outs, recs)):
        tag = (key, ti)
        assert o.dtype == torch.float16 and list(o.shape) == t["shape"], tag
        got = _words(o)
        assert H.words_hash(got.view(np.float16)) == t["out_hash"], tag
        stored = H.arrays().get("%s/%d" % (key, ti))
        if stored is not None:
            assert np.array_equal(got, stored.view(np.uint16).reshape(-1)), tag
        assert np.float64(r["thr64"]).tobytes() == np.float64(float.fromhex(t["thr64_hex"])).tobytes(), tag
        assert r["thr32_bits"] == t["cmp_bits"], tag
        assert r["max_abs_bits"] == t["max_bits"], tag
        assert r["zero_count"] == t["zero_count"] == int((got & 0x7FFF == 0).sum()), tag
        assert r["eff_level"] == t["eff_level"] and r["coeff_numel"] == t["coeff_numel"], tag
        assert r["numel"] == got.size, tag
        assert (r["path"] == eng.MODE_HALF) == (t["kind"] == "B"), tag


def _run(eng, call, xs, **kw):
    return eng.prune(xs, call["wavelet"], call["level"], call["pct"], carry_level=call["carry"], mode=call["mode"], **kw)


@pytest.mark.parametrize("name", CALL_NAMES)
def test_fixture_calls(eng, name):
    """every fixture call at every stored percentile; the mixed list with and without the carry"""
    keys = sorted(k for k, c in H.manifest()["calls"].items() if c["name"] == name)
    assert keys
    for key in keys:
        call = H.manifest()["calls"][key]
        xs_np = _inputs(call)
        xs = _cuda(xs_np)
        outs, recs = _run(eng, call, xs)
        _check(key, call, outs, recs, eng)
        assert all(np.array_equal(_words(x), v.view(np.uint16).reshape(-1)) for x, v in zip(xs, xs_np)), "input untouched"


def test_wide_group(eng):
    """populations of 2..39 values over many binades, one call per percentile: the cases where an
    exact b - a or a float32 compare gives another answer are among them"""
    wide = H.manifest()["wide"]
    words = H.arrays()["wide/words"]
    assert sum(c["differs_exact_diff"] for c in wide) >= 20 and sum(c["differs_f32_compare"] for c in wide) >= 5
    for pct in sorted({c["pct"] for c in wide}):
        cases = [c for c in wide if c["pct"] == pct]
        xs = [torch.from_numpy(words[c["offset"]:c["offset"] + c["n"]].view(np.float16).copy()).cuda() for c in cases]
        outs, recs = eng.prune(xs, "haar", 2, pct)
        for c, o, r in zip(cases, outs, recs):
            want = words[c["offset"] + c["n"]:c["offset"] + 2 * c["n"]]
            assert np.array_equal(_words(o), want), c
            assert np.float64(r["thr64"]).tobytes() == np.float64(float.fromhex(c["thr64_hex"])).tobytes(), c
            assert r["thr32_bits"] == c["cmp_bits"] and r["max_abs_bits"] == c["max_bits"], c
            assert r["zero_count"] == c["zero_count"] and r["path"] == eng.MODE_HALF, c


def test_more_tensors_than_one_table(eng):
    """70 tensors in one call (tables of 32): each as it comes out of a call of its own"""
    wide = H.manifest()["wide"][:70]
    words = H.arrays()["wide/words"]
    xs = [torch.from_numpy(words[c["offset"]:c["offset"] + c["n"]].view(np.float16).copy()).cuda() for c in wide]
    outs, recs = eng.prune(xs, "haar", 2, 61.8)
    for i in (0, 1, 31, 32, 33, 63, 64, 69):
        o1, r1 = eng.prune([xs[i]], "haar", 2, 61.8)
        assert np.array_equal(_words(outs[i]), _words(o1[0])) and recs[i] == r1[0], i
    ref = [np.where(np.abs(x.cpu().numpy()) < np.float16(r["thr32"]), np.float16(0), x.cpu().numpy()) for x, r in zip(xs, recs)]
    assert all(np.array_equal(_words(o), v.view(np.uint16)) for o, v in zip(outs, ref))


@pytest.mark.parametrize("key", ["mixed_carry/50", "mixed_layers/50", "b_odd/50"])
def test_in_place_equals_out_of_place(eng, key):
    call = H.manifest()["calls"][key]
    xs = _cuda(_inputs(call))
    outs, recs = _run(eng, call, xs, outs=xs)
    assert all(o.data_ptr() == x.data_ptr() for o, x in zip(outs, xs))
    _check(key, call, outs, recs, eng)


@pytest.mark.parametrize("key,in_off,out_off", [("b_odd/50", 1, 1), ("b_odd/50", 1, 4), ("b_odd/50", 3, 0),
                                                ("b_vec37/50", 5, 7), ("a_c7x7/50", 1, 3), ("a_c3x3/50", 4, 12),
                                                ("mixed_carry/50", 7, 2)])
def test_subtensors_at_odd_element_offsets(eng, key, in_off, out_off):
    """tensors that start on a 2-byte boundary only, inside larger float16 buffers: the scalar head
    and tail, the vector body, and the word-by-word walk where input and output differ in phase;
    the words around the outputs stay as they were"""
    call = H.manifest()["calls"][key]
    xs_np = _inputs(call)
    xs, outs, bufs = [], [], []
    for x in xs_np:
        n = x.size
        bi = torch.zeros(n + 16, dtype=torch.float16, device="cuda")
        bo = torch.full((n + 32,), 7.0, dtype=torch.float16, device="cuda")
        bi[in_off:in_off + n] = torch.from_numpy(x.reshape(-1)).cuda()
        xs.append(bi[in_off:in_off + n].view(x.shape))
        outs.append(bo[out_off:out_off + n].view(x.shape))
        bufs.append((bo, n))
        assert xs[-1].data_ptr() % 16 == (bi.data_ptr() + 2 * in_off) % 16 and xs[-1].is_contiguous()
    got, recs = _run(eng, call, xs, outs=outs)
    _check(key, call, got, recs, eng)
    for bo, n in bufs:
        rest = torch.cat([bo[:out_off], bo[out_off + n:]])
        assert bool((rest == 7.0).all()), "words outside the output were written"


def test_graph_capture_replays_on_changed_inputs(eng):
    call = H.manifest()["calls"]["mixed_carry/50"]
    a_np = _inputs(call)
    b_np = [(-x[::-1]).copy() if x.ndim == 1 else (x * np.float16(0.5)).astype(np.float16) for x in a_np]
    ref_a = _run(eng, call, _cuda(a_np))
    ref_b = _run(eng, call, _cuda(b_np))
    xs = _cuda(a_np)
    outs = [torch.empty_like(x) for x in xs]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up: the workspace exists before the capture
        eng.launch(xs, call["wavelet"], call["level"], call["pct"], outs=outs, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.cuda.graph(g, stream=s):
            _, resd = eng.launch(xs, call["wavelet"], call["level"], call["pct"], outs=outs)
    for inputs, (ref_outs, ref_recs) in ((b_np, ref_b), (a_np, ref_a)):
        for x, v in zip(xs, inputs):
            x.copy_(torch.from_numpy(v))
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eng.decode(resd, len(xs)) == ref_recs
        for o, r in zip(outs, ref_outs):
            assert np.array_equal(_words(o), _words(r))
    _check("mixed_carry/50", call, outs, eng.decode(resd, len(xs)), eng)


def test_repeated_calls_give_identical_records(eng):
    """the workspace is left as the next call needs it: three calls on one stream, a float32 call
    of the same shapes in between"""
    call = H.manifest()["calls"]["mixed_carry/50"]
    xs = _cuda(_inputs(call))
    first = _run(eng, call, xs)
    eng.prune([x.float() for x in xs], call["wavelet"], call["level"], call["pct"])
    other = H.manifest()["calls"]["b_odd/50"]
    _run(eng, other, _cuda(_inputs(other)))
    for _ in range(2):
        outs, recs = _run(eng, call, xs)
        assert recs == first[1]
        assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(outs, first[0]))
    _check("mixed_carry/50", call, outs, recs, eng)


@pytest.mark.parametrize("key", ["conv_a/50", "conv_b/50"])
def test_prune_layer_weights_on_a_half_conv(eng, key):
    """prune_layer_weights on torch.nn.Conv2d(3, 8, 3).half(): dtype, counts and both printed lines"""
    from wavelettransforms_amd import dwt_pruning as D
    call = H.manifest()["calls"][key]
    t = call["tensors"][0]
    layer = torch.nn.Conv2d(3, 8, 3).half().cuda()
    assert list(layer.weight.shape) == t["shape"]
    bias = layer.bias.detach().clone()
    layer.weight.data = torch.from_numpy(_inputs(call)[0]).cuda()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        original, nonzero, zeros = D.prune_layer_weights(layer, call["wavelet"], call["level"], call["pct"])
    assert buf.getvalue().splitlines() == call["layer_lines"] and call["layer_lines"][0] == t["line"]
    assert (original, nonzero, zeros) == (layer.weight.numel(), t["nonzero"], t["zero_count"])
    assert layer.weight.dtype == torch.float16 and layer.weight.is_cuda
    assert H.words_hash(_words(layer.weight).view(np.float16)) == t["out_hash"]
    assert torch.equal(layer.bias, bias)
    outs, total = D.multi_resolution_analysis([torch.from_numpy(_inputs(call)[0])], call["wavelet"], call["level"],
                                              call["pct"], verbose=False)
    assert outs[0].dtype == torch.float16 and not outs[0].is_cuda and total == t["zero_count"]
    assert H.words_hash(_words(outs[0]).view(np.float16)) == t["out_hash"]


def test_dtype_errors(eng):
    """mixed dtypes, bfloat16 and float64 are TypeErrors; so is float16 into the sweeps, flatten,
    the threshold function and the absolute-threshold module; outs must be float16 too"""
    from wavelettransforms_amd import dwt_pruning as D
    from wavelettransforms_amd import dwt_pruning_NoEntropy as DN
    h = torch.zeros(4, 4, dtype=torch.float16, device="cuda")
    f = torch.zeros(4, 4, device="cuda")
    for bad in ([h, f], [f, h], [h, h.bfloat16()], [h.bfloat16()], [f.double()], [h, f.double()]):
        with pytest.raises(TypeError):
            eng.prune(bad, "haar", 1, 50.0)
        with pytest.raises(TypeError):
            D.multi_resolution_analysis(bad, "haar", 1, 50.0, verbose=False)
    with pytest.raises(TypeError, match="float16 CUDA tensor"):
        eng.prune([h], "haar", 1, 50.0, outs=[f])
    with pytest.raises(TypeError, match="float32 CUDA tensor"):
        eng.prune([f], "haar", 1, 50.0, outs=[h])
    with pytest.raises(TypeError):
        eng.prune([h], "haar", 1, 50.0, flatten=True)
    with pytest.raises(TypeError):
        D.multi_resolution_analysis([h], "haar", 1, 50.0, flatten=True, verbose=False)
    with pytest.raises(TypeError):
        D.multi_resolution_analysis_sweep([h], "haar", 1, [50.0, 90.0])
    with pytest.raises(TypeError):
        eng.prune_sweep([h], "haar", 1, [50.0])
    with pytest.raises(TypeError):
        D.percentile_based_thresholding(h, 50)
    with pytest.raises(TypeError):
        eng.prune_abs([h], "haar", 1, 0.01)
    with pytest.raises(TypeError):
        eng.prune_abs_sweep([h], "haar", 1, [0.01])
    with pytest.raises(TypeError):
        DN.multi_resolution_analysis([h], "haar", 1, 0.01)
    with pytest.raises(TypeError):
        eng.min_prune([h], 0.5)


# ---- +-inf and NaN in tensors that get no transform, against half_ref.kind_b_ref ----

SPECIAL_PCTS = [0.0, 50.0, 61.8, 100.0]
BIG_N = 41145  # odd; at an odd element offset: 7 head words, three blocks of vectors, 2 tail words


def _check_special(eng, words, o, r, pct, eff_level, tag):
    """one kind-B tensor against the restated NumPy rule: words exactly, thr64, the compare value
    and the maximum by special_values.assert_same_bits, counts and level exactly"""
    ref = H.kind_b_ref(words, pct)
    got = _words(o)
    assert o.dtype == torch.float16 and np.array_equal(got, ref["out"]), (tag, np.flatnonzero(got != ref["out"])[:5])
    SV.assert_same_bits(np.float64(r["thr64"]), ref["thr64"], (tag, "thr64"))
    SV.assert_same_bits(SV.f32_from_bits(r["thr32_bits"]), ref["cmp"].astype(np.float32), (tag, "thr32"))
    SV.assert_same_bits(SV.f32_from_bits(r["max_abs_bits"]), ref["max"].astype(np.float32), (tag, "max_abs"))
    assert r["zero_count"] == ref["zero_count"], (tag, r["zero_count"], ref["zero_count"])
    assert r["eff_level"] == eff_level and r["coeff_numel"] == r["numel"] == words.size, (tag, r)
    assert r["path"] == eng.MODE_HALF, (tag, r)
    return ref


def _half_cuda(words, shape=None):
    t = torch.from_numpy(np.array(words, np.uint16).view(np.float16)).cuda()
    return t if shape is None else t.view(shape)


@pytest.mark.parametrize("pct", SPECIAL_PCTS)
def test_special_values_small_populations(eng, pct):
    """every population of half_ref.special_populations at 1, 2, 3 and 37 weights in one call (more
    than two tables), and (4, 4, 3, 3) under bior3.3 level 5, which the clamp leaves at level 0"""
    pops = [(name, w) for name, w in H.special_populations() if len(w) <= 37]
    assert len(pops) > 64 and {len(w) for _, w in pops} == {1, 2, 3, 37}
    xs = [_half_cuda(w) for _, w in pops]
    outs, recs = eng.prune(xs, "haar", 2, pct)
    for (name, w), x, o, r in zip(pops, xs, outs, recs):
        _check_special(eng, w, o, r, pct, 2, (name, pct))
        assert np.array_equal(_words(x), w), (name, "input untouched")
    b = H.base_words(144, 7)
    r50, r618 = H.np_ranks(144, 50.0)[0] + 1, H.np_ranks(144, 61.8)[0] + 1
    conv = [b, H.put(b, {71: H.SNAN}), H.infs_from_rank(b, 143), H.infs_from_rank(b, r50), H.infs_from_rank(b, r618),
            H.put(H.infs_from_rank(b, 140), {0: H.NEG_QNAN}), H.infs_from_rank(b, 0), H.infs_from_rank(b, 1)]
    xs = [_half_cuda(w, (4, 4, 3, 3)) for w in conv]
    outs, recs = eng.prune(xs, "bior3.3", 5, pct)
    for i, (w, o, r) in enumerate(zip(conv, outs, recs)):
        ref = _check_special(eng, w, o, r, pct, 0, ("conv", i, pct))
        assert list(o.shape) == [4, 4, 3, 3]
        if (i, pct) in ((3, 50.0), (7, 0.0)) or (i in (2, 3, 4) and pct == 100.0):
            assert np.isnan(ref["thr64"]), (i, pct)  # inf at rank lo + 1 at gamma 1/2 and 0; an infinite maximum
        if (i, pct) == (4, 61.8):
            assert ref["thr64"] == np.inf and ref["zero_count"] == r618, (i, pct)  # gamma 0.374


def _big_cases():
    """41 145 weights with one special word: element 0 (the scalar head of a tensor at an odd
    element offset), a word of the middle block's vector body, the last word of the scalar tail"""
    b = H.base_words(BIG_N, 11)
    head, body, last = 0, 7 + 8 * (2048 + 1000) + 3, BIG_N - 1
    cases = [b]
    for pos in (head, body, last):
        cases.append(H.put(b, {pos: [H.QNAN, H.SNAN, H.NEG_QNAN][len(cases) % 3]}))
        cases.append(H.put(b, {pos: H.NEG_INF if pos == body else H.INF}))
    return cases, (head, body, last)


@pytest.mark.parametrize("in_place", [False, True])
def test_special_values_in_head_body_and_tail(eng, in_place):
    """a NaN or an inf that one workgroup's histogram alone sees (block 0 takes the head and the
    tail, block 1 the middle vectors) reaches the tensor's maximum and threshold; out of place the
    output's phase differs from the input's and the mask walks word by word, in place it stores
    vectors"""
    cases, (head, body, last) = _big_cases()
    for pct in SPECIAL_PCTS:
        bufs = [torch.zeros(BIG_N + 16, dtype=torch.float16, device="cuda") for _ in cases]
        xs = []
        for buf, w in zip(bufs, cases):
            buf[1:1 + BIG_N] = _half_cuda(w)
            xs.append(buf[1:1 + BIG_N])
        assert all(x.data_ptr() % 16 == 2 for x in xs)
        sp = 7 + 8 * ((BIG_N - 7) // 8)
        assert (BIG_N - 7) // 8 > 2 * 16384 // 8 and sp <= last < BIG_N and 7 + 16384 <= body < 7 + 2 * 16384
        outs, recs = eng.prune(xs, "haar", 2, pct, outs=xs if in_place else None)
        for i, (w, x, o, r) in enumerate(zip(cases, xs, outs, recs)):
            ref = _check_special(eng, w, o, r, pct, 2, (i, pct, in_place))
            if in_place:
                assert o.data_ptr() == x.data_ptr()
            else:
                assert o.data_ptr() % 16 != 2 and np.array_equal(_words(x), w), (i, "input untouched")
            if i % 2 == 1:  # the NaN cases: the maximum and the threshold are NaN, nothing is pruned
                assert np.isnan(ref["max"]) and np.isnan(ref["thr64"]) and np.array_equal(ref["out"], w), i
            elif i:         # one inf: a finite threshold below the 100th percentile, NaN at it
                assert np.isinf(ref["max"]) and np.isnan(ref["thr64"]) == (pct == 100.0), (i, pct)
        for buf in bufs:
            assert not bool(buf[0]) and not bool(buf[1 + BIG_N:].any()), "words outside the tensor were written"


def _neighbours(eng, sizes, special, own, pct):
    """one call of 1-D tensors of `sizes`, those of `special` {index: function of the base words}
    holding special values: every tensor against the restated rule, those of `own` also against a
    call of their own"""
    ws = [H.base_words(n, 300 + i) for i, n in enumerate(sizes)]
    for i, f in special.items():
        ws[i] = f(ws[i])
    xs = [_half_cuda(w) for w in ws]
    outs, recs = eng.prune(xs, "haar", 2, pct, carry_level=False)
    for i, (w, o, r) in enumerate(zip(ws, outs, recs)):
        ref = _check_special(eng, w, o, r, pct, 2, (i, pct))
        if i not in special:
            assert np.isfinite(ref["thr64"]), i
    for i in own:
        assert i not in special
        o1, r1 = eng.prune([xs[i]], "haar", 2, pct, carry_level=False)
        assert np.array_equal(_words(outs[i]), _words(o1[0])) and recs[i] == r1[0], (i, pct, recs[i], r1[0])


@pytest.mark.parametrize("pct", SPECIAL_PCTS)
def test_special_tensors_leave_their_neighbours_alone(eng, pct):
    """eight tensors, numbers 2 and 5 with a NaN and an inf; 70 tensors (three tables), numbers 31,
    32 and 69 special: the ordinary ones come out as from a call of their own"""
    nan_and_inf = lambda w: H.put(H.infs_from_rank(w, len(w) - 1), {len(w) // 2: H.QNAN})  # noqa: E731
    top_inf = lambda w: H.infs_from_rank(w, len(w) - 1)  # noqa: E731
    _neighbours(eng, [37, 2000, 500, 144, 1000, 37, 3, 20000], {2: nan_and_inf, 5: top_inf}, [0, 1, 3, 4, 6, 7], pct)
    _neighbours(eng, [2 + i % 38 for i in range(70)], {31: nan_and_inf, 32: top_inf, 69: nan_and_inf},
                [0, 30, 33, 63, 64, 68], pct)

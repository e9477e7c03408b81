"""Early stores of the resident launch (k_resident, include/wtprune.h wtp_set_resident_early): a
shared segment's selector publishes the key range [lo, hi] of the ranks' buckets before the
threshold, and the segment's data workgroups store at once every wave-wide float4 store with no
key inside it.  Results must stay bit-equal to the C oracle (values, float64 threshold bits, zero
counts) with the early stores counted (mode 2) and off (mode 0); the counters say whether the
early path ran where it should and stayed off where no bound may be published."""
import warnings

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import golden_io as G
from tests.test_gpu_resident import _miss_input

pytestmark = pytest.mark.gpu

RES_CHUNK = 49152  # weights per resident workgroup (csrc/wtp_internal.h)
SHAPES = (RES_CHUNK + 5, 2 * RES_CHUNK, 3 * RES_CHUNK + 4099)
PCTS = (10.0, 38.2, 50.0, 78.60000000000001)
WAVELET, LEVEL = "db8", 5  # 1-D tensors: effective level 0


@pytest.fixture(scope="module")
def eng():
    from wavelettransforms_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    prev_r = engine.set_resident(True)
    prev_e = engine.set_resident_early(1)
    yield engine
    engine.set_resident_early(prev_e)
    engine.set_resident(prev_r)


def _values(n, seed):
    """iid normal x 0.05, ~2 % exact zeros, some -0.0"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.05).astype(np.float32)
    x[rng.integers(0, n, max(1, n // 50))] = 0.0
    x[rng.integers(0, n, max(1, n // 500))] = -0.0
    return x


@pytest.fixture(scope="module")
def shapes_host():
    """Per shape one array of n + 1 values: [:n] is the aligned tensor, [1:] the unaligned one."""
    return [_values(n + 1, 100 + i) for i, n in enumerate(SHAPES)]


@pytest.fixture(scope="module")
def shapes_refs(shapes_host):
    """(host input, oracle output, oracle record) per tensor and percentile, computed once."""
    refs = {}
    for pct in PCTS:
        row = []
        for h, n in zip(shapes_host, SHAPES):
            for xin in (h[:n], h[1:n + 1]):
                ref, rr = O.prune_tensor(xin.copy(), WAVELET, LEVEL, pct)
                row.append((xin, ref, rr))
        refs[pct] = row
    return refs


def _device_pairs(shapes_host):
    """The six device inputs (aligned, 4-byte-offset unaligned per shape) and matching outputs."""
    xs, outs = [], []
    for h, n in zip(shapes_host, SHAPES):
        base = torch.from_numpy(h).cuda()
        xs += [base[:n].clone(), base[1:n + 1]]
        outs += [torch.empty(n, dtype=torch.float32, device="cuda"),
                 torch.empty(n + 1, dtype=torch.float32, device="cuda")[1:]]
    return xs, outs


def _same(o, ref, r, rr, nan=False):
    assert np.array_equal(o.view(np.uint32), ref.view(np.uint32)) or (nan and np.array_equal(o, ref, equal_nan=True))
    assert r["zero_count"] == rr["zero_count"]
    assert G.f64_bits_equal(r["thr64"], rr["thr64"]) or (nan and np.isnan(r["thr64"]) and np.isnan(rr["thr64"]))


def _run(eng, mode, xs, pct, outs=None, wavelet=WAVELET, level=LEVEL):
    """One prune call in early-store mode `mode`; (outs on the host, records, (early, deferred))."""
    prev = eng.set_resident_early(mode)
    try:
        eng.resident_early_counts()  # clear
        outs, res = eng.prune(xs, wavelet, level, pct, outs=outs, carry_level=False)
        counts = eng.resident_early_counts()
    finally:
        eng.set_resident_early(prev)
    return [o.cpu().numpy() for o in outs], res, counts


def test_switch(eng):
    assert eng.set_resident_early(2) == 1
    assert eng.set_resident_early(0) == 2
    with pytest.raises(ValueError):
        eng.set_resident_early(3)
    assert eng.set_resident_early(True) == 0
    assert eng.set_resident_early(1) == 1


@pytest.mark.parametrize("pct", PCTS)
def test_shapes(eng, shapes_host, shapes_refs, pct):
    """Shared segments of 2, 2 and 4 workgroups, ragged, aligned and unaligned, in one call: the
    early path runs (count > 0), holds back at most 10 % of the wave stores (simulated 1-3.4 %:
    [lo, hi] is 1/1024 of the window), and both modes equal the oracle bit for bit."""
    xs, outs = _device_pairs(shapes_host)
    got = {}
    for mode in (2, 0):
        for o in outs:
            o.fill_(7.0)
        got[mode] = _run(eng, mode, xs, pct, outs=outs)
    for mode in (2, 0):
        o_h, res, _ = got[mode]
        for o, r, (_, ref, rr) in zip(o_h, res, shapes_refs[pct]):
            _same(o, ref, r, rr)
            assert r["path"] in (1, 2), r["path"]
    for a, b in zip(got[2][0], got[0][0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    early, deferred = got[2][2]
    print("pct %g: early %d deferred %d wave stores" % (pct, early, deferred))
    assert got[0][2] == (0, 0)
    assert early > 0
    assert deferred <= 0.10 * (early + deferred), (early, deferred)


def test_in_place_publishes_no_bound(eng, shapes_host, shapes_refs):
    xs, _ = _device_pairs(shapes_host)
    o_h, res, counts = _run(eng, 2, xs, 50.0, outs=xs)
    assert counts == (0, 0)
    for o, r, (_, ref, rr) in zip(o_h, res, shapes_refs[50.0]):
        _same(o, ref, r, rr)


def _no_bound_inputs():
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(100_000) * 0.05).astype(np.float32)
    nan = a.copy()
    nan[123] = np.nan
    inf = a.copy()  # inf-heavy: the ranks' buckets reach +inf
    inf[rng.random(100_000) < 0.6] = np.inf
    inf[99_000] = -np.inf
    return {"nan": (nan, 50.0), "inf": (inf, 50.0), "miss": (_miss_input(300_000, 3), 37.5)}


@pytest.mark.parametrize("name", ["nan", "inf", "miss"])
def test_no_bound_special_values(eng, name):
    """Inputs for which no bound may be published: a NaN (the threshold is NaN), +inf in the ranks'
    buckets, a window that misses the ranks.  The +inf input is inf-heavy (60 % of the values) on
    purpose: with only a couple of infs, as in test_gpu_resident.test_nan_and_inf, the ranks'
    buckets stay finite and the kernel's rule (hi < 0x7F800000) rightly allows the bound."""
    x, pct = _no_bound_inputs()[name]
    ref, rr = O.prune_tensor(x.copy(), WAVELET, LEVEL, pct)
    for mode in (2, 0):
        (o,), (r,), (early, _) = _run(eng, mode, [torch.from_numpy(x).cuda()], pct)
        _same(o, ref, r, rr, nan=True)
        assert early == 0 or r["path"] == 3, (name, mode, early, r["path"])
        if name == "nan":
            assert early == 0


@pytest.mark.parametrize("pct", [0.0, 100.0])
def test_no_bound_at_the_ends(eng, shapes_host, pct):
    """pct 0 (the window is open below and the ranks' bucket is the zeros: more keys than the
    selector stages) and pct 100 (the window is open above).  The kernel publishes a bound only for
    a window closed on both sides, so a small pct-100 segment whose open window still resolves
    (path 1) stores nothing early.  Each tensor in a call of its own: the counters are that
    tensor's."""
    for h, n in zip(shapes_host, SHAPES):
        x = h[:n]
        ref, rr = O.prune_tensor(x.copy(), WAVELET, LEVEL, pct)
        for mode in (2, 0):
            (o,), (r,), (early, _) = _run(eng, mode, [torch.from_numpy(x.copy()).cuda()], pct)
            _same(o, ref, r, rr)
            assert early == 0 or r["path"] == 3, (n, mode, early, r["path"])


def test_heavily_tied(eng):
    """Values rounded to 1/64: whole buckets of equal keys.  Correctness only."""
    rng = np.random.default_rng(13)
    x = (np.round(rng.standard_normal(4 * RES_CHUNK + 77) * 0.5 * 64) / 64).astype(np.float32)
    for pct in (10.0, 50.0, 78.60000000000001):
        ref, rr = O.prune_tensor(x.copy(), WAVELET, LEVEL, pct)
        for mode in (2, 0):
            (o,), (r,), _ = _run(eng, mode, [torch.from_numpy(x).cuda()], pct)
            _same(o, ref, r, rr)


STALE_PCTS = (50.0, 10.0, 78.60000000000001, 50.0)


def test_stale_state_eager(eng, shapes_host, shapes_refs):
    """The same tensors pruned four times back to back into the same outputs: a bound or threshold
    granule that survived a launch would store through the previous call's range."""
    xs, outs = _device_pairs(shapes_host)
    prev = eng.set_resident_early(2)
    try:
        for pct in STALE_PCTS:
            _, res = eng.prune(xs, WAVELET, LEVEL, pct, outs=outs, carry_level=False)
            for o, r, (_, ref, rr) in zip(outs, res, shapes_refs[pct]):
                _same(o.cpu().numpy(), ref, r, rr)
        assert eng.resident_early_counts()[0] > 0
    finally:
        eng.set_resident_early(prev)


def test_stale_state_graph(eng, shapes_host, shapes_refs):
    """The four calls inside ONE captured graph, replayed twice; every call's outputs are copied
    aside inside the graph."""
    xs, outs = _device_pairs(shapes_host)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up: the workspace exists before the capture
        eng.launch(xs, WAVELET, LEVEL, 50.0, outs=outs, carry_level=False, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    snaps, recs = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.cuda.graph(g, stream=s):
            for pct in STALE_PCTS:
                _, resd = eng.launch(xs, WAVELET, LEVEL, pct, outs=outs, carry_level=False)
                snaps.append([o.clone() for o in outs])
                recs.append(resd)
    for _ in range(2):
        for o in outs:
            o.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        for pct, snap, resd in zip(STALE_PCTS, snaps, recs):
            for o, r, (_, ref, rr) in zip(snap, eng.decode(resd, len(xs)), shapes_refs[pct]):
                _same(o.cpu().numpy(), ref, r, rr)


def test_timeout_out_of_place(eng, shapes_host, shapes_refs):
    """A 0 us wait bound, out of place: the launch never touches its inputs and flags the tensors
    whose waits timed out (their outputs may be partly written); engine.prune's re-run makes every
    output oracle-exact."""
    from wavelettransforms_amd import _native as N
    xs, outs = _device_pairs(shapes_host)
    hosts = [x.cpu().numpy().copy() for x in xs]
    prev = N.lib().wtp_set_resident_timeout_us(0)
    try:
        _, res = eng.launch(xs, WAVELET, LEVEL, 50.0, outs=outs, carry_level=False)
        torch.cuda.synchronize()
        bad = eng.fault_mask(res, len(xs))
        for x, h in zip(xs, hosts):
            assert np.array_equal(x.cpu().numpy().view(np.uint32), h.view(np.uint32))
        assert bad.any(), "a 0 us bound should fault the multi-workgroup segments"
        o2, recs = eng.prune(xs, WAVELET, LEVEL, 50.0, outs=outs, carry_level=False)
    finally:
        N.lib().wtp_set_resident_timeout_us(prev)
    for x, h, o, r, (_, ref, rr) in zip(xs, hosts, o2, recs, shapes_refs[50.0]):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), h.view(np.uint32))
        _same(o.cpu().numpy(), ref, r, rr)
        assert r["path"] != eng.MODE_FAULT

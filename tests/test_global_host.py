"""Host-side contract of the global percentile (include/wtprune.h: wtp_prune_global_f32,
wtp_global_workspace_size): the symbols, validation before any device work through the C ABI with
fake device pointers (every argument error of tests/test_sweep_host.py has its counterpart), the
workspace query, the 2^32 - 1 rule of the pool on descriptors alone, and the Python layer on an
empty list and on the dtypes it refuses.  No GPU: every call here fails validation, stops at its
workspace check, or only computes sizes."""
import ctypes

import pytest
import torch

from wavelettransforms_amd import _native as N
from wavelettransforms_amd import dwt_pruning as D
from wavelettransforms_amd import engine

CARRY, FLATTEN, NO_RESIDENT, THR_ONLY = 1, 2, 4, 16
FAKE = 0x10000


def _desc(shapes, fake=FAKE, out=None):
    arr = (N.WtpTensor * max(1, len(shapes)))()
    for d, shape in zip(arr, shapes):
        d.in_ = fake
        d.out = out          # ignored by this entry: NULL is fine
        d.ndim = len(shape)
        for j, s in enumerate(shape):
            d.shape[j] = s
    return arr


def _outs(npct, n, base=0x200000):
    return (ctypes.c_void_p * (npct * n))(*[base + 0x1000 * i for i in range(npct * n)])


def _call(shapes, pcts, wavelet=b"haar", level=2, flags=CARRY, outs="auto", desc=None, npct=None, res="auto"):
    L = N.lib()
    n = len(shapes)
    k = len(pcts) if npct is None else npct
    d = _desc(shapes) if desc is None else desc
    parr = (ctypes.c_double * max(1, len(pcts)))(*pcts) if pcts is not None else None
    if outs == "auto":
        outs = _outs(max(k, 1), max(n, 1))
    if res == "auto":
        res = ctypes.create_string_buffer(N.RESULT_BYTES * max(1, k * n))
    return L.wtp_prune_global_f32(d, n, L.wtp_wavelet_id(wavelet), level, parr, k, flags, outs, None, 0, res, None)


SHAPES = [(4, 2, 8, 8), (33,), (6, 6)]


def test_symbols_exported_and_declared():
    L = N.lib()
    for name in ("wtp_prune_global_f32", "wtp_global_workspace_size"):
        assert name in N.exported_symbols()
        assert getattr(L, name).argtypes is not None
    assert engine.MODE_GLOBAL == 7
    assert L.wtp_abi_version() == 1
    assert "multi_resolution_analysis_global" in D.__all__


def test_a_valid_call_reaches_its_workspace_check():
    assert _call(SHAPES, [10.0, 50.0, 100.0]) == N.WTP_EWORKSPACE
    assert "workspace too small" in N.last_error()
    assert _call(SHAPES, [50.0, 50.0, 0.0], flags=0) == N.WTP_EWORKSPACE          # duplicates, unsorted
    assert _call(SHAPES, [50.0], flags=CARRY | THR_ONLY, outs=None) == N.WTP_EWORKSPACE
    assert _call(SHAPES, [50.0] * 8) == N.WTP_EWORKSPACE


def test_argument_errors():
    L = N.lib()
    assert _call(SHAPES, [50.0], npct=0) == N.WTP_EARG
    assert _call(SHAPES, [50.0] * 9) == N.WTP_EARG
    assert _call(SHAPES, None, npct=1) == N.WTP_EARG
    for bad in (FLATTEN, NO_RESIDENT, CARRY | FLATTEN, 8, 32, THR_ONLY | 64):
        assert _call(SHAPES, [50.0], flags=bad) == N.WTP_EARG, bad
        assert "flags" in N.last_error()
    assert _call(SHAPES, [50.0], outs=None) == N.WTP_EARG                          # no outputs, not thresholds-only
    assert _call(SHAPES, [50.0], res=None) == N.WTP_EARG
    assert _call(SHAPES, [50.0], desc=_desc(SHAPES, fake=None)) == N.WTP_EARG
    assert L.wtp_last_error_tensor() == 0
    # a NULL output pointer of tensor 1 at percentile 1
    o = _outs(2, 3)
    o[1 * 3 + 1] = None
    assert _call(SHAPES, [10.0, 20.0], outs=o) == N.WTP_EARG and L.wtp_last_error_tensor() == 1
    assert _call(SHAPES, [10.0, 20.0], outs=o, flags=CARRY | THR_ONLY) == N.WTP_EWORKSPACE
    # two outputs of tensor 2 at the same address
    o = _outs(3, 3)
    o[2 * 3 + 2] = o[0 * 3 + 2]
    assert _call(SHAPES, [10.0, 20.0, 30.0], outs=o) == N.WTP_EARG and L.wtp_last_error_tensor() == 2
    assert "same buffer" in N.last_error()
    # one output may be the input
    o = _outs(2, 3)
    o[1 * 3 + 0] = FAKE
    assert _call(SHAPES, [10.0, 20.0], outs=o) == N.WTP_EWORKSPACE


@pytest.mark.parametrize("pcts", [[-0.001], [100.001], [float("nan")], [10.0, 50.0, 101.0, 90.0], [10.0, float("nan")]])
def test_bad_percentile_among_good_ones(pcts):
    assert _call(SHAPES, pcts) == N.WTP_EBADPCT
    assert N.lib().wtp_last_error_tensor() == 0
    assert "Percentiles must be in the range [0, 100]" in N.last_error()
    assert _call([], pcts) == N.WTP_EBADPCT


def test_everything_plan_tensors_rejects():
    L = N.lib()
    assert _call(SHAPES, [50.0], wavelet=b"nosuch") == N.WTP_EBADWAVELET and L.wtp_last_error_tensor() == 0
    assert _call([(33,)], [50.0], wavelet=b"nosuch") == N.WTP_EWORKSPACE        # no wavelet lookup for ndim < 2
    assert _call(SHAPES, [50.0], level=-1) == N.WTP_EBADLEVEL
    assert _call([(8, 8), (5, 8)], [50.0], level=1) == N.WTP_ECROP and L.wtp_last_error_tensor() == 1
    assert _call([(8, 8), (2, 3, 4, 5, 7)], [50.0], level=1) == N.WTP_ECROP
    assert _call([(2, 2, 5, 7)], [50.0], level=1) == N.WTP_EWORKSPACE           # a 4-D tensor is cropped
    d = _desc([(8, 8)])
    d[0].ndim = 9
    assert _call([(8, 8)], [50.0], desc=d) == N.WTP_EARG
    # the wavelet check comes before the percentile check, as in the reference
    assert _call(SHAPES, [101.0], wavelet=b"nosuch") == N.WTP_EBADWAVELET
    # under the carry the clamp of the (3, 3) kernel holds for the odd 2-D tensor behind it
    # (bior3.3: level 0), without it the tensor runs at level 1 and cannot be cropped
    assert _call([(4, 2, 3, 3), (15, 16)], [50.0], wavelet=b"bior3.3", level=1, flags=CARRY) == N.WTP_EWORKSPACE
    assert _call([(4, 2, 3, 3), (15, 16)], [50.0], wavelet=b"bior3.3", level=1, flags=0) == N.WTP_ECROP


def test_an_empty_pool_is_answered_as_the_sweep_answers_it():
    """no tensors: WTP_OK, nothing written (no pointer is looked at); an empty tensor in the list:
    WTP_EEMPTY at that tensor, even when every tensor is empty -- the sweep's answers"""
    L = N.lib()
    assert _call([], [50.0]) == N.WTP_OK
    assert _call([], [50.0], outs=None, res=None) == N.WTP_OK
    assert _call([(8, 8), (0,)], [50.0]) == N.WTP_EEMPTY and L.wtp_last_error_tensor() == 1
    assert _call([(0,), (0, 3)], [50.0]) == N.WTP_EEMPTY and L.wtp_last_error_tensor() == 0
    assert _call([(4, 0, 3, 3)], [50.0]) == N.WTP_EEMPTY
    wid = L.wtp_wavelet_id(b"haar")
    for shapes in ([(8, 8), (0,)], [(0,), (0, 3)]):
        d, n = _desc(shapes), len(shapes)
        parr = (ctypes.c_double * 1)(50.0)
        res = ctypes.create_string_buffer(N.RESULT_BYTES * n)
        assert L.wtp_prune_sweep_f32(d, n, wid, 2, parr, 1, CARRY, _outs(1, n), None, 0, res, None) == N.WTP_EEMPTY
        assert L.wtp_global_workspace_size(d, n, wid, 2, 1, CARRY) == 0
    assert L.wtp_prune_sweep_f32(_desc([]), 0, wid, 2, (ctypes.c_double * 1)(50.0), 1, CARRY, None, None, 0, None,
                                 None) == N.WTP_OK


def test_workspace_query():
    L = N.lib()
    wid = L.wtp_wavelet_id(b"haar")
    d = _desc(SHAPES)
    q = lambda npct, flags=CARRY, desc=d, n=3, w=wid, lvl=2: L.wtp_global_workspace_size(desc, n, w, lvl, npct, flags)
    sizes = [q(k) for k in range(1, 9)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    assert q(1, CARRY | THR_ONLY) > 0
    assert q(0) == 0 and q(9) == 0 and q(-1) == 0
    for bad in (FLATTEN, NO_RESIDENT, 8, 32):
        assert q(1, bad) == 0
    assert q(1, w=-1) == 0 and q(1, lvl=-1) == 0 and q(1, n=-1) == 0
    assert L.wtp_global_workspace_size(None, 1, wid, 2, 1, CARRY) == 0
    assert q(1, desc=_desc([(8, 8), (0,)]), n=2) == 0
    assert q(1, desc=_desc([(5, 8)]), n=1, lvl=1) == 0
    one_d = _desc([(5,), (4099,)])
    assert q(1, desc=one_d, n=2, w=-1) > 0 and q(8, desc=one_d, n=2, w=-1) >= q(1, desc=one_d, n=2, w=-1)
    # the transformed tensors' packed arrays are in it
    big = _desc([(64, 64)])
    assert q(1, desc=big, n=1) - q(1, desc=big, n=1, lvl=0) >= 64 * 64 * 4
    # one state and one set of histograms whatever the tensor count: thirty 1-D tensors cost thirty
    # threshold-table words more than one, not thirty histograms (the sweep's do)
    many = _desc([(5,)] * 30)
    assert q(1, desc=many, n=30, w=-1) - q(1, desc=_desc([(5,)]), n=1, w=-1) < 4096
    assert L.wtp_sweep_workspace_size(many, 30, -1, 2, 1, CARRY) > 30 * (2048 + 2 * 16 * 1024) * 4


def test_the_pool_holds_at_most_2_32_minus_1_keys():
    """descriptors only, nothing allocated"""
    L = N.lib()
    big = 2 ** 31 - 1
    # a tensor of 2^31 keys is refused on its own (the per-tensor rule of every entry) ...
    assert _call([(2 ** 31,), (2 ** 31,)], [50.0]) == N.WTP_EARG
    # ... three of 2^31 - 1 pass it and overflow the pool: the message names the count
    assert _call([(big,), (big,), (big,)], [50.0]) == N.WTP_EARG
    assert str(3 * big) in N.last_error() and "2^32-1" in N.last_error() and L.wtp_last_error_tensor() == -1
    assert _call([(big,), (big,), (2,)], [50.0]) == N.WTP_EARG and str(2 ** 32) in N.last_error()
    # 2^32 - 1 keys in all are accepted as far as the workspace check
    assert _call([(big,), (big,), (1,)], [50.0]) == N.WTP_EWORKSPACE
    assert _call([(big,), (big,), (1,)], [0.0, 100.0], flags=THR_ONLY, outs=None) == N.WTP_EWORKSPACE
    # packed arrays count with their padding zeros: 2-D tensors of 2^30 keys each
    four = [(32768, 32768)] * 4
    assert _call(four[:3], [50.0], level=1) == N.WTP_EWORKSPACE
    assert _call(four, [50.0], level=1) == N.WTP_EARG and str(2 ** 32) in N.last_error()
    wid = L.wtp_wavelet_id(b"haar")
    assert L.wtp_global_workspace_size(_desc([(big,), (big,), (1,)]), 3, wid, 2, 1, CARRY) > 0
    assert L.wtp_global_workspace_size(_desc([(big,), (big,), (2,)]), 3, wid, 2, 1, CARRY) == 0
    # the other percentile checks come first, where plan_tensors makes them
    assert _call([(big,), (big,), (big,)], [101.0]) == N.WTP_EBADPCT


def test_empty_list_through_python():
    outs, res = engine.launch_global([], "haar", 2, [10.0, 50.0])
    assert outs == [[], []] and res is None
    assert (outs, res) == engine.launch_sweep([], "haar", 2, [10.0, 50.0])
    outs, res = engine.launch_global([], "haar", 2, [10.0, 50.0], thresholds_only=True)
    assert outs is None and res is None
    assert engine.prune_global([], "haar", 2, [10.0, 50.0]) == ([[], []], [[], []])
    assert D.multi_resolution_analysis_global([], "haar", 2, [10.0, 50.0, 90.0]) == [([], 0)] * 3


class _OnGpu:
    """a tensor as the dtype check sees it, without a device: the check precedes any device work"""

    def __new__(cls, dtype):
        t = torch.zeros(4, dtype=dtype)

        class T(torch.Tensor):
            is_cuda = True
        return t.as_subclass(T)


@pytest.mark.parametrize("dtypes", [(torch.float16,), (torch.bfloat16,), (torch.float64,), (torch.float32, torch.float16),
                                    (torch.float16, torch.float32)])
def test_dtypes_other_than_float32_raise_type_error(dtypes):
    xs = [_OnGpu(dt) for dt in dtypes]
    with pytest.raises(TypeError):
        engine.launch_global(xs, "haar", 1, [50.0])
    with pytest.raises(TypeError):
        engine.prune_global(xs, "haar", 1, [50.0])
    with pytest.raises(TypeError):
        engine.launch_sweep(xs, "haar", 1, [50.0])

"""CPU checks of the absolute-threshold sweep entry (wtp_prune_abs_sweep_f32): the exports, the
validation table through the C ABI with null or dummy device pointers (validation happens before
any device work), the workspace contract and the engine's argument check.  No kernel runs."""
import ctypes

import pytest

from oracle import oracle as O
from tests import golden_io as G
from tests.test_abs_threshold_host import ABS_TABLE  # the ordinary entry's own table
from wavelettransforms_amd import _native as N

DUMMY = 0x1000  # a non-null "device pointer" that validation never dereferences


def _desc(shapes, out=None):
    arr = (N.WtpTensor * len(shapes))()
    for i, s in enumerate(shapes):
        arr[i].in_ = DUMMY
        arr[i].out = out  # ignored by the sweep entry
        arr[i].ndim = len(s)
        for j, v in enumerate(s):
            arr[i].shape[j] = v
    return arr


def _outs(n, nthr, edit=None):
    """nthr * n distinct dummy output pointers, threshold-major; edit(list) may spoil them"""
    ptrs = [DUMMY + 0x100 * (1 + k * n + t) for k in range(nthr) for t in range(n)]
    if edit:
        edit(ptrs)
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _thr(*vals):
    return (ctypes.c_double * max(1, len(vals)))(*vals)


def _call(shapes, wavelet, level, thrs, nthr=None, outs="default", edit=None):
    L = N.lib()
    wid = L.wtp_wavelet_id(wavelet.encode())
    nthr = len(thrs) if nthr is None else nthr
    o = _outs(len(shapes), max(nthr, 1), edit) if outs == "default" else outs
    return L.wtp_prune_abs_sweep_f32(_desc(shapes), len(shapes), wid, level, _thr(*thrs) if thrs is not None else None,
                                     nthr, o, None, 0, DUMMY, None)


def test_symbols_exported_and_declared():
    L = N.lib()
    declared = N.exported_symbols()
    for name in ("wtp_abs_sweep_workspace_size", "wtp_prune_abs_sweep_f32", "wtp_abs_workspace_size", "wtp_prune_abs_f32"):
        assert name in declared and hasattr(L, name)
    assert L.wtp_abi_version() == 1  # symbols only
    assert N.ABS_RESULT_BYTES == 48 and N.RESULT_BYTES == 48
    from wavelettransforms_amd import engine
    assert engine.WTP_ABS_SWEEP_MAX_THR == 8


@pytest.mark.parametrize("nthr", [1, 3, 8])
@pytest.mark.parametrize("shapes,wavelet,level,code", ABS_TABLE)
def test_everything_the_abs_entry_rejects(shapes, wavelet, level, code, nthr):
    L = N.lib()
    wid = L.wtp_wavelet_id(wavelet.encode())
    thrs = [0.5, 0.25, 0.5, 0.0, float("nan"), -1.0, float("inf"), 1e40][:nthr]
    size = L.wtp_abs_sweep_workspace_size(_desc(shapes), len(shapes), wid, level, nthr)
    rc = _call(shapes, wavelet, level, thrs)
    if code is None:
        # one plan behind both entries: the ordinary entry's workspace, whatever the number of thresholds
        assert size == L.wtp_abs_workspace_size(_desc(shapes, DUMMY), len(shapes), wid, level) > 0
        assert rc == N.WTP_EWORKSPACE  # valid request, no workspace given: the only complaint
        return
    assert size == 0
    assert rc == code
    assert L.wtp_last_error_tensor() == len(shapes) - 1
    assert N.last_error()
    # the same status and message as the ordinary entry
    msg = N.last_error()
    assert L.wtp_prune_abs_f32(_desc(shapes, DUMMY), len(shapes), wid, level, 0.5, None, 0, DUMMY, None) == code
    assert N.last_error() == msg


def test_threshold_count_and_pointer():
    shapes = [(4, 4, 3, 3), (16,)]
    for nthr in (0, 9, -1):
        assert _call(shapes, "haar", 1, [0.5] * 9, nthr=nthr) == N.WTP_EARG
        assert "1 to 8 thresholds" in N.last_error()
        L = N.lib()
        assert L.wtp_abs_sweep_workspace_size(_desc(shapes), 2, L.wtp_wavelet_id(b"haar"), 1, nthr) == 0
    assert _call(shapes, "haar", 1, None, nthr=2) == N.WTP_EARG
    assert _call(shapes, "haar", 1, [0.5, 0.5]) == N.WTP_EWORKSPACE  # thresholds may repeat


def test_output_pointers():
    shapes = [(4, 4, 3, 3), (16,), (33, 17)]
    n = len(shapes)
    L = N.lib()

    def null_out(p):
        p[1 * n + 2] = None
    assert _call(shapes, "haar", 1, [0.1, 0.2, 0.3], edit=null_out) == N.WTP_EARG
    assert L.wtp_last_error_tensor() == 2 and "null" in N.last_error()

    def dup_out(p):
        p[2 * n + 1] = p[0 * n + 1]
    assert _call(shapes, "haar", 1, [0.1, 0.2, 0.3], edit=dup_out) == N.WTP_EARG
    assert L.wtp_last_error_tensor() == 1 and "same buffer" in N.last_error()
    assert _call(shapes, "haar", 1, [0.1, 0.2], outs=None) == N.WTP_EARG

    def in_place(p):  # one output of a tensor may be its input
        p[1 * n + 0] = DUMMY
    assert _call(shapes, "haar", 1, [0.1, 0.2, 0.3], edit=in_place) == N.WTP_EWORKSPACE
    # an empty 1-D tensor needs no output
    shapes = [(0,), (4, 4, 3, 3)]

    def null_empty(p):
        p[0] = None
        p[2] = None
    assert _call(shapes, "haar", 1, [0.1, 0.2], edit=null_empty) == N.WTP_EWORKSPACE
    assert _call([(0,)], "haar", 1, [0.1, 0.2], outs=None) == N.WTP_EWORKSPACE


def test_null_input_is_rejected_whatever_out_is():
    L = N.lib()
    d = _desc([(4, 4, 3, 3)])
    d[0].in_ = None
    rc = L.wtp_prune_abs_sweep_f32(d, 1, L.wtp_wavelet_id(b"haar"), 1, _thr(0.5), 1, _outs(1, 1), None, 0, DUMMY, None)
    assert rc == N.WTP_EARG and L.wtp_last_error_tensor() == 0
    assert L.wtp_prune_abs_sweep_f32(None, 1, 0, 1, _thr(0.5), 1, _outs(1, 1), None, 0, DUMMY, None) == N.WTP_EARG
    assert L.wtp_prune_abs_sweep_f32(_desc([(4,)]), 1, 0, 1, _thr(0.5), 1, _outs(1, 1), None, 0, None, None) == N.WTP_EARG
    assert L.wtp_prune_abs_sweep_f32(None, 0, 0, 1, _thr(0.5), 1, None, None, 0, None, None) == N.WTP_OK


def test_workspace_contract():
    L = N.lib()
    wid = L.wtp_wavelet_id(b"bior3.3")

    def ws(shapes, nthr, level=5, w=wid):
        return L.wtp_abs_sweep_workspace_size(_desc(shapes), len(shapes), w, level, nthr)

    def ws_abs(shapes, level=5, w=wid):
        return L.wtp_abs_workspace_size(_desc(shapes, DUMMY), len(shapes), w, level)

    # tiny images stay on chip: the same few bytes whatever the batch and the number of thresholds
    small = ws([(8, 8, 3, 3)], 1)
    assert 0 < small <= 4096
    for nthr in (1, 2, 8):
        assert ws([(512, 512, 3, 3)], nthr) == small
        assert ws([(512, 512, 3, 3), (64, 3, 7, 7), (512,)], nthr) == small
        assert ws([s for _, s in G.W.RESNET18_CONVS], nthr) == small
    # chain tensors: the ordinary entry's (one packed array, read by every threshold's inverse)
    db8 = L.wtp_wavelet_id(b"db8")
    pr, pc = O.packed_shape(256, 256, 8)
    for nthr in (1, 8):
        assert ws([(256, 256)], nthr, 8, db8) == ws_abs([(256, 256)], 8, db8) >= 4 * pr * pc
        assert ws([(256, 256), (3, 3, 3, 3), (100, 100)], nthr, 8, db8) == ws_abs([(256, 256), (3, 3, 3, 3), (100, 100)], 8, db8)
    assert ws([(3, 2, 8, 9)], 3, 3) > ws([(3, 2, 8, 8)], 3, 3)
    # an invalid request has no size
    assert ws([(4, 4, 3, 3)], 0) == ws([(4, 4, 3, 3)], 9) == 0
    assert ws([(4, 4, 3, 3)], 2, 33) == ws([(4, 4, 3, 3)], 2, -1) == ws([(0, 3, 3)], 2) == 0
    assert ws([(4, 4, 3, 3)], 2, 1, L.wtp_wavelet_id(b"nosuch")) == 0
    assert L.wtp_abs_sweep_workspace_size(None, 1, wid, 1, 2) == 0


def test_engine_rejects_an_output_count_mismatch():
    """checked before the engine touches a device: no tensors, two thresholds, three output sets"""
    from wavelettransforms_amd import engine
    with pytest.raises(ValueError, match="3 output sets for 2 thresholds"):
        engine.launch_abs_sweep([], "haar", 1, [0.1, 0.2], outs=[[], [], []])
    with pytest.raises(ValueError, match="1 outputs for 0 tensors"):
        engine.launch_abs_sweep([], "haar", 1, [0.1], outs=[[None]])
    assert engine.prune_abs_sweep([], "haar", 1, [0.1, 0.2]) == ([[], []], [[], []])


def test_mirror_signature():
    import inspect

    from wavelettransforms_amd import dwt_pruning_NoEntropy as D
    assert "multi_resolution_analysis_sweep" in D.__all__
    assert list(inspect.signature(D.multi_resolution_analysis_sweep).parameters) == ["weights", "wavelet", "level",
                                                                                     "thresholds"]
    assert D.multi_resolution_analysis_sweep([], "haar", 1, [0.1, 0.2]) == [([], 0), ([], 0)]

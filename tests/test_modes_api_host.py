"""Host-side contract of the extension-mode entry points (include/wtprune.h): names, validation
before any device work, workspace queries, and the Python layer's exceptions.  No GPU: every call
here fails validation or only computes sizes."""
import ctypes

import pytest
import torch

from wavelettransforms_amd import _native as N
from wavelettransforms_amd import dwt_pruning as D
from wavelettransforms_amd import engine

FLATTEN = 2


def _desc(shapes, fake=0x10000):
    arr = (N.WtpTensor * len(shapes))()
    for d, shape in zip(arr, shapes):
        d.in_ = fake
        d.out = fake
        d.ndim = len(shape)
        for j, s in enumerate(shape):
            d.shape[j] = s
    return arr


def test_mode_ids():
    L = N.lib()
    names = ["periodization", "zero", "constant", "symmetric", "reflect", "periodic", "smooth", "antisymmetric",
             "antireflect"]
    for i, name in enumerate(names):
        assert L.wtp_mode_id(name.encode()) == i
        assert L.wtp_mode_name(i) == name.encode()
    for bad in (b"", b"Symmetric", b"sym", b"periodisation", b"zpd"):
        assert L.wtp_mode_id(bad) == -1
    assert L.wtp_mode_id(None) == -1 and L.wtp_mode_name(9) is None and L.wtp_mode_name(-1) is None
    assert L.wtp_abi_version() == 1
    assert engine.MODES == tuple(names[:6])


@pytest.mark.parametrize("mode", ["smooth", "antisymmetric", "antireflect"])
def test_unimplemented_modes_raise_not_implemented(mode):
    with pytest.raises(NotImplementedError):
        D.multi_resolution_analysis([torch.zeros(4, 4)], "haar", 1, 50.0, mode=mode)
    with pytest.raises(NotImplementedError):
        D.prune_layer_weights(torch.nn.Conv2d(2, 2, 3), "haar", 1, 50.0, mode=mode)
    L = N.lib()
    d = _desc([(4, 4)])
    assert L.wtp_prune_mode_f32(d, 1, L.wtp_wavelet_id(b"haar"), 1, 50.0, 0, L.wtp_mode_id(mode.encode()), None, 0,
                                None, None) == N.WTP_EARG
    assert L.wtp_workspace_size_mode(d, 1, L.wtp_wavelet_id(b"haar"), 1, 0, L.wtp_mode_id(mode.encode())) == 0


def test_unknown_mode_raises_pywts_value_error():
    with pytest.raises(ValueError, match=r"Unknown mode name 'foo'\."):
        D.multi_resolution_analysis([torch.zeros(4, 4)], "haar", 1, 50.0, mode="foo")
    with pytest.raises(ValueError, match="Unknown mode name"):
        D.multi_resolution_analysis([], "haar", 1, 50.0, mode="Symmetric")


def test_flatten_with_a_mode_is_earg():
    L = N.lib()
    d = _desc([(4, 4)])
    wid = L.wtp_wavelet_id(b"haar")
    res = ctypes.create_string_buffer(N.RESULT_BYTES)
    assert L.wtp_prune_mode_f32(d, 1, wid, 1, 50.0, FLATTEN, L.wtp_mode_id(b"symmetric"), None, 0, res, None) == N.WTP_EARG
    assert "periodization" in N.last_error()
    assert L.wtp_workspace_size_mode(d, 1, wid, 1, FLATTEN, L.wtp_mode_id(b"symmetric")) == 0
    assert L.wtp_workspace_size_mode(d, 1, wid, 1, FLATTEN, 0) == L.wtp_workspace_size_ex(d, 1, wid, 1, FLATTEN) > 0


@pytest.mark.parametrize("shape", [(5, 8), (8, 5), (7, 7), (3, 6, 7)])
def test_odd_2d_and_3d_tensors_are_ecrop(shape):
    """waverec2 returns H + (H odd) by W + (W odd); the reference's 4-index crop cannot cut a 2-D
    or 3-D tensor back"""
    L = N.lib()
    d = _desc([shape])
    wid = L.wtp_wavelet_id(b"haar")
    res = ctypes.create_string_buffer(N.RESULT_BYTES)
    for mode in (b"zero", b"constant", b"symmetric", b"reflect", b"periodic"):
        rc = L.wtp_prune_mode_f32(d, 1, wid, 1, 50.0, 0, L.wtp_mode_id(mode), None, 0, res, None)
        assert rc == N.WTP_ECROP and L.wtp_last_error_tensor() == 0
        assert L.wtp_workspace_size_mode(d, 1, wid, 1, 0, L.wtp_mode_id(mode)) == 0
    # even sides, or a clamp to level 0, are fine: the call gets as far as its workspace check
    for ok, wname in (((6, 8), b"haar"), ((5, 7), b"bior3.3")):
        d = _desc([ok])
        rc = L.wtp_prune_mode_f32(d, 1, L.wtp_wavelet_id(wname), 1, 50.0, 0, L.wtp_mode_id(b"symmetric"), None, 0, res, None)
        assert rc == N.WTP_EWORKSPACE


def test_workspace_size_mode():
    L = N.lib()
    wid = L.wtp_wavelet_id(b"db2")
    sym = L.wtp_mode_id(b"symmetric")
    d = _desc([(4, 3, 8, 8), (2, 2, 9, 9), (16, 40)])
    assert L.wtp_workspace_size_mode(d, 3, wid, 1, 0, sym) > 0
    assert L.wtp_workspace_size_mode(d, 3, wid, 1, 0, 0) == L.wtp_workspace_size_ex(d, 3, wid, 1, 0)
    # level 0 after the clamp: the same plan in every mode
    d0 = _desc([(4, 4, 3, 3)])
    b33 = L.wtp_wavelet_id(b"bior3.3")
    assert L.wtp_workspace_size_mode(d0, 1, b33, 5, 0, sym) == L.wtp_workspace_size_ex(d0, 1, b33, 5, 0)
    # invalid requests
    assert L.wtp_workspace_size_mode(d, 3, -1, 1, 0, sym) == 0          # unknown wavelet
    assert L.wtp_workspace_size_mode(d, 3, wid, -1, 0, sym) == 0         # negative level
    assert L.wtp_workspace_size_mode(d, 3, wid, 1, 0, 9) == 0            # unknown mode id
    assert L.wtp_workspace_size_mode(d, 3, wid, 1, 0, -1) == 0
    assert L.wtp_workspace_size_mode(d, 3, wid, 1, 64, sym) == 0         # unknown flag
    assert L.wtp_workspace_size_mode(None, 3, wid, 1, 0, sym) == 0
    assert L.wtp_workspace_size_mode(d, -1, wid, 1, 0, sym) == 0


def test_packed_shape_mode():
    L = N.lib()
    r, c = ctypes.c_int64(), ctypes.c_int64()
    sym = L.wtp_mode_id(b"symmetric")
    assert L.wtp_packed_shape_mode(8, 8, L.wtp_wavelet_id(b"db2"), 1, sym, ctypes.byref(r), ctypes.byref(c)) == 0
    assert (r.value, c.value) == (10, 10)
    assert L.wtp_packed_shape_mode(96, 100, L.wtp_wavelet_id(b"bior3.3"), 3, sym, ctypes.byref(r), ctypes.byref(c)) == 0
    assert (r.value, c.value) == (116, 119)  # 96 -> 51 -> 29 -> 18, 100 -> 53 -> 30 -> 18
    assert L.wtp_packed_shape_mode(7, 7, L.wtp_wavelet_id(b"haar"), 2, 0, ctypes.byref(r), ctypes.byref(c)) == 0
    assert (r.value, c.value) == (8, 8)
    assert L.wtp_packed_shape_mode(1, 4, L.wtp_wavelet_id(b"haar"), 1, L.wtp_mode_id(b"reflect"), ctypes.byref(r),
                                   ctypes.byref(c)) == N.WTP_EARG

"""CPU checks of the absolute-threshold entry (wtp_prune_abs_f32, ResNet/dwt_pruning_NoEntropy.py):
the exports, the validation table with null device pointers, the workspace contract, and the
committed PyWavelets goldens against the UNCHANGED C oracle at unclamped levels (the yardstick
the GPU tests use).  No kernel runs."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import golden_io as G
from wavelettransforms_amd import _native as N

ABS = json.load(open(os.path.join(G.GOLDEN, "abs_manifest.json")))
ARR = dict(np.load(os.path.join(G.GOLDEN, "abs_cases.npz")))


def _desc(shapes):
    arr = (N.WtpTensor * len(shapes))()
    for i, s in enumerate(shapes):
        arr[i].in_ = 0x1000
        arr[i].out = 0x1000
        arr[i].ndim = len(s)
        for j, v in enumerate(s):
            arr[i].shape[j] = v
    return arr


def test_symbols_exported_and_declared():
    L = N.lib()
    declared = N.exported_symbols()
    for name in ("wtp_abs_workspace_size", "wtp_prune_abs_f32"):
        assert name in declared and hasattr(L, name)
    assert L.wtp_abi_version() == 1
    assert N.ABS_RESULT_BYTES == 48
    assert N.RESULT_BYTES == 48  # wtp_result's layout is unchanged


# (shapes, wavelet, level, status or None for a valid request); the sweep entry takes the same rows
# (tests/test_abs_sweep_host.py)
ABS_TABLE = [
    ([(4, 4, 3, 3)], "nosuch", 1, N.WTP_EBADWAVELET),
    ([(16,)], "nosuch", 1, None),                          # ndim < 2 never looks the wavelet up
    ([(16,)], "haar", -1, None),                           # ... nor the level
    ([(4, 4, 3, 3)], "haar", -1, N.WTP_EBADLEVEL),
    ([(4, 4, 3, 3)], "haar", 33, N.WTP_EARG),
    ([(4, 4, 3, 3)], "haar", 32, None),
    ([(0, 4, 3, 3)], "haar", 1, N.WTP_EARG),               # empty ndim >= 2
    ([(0,)], "haar", 1, None),                             # empty 1-D: a no-op
    ([(33, 17)], "db4", 2, None),                          # no WTP_ECROP on this path
    ([(2, 2, 2, 18, 33)], "db2", 1, None),
    ([(4, 4, 3, 3)], "bior3.3", 5, None),                  # above dwt_max_level: not clamped, not an error
    ([(16,), (33, 17), (0, 5)], "db4", 2, N.WTP_EARG),     # the third tensor fails, index reported
]


@pytest.mark.parametrize("shapes,wavelet,level,code", ABS_TABLE)
def test_validation_before_any_device_work(shapes, wavelet, level, code):
    L = N.lib()
    wid = L.wtp_wavelet_id(wavelet.encode())
    d = _desc(shapes)
    if code is None:
        assert L.wtp_abs_workspace_size(d, len(shapes), wid, level) > 0
        # valid request, no workspace given: the only complaint is the workspace
        assert L.wtp_prune_abs_f32(d, len(shapes), wid, level, 0.5, None, 0, 0x1000, None) == N.WTP_EWORKSPACE
        return
    assert L.wtp_abs_workspace_size(d, len(shapes), wid, level) == 0
    rc = L.wtp_prune_abs_f32(d, len(shapes), wid, level, 0.5, None, 0, 0x1000, None)
    assert rc == code
    assert L.wtp_last_error_tensor() == len(shapes) - 1
    assert N.last_error()


def test_bad_level_message_is_pywts():
    L = N.lib()
    d = _desc([(4, 4, 3, 3)])
    assert L.wtp_prune_abs_f32(d, 1, L.wtp_wavelet_id(b"haar"), -2, 0.5, None, 0, 0x1000, None) == N.WTP_EBADLEVEL
    assert N.last_error() == "Level value of -2 is too low . Minimum level is 0."


def test_workspace_contract():
    L = N.lib()
    wid = L.wtp_wavelet_id(b"bior3.3")

    def ws(shapes, level=5, w=wid):
        return L.wtp_abs_workspace_size(_desc(shapes), len(shapes), w, level)

    # tiny images stay on chip: no packed array, no level temp, whatever the batch
    assert ws([(512, 512, 3, 3)]) == ws([(8, 8, 3, 3)]) > 0
    assert ws([(512, 512, 3, 3), (64, 3, 7, 7), (512,)]) == ws([(8, 8, 3, 3)])
    resnet = [s for _, s in G.W.RESNET18_CONVS]
    assert 0 < ws(resnet) < (1 << 20)
    # a larger tensor holds its packed array (and level temps) there
    db8 = L.wtp_wavelet_id(b"db8")
    pr, pc = O.packed_shape(256, 256, 8)
    assert ws([(256, 256)], 8, db8) >= 4 * pr * pc
    # the chain tensors of a call run one after another and share one region
    assert ws([(256, 256), (256, 256), (100, 100)], 8, db8) == ws([(256, 256)], 8, db8)
    # the tiny limit: 8 x 8 stays on chip, 8 x 9 does not
    assert ws([(3, 2, 8, 9)], 3) > ws([(3, 2, 8, 8)], 3)


def _oracle(x, wavelet, level, thr32):
    if x.ndim < 2:
        return np.where(np.abs(x) < thr32, np.float32(0), x)
    return O.waverec2_packed(O.wavedec2_packed(x, wavelet, level), x.shape, wavelet, level, thr32)


def test_goldens_equal_the_unchanged_oracle():
    """PyWavelets 1.1.1 at unclamped levels (lines shorter than the filter, odd shapes, non-tight
    packings) = oracle.wavedec2_packed -> threshold on load -> waverec2_packed, bit for bit."""
    assert ABS["pywt"] == "1.1.1" and ABS["numpy"].startswith("1.")
    assert len(ABS["cases"]) >= 100
    for name, rec in ABS["cases"].items():
        shape = tuple(rec["shape"])
        x = ARR[name + "/in"] if name + "/in" in ARR else G.W.synth_numpy(shape, *rec["synth"])
        thr32 = np.float32(rec["threshold"])
        assert int(thr32.view(np.uint32)) == rec["thr32_bits"]
        out = _oracle(x, rec["wavelet"], rec["level"], thr32)
        gold = ARR[name + "/out"]
        assert out.dtype == gold.dtype == np.float32 and out.shape == gold.shape == shape
        assert np.array_equal(out, gold), name
        assert G.canon_hash(out) == rec["out_hash"], name
        assert int(np.count_nonzero(x)) == rec["nonzero_in"] and int(np.count_nonzero(out)) == rec["nonzero_out"], name
        if len(shape) >= 2:
            assert list(O.packed_shape(shape[-2], shape[-1], rec["level"])) == rec["packed_shape"][-2:], name
            lib = N.lib()
            pr, pc = ctypes.c_int64(), ctypes.c_int64()
            assert lib.wtp_packed_shape(shape[-2], shape[-1], rec["level"], ctypes.byref(pr), ctypes.byref(pc)) == 0
            assert [pr.value, pc.value] == rec["packed_shape"][-2:], name


def test_special_goldens_pin_the_float32_compare():
    rec = ABS["cases"]["abs_special_1d"]
    x, out = ARR["abs_special_1d/in"], ARR["abs_special_1d/out"]
    assert rec["threshold"] == 0.7
    keep = x == np.float32(0.7)
    assert keep.sum() >= 2 and np.array_equal(out[keep], x[keep])      # float32(0.7) is not below 0.7
    assert (np.abs(x[keep].astype(np.float64)) < 0.7).all()            # ... a float64 compare would zero it
    assert rec["nonzero_in"] == int(np.count_nonzero(x)) == x.size - 2  # -0.0 and 0.0
    assert out[np.abs(x) < np.float32(1e-30)].tolist() == [0.0] * 4     # zeros and denormals


def test_mirror_module_signatures():
    import inspect

    from wavelettransforms_amd import dwt_pruning_NoEntropy as D
    assert list(inspect.signature(D.multi_resolution_analysis).parameters) == ["weights", "wavelet", "level",
                                                                               "threshold", "mode"]
    assert inspect.signature(D.multi_resolution_analysis).parameters["mode"].default == "periodization"
    assert list(inspect.signature(D.prune_layer_weights).parameters) == ["layer", "wavelet", "level", "threshold"]
    assert list(inspect.signature(D.wavelet_pruning).parameters) == ["model", "wavelet", "level", "threshold",
                                                                     "csv_path", "guid"]
    with pytest.raises(NotImplementedError):
        D.multi_resolution_analysis([], "haar", 1, 0.1, mode="symmetric")
    assert D.multi_resolution_analysis([], "haar", 1, 0.1) == ([], 0)

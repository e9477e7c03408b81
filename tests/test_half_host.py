"""Host-side contract of the float16 entry (include/wtprune.h wtp_workspace_size_f16 /
wtp_prune_f16) and of the Python layer's dtype rules.  No GPU: every call here fails validation,
stops at its workspace check or only computes sizes."""
import ctypes
import random

import pytest
import torch

from wavelettransforms_amd import _native as N
from wavelettransforms_amd import engine

CARRY, FLATTEN, NO_RESIDENT = 1, 2, 4


def _desc(shapes, fake=0x10000):
    arr = (N.WtpTensor * max(1, len(shapes)))()
    for d, shape in zip(arr, shapes):
        d.in_ = fake
        d.out = fake
        d.ndim = len(shape)
        for j, s in enumerate(shape):
            d.shape[j] = s
    return arr


def _res(n):
    return ctypes.create_string_buffer(N.RESULT_BYTES * max(1, n))


def _call16(L, shapes, wavelet, level, pct, flags=CARRY, mode=0, fake=0x10000):
    d = _desc(shapes, fake)
    rc = L.wtp_prune_f16(d, len(shapes), L.wtp_wavelet_id(wavelet), level, pct, flags, mode, None, 0, _res(len(shapes)), None)
    return rc, L.wtp_last_error_tensor()


def _call32(L, shapes, wavelet, level, pct, flags=CARRY, mode=0):
    d = _desc(shapes)
    rc = L.wtp_prune_mode_f32(d, len(shapes), L.wtp_wavelet_id(wavelet), level, pct, flags, mode, None, 0,
                              _res(len(shapes)), None)
    return rc, L.wtp_last_error_tensor()


VALID = [
    ([(37,)], b"haar", 2),
    ([(4, 4, 3, 3)], b"bior3.3", 5),
    ([(8, 4, 3, 3)], b"haar", 1),
    ([(4, 3, 16, 16), (11,), (8, 4, 3, 3), (2, 2, 5, 5), (6, 6)], b"haar", 3),
    ([(5, 13, 3, 211)], b"bior3.3", 5),
    ([(3,)], b"no-such-wavelet", 2),  # ndim < 2 never looks the wavelet up
]


@pytest.mark.parametrize("shapes,wavelet,level", VALID)
def test_workspace_size_of_valid_lists(shapes, wavelet, level):
    L = N.lib()
    wid = L.wtp_wavelet_id(wavelet)
    d = _desc(shapes)
    for flags in (0, CARRY, CARRY | NO_RESIDENT):
        for mode in (0, 3):
            nb = L.wtp_workspace_size_f16(d, len(shapes), wid, level, flags, mode)
            assert nb > 0 and nb % 256 == 0
            # the call validates, then stops at its workspace check: nothing ran
            rc = L.wtp_prune_f16(d, len(shapes), wid, level, 50.0, flags, mode, None, 0, _res(len(shapes)), None)
            assert rc == N.WTP_EWORKSPACE, N.last_error()
            assert str(nb) in N.last_error()
    assert L.wtp_prune_f16(None, 0, wid, level, 50.0, 0, 0, None, 0, None, None) == N.WTP_OK


def test_workspace_holds_the_inner_call_and_the_staging():
    """transformed tensors: the float32 call's workspace, one float32 staging word per weight and
    the float16 scratch; untransformed ones: 8 KB of histogram per tensor, whatever their size"""
    L = N.lib()
    haar = L.wtp_wavelet_id(b"haar")
    shapes = [(16, 8, 8, 8), (4, 3, 16, 16)]
    d = _desc(shapes)
    inner = L.wtp_workspace_size_mode(d, 2, haar, 2, CARRY, 0)
    nb = L.wtp_workspace_size_f16(d, 2, haar, 2, CARRY, 0)
    assert nb >= inner + 4 * (16 * 8 * 8 * 8 + 4 * 3 * 16 * 16)
    bior = L.wtp_wavelet_id(b"bior3.3")
    small = L.wtp_workspace_size_f16(_desc([(64, 3, 7, 7)]), 1, bior, 5, CARRY, 0)
    large = L.wtp_workspace_size_f16(_desc([(512, 512, 3, 3)]), 1, bior, 5, CARRY, 0)
    two = L.wtp_workspace_size_f16(_desc([(64, 3, 7, 7), (512, 512, 3, 3)]), 2, bior, 5, CARRY, 0)
    assert small == large and 8192 <= two - small < 16384


INVALID = [
    ([(4, 4)], b"nope", 1, 50.0, N.WTP_EBADWAVELET, 0),
    ([(37,), (4, 4)], b"nope", 1, 50.0, N.WTP_EBADWAVELET, 1),
    ([(37,), (4, 4)], b"nope", 1, 101.0, N.WTP_EBADPCT, 0),     # the 1-D tensor's percentile comes first
    ([(4, 4), (37,)], b"nope", 1, 101.0, N.WTP_EBADWAVELET, 0),  # the wavelet lookup comes first
    ([(4, 4)], b"haar", -1, 50.0, N.WTP_EBADLEVEL, 0),
    ([(4, 4)], b"haar", 1, -0.5, N.WTP_EBADPCT, 0),
    ([(4, 4)], b"haar", 1, float("nan"), N.WTP_EBADPCT, 0),
    ([(8, 4, 3, 3), (0,)], b"haar", 1, 50.0, N.WTP_EEMPTY, 1),
    ([(4, 0, 3, 3)], b"haar", 1, 50.0, N.WTP_EEMPTY, 0),
    ([(6, 6), (5, 8)], b"haar", 1, 50.0, N.WTP_ECROP, 1),
    ([(3, 6, 7)], b"haar", 1, 50.0, N.WTP_ECROP, 0),
]


@pytest.mark.parametrize("shapes,wavelet,level,pct,code,tensor", INVALID)
def test_error_codes_in_the_references_order(shapes, wavelet, level, pct, code, tensor):
    """the float32 entry's code and tensor for the same list, before any device work, and a
    workspace size of 0"""
    L = N.lib()
    for flags in (0, CARRY):
        assert _call16(L, shapes, wavelet, level, pct, flags) == (code, tensor)
        assert _call32(L, shapes, wavelet, level, pct, flags) == (code, tensor)
    if code != N.WTP_EBADPCT:  # the size query has no percentile
        assert L.wtp_workspace_size_f16(_desc(shapes), len(shapes), L.wtp_wavelet_id(wavelet), level, CARRY, 0) == 0


def test_flatten_bad_flags_bad_modes_and_pointers_are_earg():
    L = N.lib()
    d = _desc([(8, 8)])
    haar = L.wtp_wavelet_id(b"haar")
    for flags in (FLATTEN, FLATTEN | CARRY, 8, 16):
        assert L.wtp_prune_f16(d, 1, haar, 1, 50.0, flags, 0, None, 0, _res(1), None) == N.WTP_EARG
        assert L.wtp_workspace_size_f16(d, 1, haar, 1, flags, 0) == 0
    assert "float32" in (L.wtp_prune_f16(d, 1, haar, 1, 50.0, FLATTEN, 0, None, 0, _res(1), None), N.last_error())[1]
    for mode in (6, 7, 8, 9, -1):  # smooth, antisymmetric, antireflect, unknown ids
        assert L.wtp_prune_f16(d, 1, haar, 1, 50.0, 0, mode, None, 0, _res(1), None) == N.WTP_EARG
        assert L.wtp_workspace_size_f16(d, 1, haar, 1, 0, mode) == 0
    assert _call16(L, [(8, 8)], b"haar", 1, 50.0, fake=0x10001) == (N.WTP_EARG, 0)  # not 2-byte aligned
    assert "2-byte" in N.last_error()
    assert _call16(L, [(8, 8)], b"haar", 1, 50.0, fake=0x10002)[0] == N.WTP_EWORKSPACE  # 2-byte aligned is enough
    assert _call16(L, [(8, 8)], b"haar", 1, 50.0, fake=0) == (N.WTP_EARG, 0)  # null
    assert L.wtp_prune_f16(d, 1, haar, 1, 50.0, 0, 0, None, 0, None, None) == N.WTP_EARG  # no records
    assert L.wtp_prune_f16(d, -1, haar, 1, 50.0, 0, 0, None, 0, _res(1), None) == N.WTP_EARG
    assert L.wtp_workspace_size_f16(None, 1, haar, 1, 0, 0) == 0
    assert L.wtp_abi_version() == 1


def _levels(L, shapes, F, level, carry):
    """the effective level of every tensor, as dwt_pruning.py:64-65 carries it"""
    cur, out = level, []
    for s in shapes:
        if not carry:
            cur = level
        if len(s) >= 2:
            cur = min(cur, L.wtp_max_level(min(s[-2:]), F))
        out.append(cur)
    return out


def test_the_transformed_sublist_sees_the_same_levels():
    """Kind A (ndim >= 2, level >= 1) runs as a sub-list through the float32 entry.  Under the
    carry the sub-list's running levels must be the full list's: a 1-D tensor leaves the level
    alone and a level-0 tensor leaves every later tensor at level 0.  The library re-plans the
    sub-list on every call and refuses (size 0, WTP_EARG) when a level differs; here the property is
    restated from wtp_max_level over 300 random lists, and the library accepts every one of them."""
    L = N.lib()
    rng = random.Random(16)
    sides = [1, 2, 3, 4, 6, 8, 16, 32, 64]
    checked = 0
    for _ in range(300):
        wname = rng.choice([b"haar", b"db2", b"bior3.3", b"rbio2.2"])
        wid, F = L.wtp_wavelet_id(wname), L.wtp_dec_len(L.wtp_wavelet_id(wname))
        level = rng.randint(0, 5)
        shapes = []
        for _ in range(rng.randint(1, 8)):
            if rng.random() < 0.25:
                shapes.append((rng.randint(1, 40),))
            else:
                shapes.append((rng.randint(1, 3), rng.randint(1, 3), rng.choice(sides), rng.choice(sides)))
        for carry in (True, False):
            full = _levels(L, shapes, F, level, carry)
            kind_a = [i for i, s in enumerate(shapes) if len(s) >= 2 and full[i] >= 1]
            sub = _levels(L, [shapes[i] for i in kind_a], F, level, carry)
            assert sub == [full[i] for i in kind_a], (shapes, level, carry)
            d = _desc(shapes)
            flags = CARRY if carry else 0
            valid = L.wtp_workspace_size_mode(d, len(shapes), wid, level, flags, 0) > 0
            assert (L.wtp_workspace_size_f16(d, len(shapes), wid, level, flags, 0) > 0) == valid, (shapes, level, N.last_error())
            if valid:
                rc = L.wtp_prune_f16(d, len(shapes), wid, level, 50.0, flags, 0, None, 0, _res(len(shapes)), None)
                assert rc == N.WTP_EWORKSPACE, N.last_error()
                checked += bool(kind_a)
    assert checked >= 100


def test_dtype_rules_of_the_python_layer():
    """all float16 or all float32; bfloat16 and float64 never; float16 only where the entry takes it"""
    h, f = torch.zeros(4, 4, dtype=torch.float16), torch.zeros(4, 4)
    assert engine.list_dtype([h, h], allow_half=True) == torch.float16
    assert engine.list_dtype([f, f], allow_half=True) == torch.float32
    assert engine.list_dtype([h, h]) == torch.float32  # the sweeps, abs, flatten, threshold, ...
    engine.check_dtype(h, torch.float16)
    engine.check_dtype(f, torch.float32)
    with pytest.raises(TypeError, match="float32 weights only"):
        engine.check_dtype(h, engine.list_dtype([h]))
    for other in (f, torch.zeros(2, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.float64)):
        with pytest.raises(TypeError, match="float16 and"):
            engine.check_dtype(other, engine.list_dtype([h, other], allow_half=True))
    for bad in (torch.bfloat16, torch.float64):
        x = torch.zeros(2, dtype=bad)
        with pytest.raises(TypeError, match="float32 weights only"):
            engine.check_dtype(x, engine.list_dtype([x, x], allow_half=True))
    assert engine.MODE_HALF == 6

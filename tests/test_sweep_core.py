"""CPU check of the percentile sweep's selection (csrc/wt_sweep_core.h: the digit split, the rank
search, the slot assignment and the lerp that csrc/sweep.hip's kernels run, compiled for the host
in tests/native/sweepcore.cpp) against np.sort and the oracle's percentile: the reference's eight
percentiles, ties, special values, tiny populations, and constructed arrays that put the ranks on
both sides of a digit boundary, all into one slot, and into sixteen slots."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import golden_io as G
from tests.ref_helpers import np_ranks

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SO = os.path.join(BUILD, "libsweepcore.so")
EXE = os.path.join(BUILD, "sweepcore")
SRC = os.path.join(HERE, "native", "sweepcore.cpp")
CSRC = os.path.join(HERE, "..", "wavelettransforms_amd", "csrc")
REF_PCTS = [t * 100 for t in (0.1, 0.236, 0.382, 0.5, 0.618, 0.786, 0.9, 1.0)]  # main_pruning.py:186


def _stale(target):
    deps = [SRC, os.path.join(CSRC, "wt_sweep_core.h"), os.path.join(CSRC, "wt_dwt_core.h")]
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def core():
    os.makedirs(BUILD, exist_ok=True)
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    u32p, i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)
    L.sweep_core_select.argtypes = [u32p, ctypes.c_longlong, u32p, ctypes.c_int, u32p, i32p, u32p]
    L.sweep_core_thresholds.argtypes = [u32p, ctypes.c_longlong, u32p, i32p, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), i32p]
    L.sweep_core_digit.argtypes = [ctypes.c_uint32, ctypes.c_int]
    L.sweep_core_digit.restype = ctypes.c_uint32
    return L


def keys_of(x):
    return np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF))


def _u32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def select(core, keys, ranks):
    ranks = np.asarray(ranks, np.uint32)
    out = np.zeros(len(ranks), np.uint32)
    slots = (ctypes.c_int * 2)()
    mk = ctypes.c_uint32()
    assert core.sweep_core_select(_u32(keys), len(keys), _u32(ranks), len(ranks), _u32(out), slots, ctypes.byref(mk)) == 0
    return out, (slots[0], slots[1]), mk.value


def thresholds(core, keys, pcts):
    n, k = len(keys), len(pcts)
    rk = [np_ranks(n, p) for p in pcts]
    r0 = np.array([r[0] for r in rk], np.uint32)
    above = (ctypes.c_int * k)(*[r[1] for r in rk])
    gamma = (ctypes.c_double * k)(*[r[2] for r in rk])
    t64, t32, slots = (ctypes.c_double * k)(), (ctypes.c_float * k)(), (ctypes.c_int * 2)()
    assert core.sweep_core_thresholds(_u32(keys), n, _u32(r0), above, gamma, k, t64, t32, slots) == 0
    return list(t64), list(t32), (slots[0], slots[1])


def check(core, x, pcts):
    """The selected keys are np.sort's, the thresholds the oracle's, for `pcts` in one selection."""
    x = np.asarray(x, np.float32).reshape(-1)
    keys = keys_of(x)
    srt = np.sort(keys)
    ranks = []
    for p in pcts:
        r0, above, _ = np_ranks(len(keys), p)
        ranks += [r0, r0 if above else r0 + 1]
    got, slots, mk = select(core, keys, ranks)
    assert np.array_equal(got, srt[ranks]), (got, srt[ranks])
    assert mk == int(srt[-1])
    t64, t32, slots2 = thresholds(core, keys, pcts)
    assert slots2 == slots
    for p, a, b in zip(pcts, t64, t32):
        want, _ = O.percentile_abs(x, p)
        assert G.f64_bits_equal(a, want), (p, a, want)
        assert (math.isnan(b) and math.isnan(want)) or G.f32_bits(b) == G.f32_bits(np.float32(want)), (p, b, want)
    assert 1 <= slots[0] <= slots[1] <= len(ranks)
    return slots


def test_program_self_check():
    """The stand-alone program: 40 random populations against std::sort."""
    os.makedirs(BUILD, exist_ok=True)
    if _stale(EXE):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", EXE, SRC])
    out = subprocess.run([EXE], capture_output=True, text=True)
    assert out.returncode == 0 and "sweepcore: ok" in out.stdout, out.stdout + out.stderr


def test_digit_split_covers_the_key(core):
    for key in (0, 1, 0x3D4CCCCD, 0x7F800000, 0x7FC00000, 0x7FFFFFFF, 0x000FFFFF, 0x00100000):
        d = [core.sweep_core_digit(key, p) for p in (1, 2, 3)]
        assert d[0] < 2048 and d[1] < 1024 and d[2] < 1024
        assert (d[0] << 20) | (d[1] << 10) | d[2] == key


@pytest.mark.parametrize("n", [2079, 36864, 50000])
def test_reference_percentiles_on_weights(core, n):
    """N(0, 0.05^2)-like weights: the sixteen ranks fall into 8 to 9 top-digit buckets and 10 to 15
    21-bit prefixes (checked with NumPy on this data); at least 4 and at least 8 are asserted."""
    x = G.W.synth_numpy((n,), 81, n % 7, G.W.sigma_exponent(0.05))
    slots = check(core, x, REF_PCTS)
    assert slots[0] >= 4 and slots[1] >= 8, slots


def test_ties(core):
    pcts = [0, 10, 50, 90, 100]
    assert check(core, np.full(40000, 0.0371, np.float32), pcts) == (1, 1)
    rng = np.random.default_rng(5)
    four = np.array([0.01, -0.02, 0.5, -3.0], np.float32)[rng.integers(0, 4, 30011)]
    s = check(core, four, REF_PCTS)
    assert s[0] <= 4 and s[1] <= 4
    x = rng.standard_normal(20000).astype(np.float32)
    x[rng.random(20000) < 0.7] = 0.0
    check(core, x, REF_PCTS)
    check(core, x, pcts)


def test_special_values(core):
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(5000) * 0.05).astype(np.float32)
    x[:50] = -0.0
    x[50:100] = np.float32(1e-42)          # denormals
    x[100:110] = np.float32(-3e-45)
    x[110:113] = np.inf
    x[113] = -np.inf
    check(core, x, REF_PCTS)
    check(core, x, [0, 99.9, 100])
    y = x.copy()
    y[777] = np.nan
    t64, t32, _ = thresholds(core, keys_of(y), [0, 50, 100])
    assert all(math.isnan(v) for v in t64) and all(math.isnan(v) for v in t32)
    check(core, y, [0, 50, 100])


def test_tiny_populations(core):
    for x in ([0.25], [-0.5, 0.125], [0.0, -0.0], [3.0, 3.0]):
        check(core, np.array(x, np.float32), [0, 23.599999999999998, 50, 100])
        check(core, np.array(x, np.float32), REF_PCTS)


def boundary_array(second_digit):
    """1001 keys, the median ranks r0 = 500 and r0 + 1 = 501 on opposite sides of a top-digit
    (or second-digit) boundary: 501 keys just below it, 500 just above."""
    edge = 0x3D400000 if not second_digit else 0x3D4CCC00  # a multiple of 2^20 / of 2^10 only
    assert edge % (1 << 20) == 0 if not second_digit else (edge % (1 << 10) == 0 and edge % (1 << 20) != 0)
    lo = edge - 1 - np.arange(501, dtype=np.uint32) * 3
    hi = edge + np.arange(500, dtype=np.uint32) * 5
    keys = np.concatenate([lo, hi]).astype(np.uint32)
    np.random.default_rng(7).shuffle(keys)
    sign = (np.arange(keys.size, dtype=np.uint32) % 2) << np.uint32(31)
    return (keys | sign).view(np.float32)


def test_ranks_across_a_top_digit_boundary(core):
    x = boundary_array(False)
    srt = np.sort(keys_of(x))
    assert srt[500] >> 20 != srt[501] >> 20
    assert check(core, x, [50])[0] == 2
    check(core, x, [49.9, 50, 50.1, 100, 0])


def test_ranks_across_a_second_digit_boundary(core):
    x = boundary_array(True)
    srt = np.sort(keys_of(x))
    assert srt[500] >> 20 == srt[501] >> 20 and srt[500] >> 10 != srt[501] >> 10
    assert check(core, x, [50]) == (1, 2)
    check(core, x, [49.9, 50, 50.1, 100, 0])


def test_sixteen_ranks_in_one_bucket_every_pass(core):
    """keys that differ in the last digit only: one slot in pass 2 and one in pass 3"""
    keys = (np.uint32(0x3D4CCC00) + (np.arange(4000, dtype=np.uint32) % 1000)).astype(np.uint32)
    assert check(core, keys.view(np.float32), REF_PCTS) == (1, 1)


def test_sixteen_ranks_in_sixteen_buckets(core):
    """one key per top-digit bucket, eight percentiles whose r0 and r0 + 1 are all different keys"""
    keys = ((np.arange(16, dtype=np.uint32) + 900) << np.uint32(20)) | np.uint32(0x2A5)
    pcts = [100.0 * (2 * k + 0.5) / 15 for k in range(8)]  # vi = 2k + 0.5: ranks 2k and 2k + 1
    assert [np_ranks(16, p)[0] for p in pcts] == [0, 2, 4, 6, 8, 10, 12, 14]
    assert check(core, keys.view(np.float32), pcts) == (16, 16)

"""CPU check of the global percentile's pooled selection (csrc/wt_global_core.h over
csrc/wt_sweep_core.h, compiled for the host in tests/native/globalcore.cpp): pools cut into pieces,
each piece histogrammed apart and flushed into one shared histogram as the workgroups of
csrc/global.hip do, give the keys of a sort of the concatenation and the oracle's percentile of it;
the pooled count and its 2^32 - 1 rule; which record field is whose.  The same header under
ASan + UBSan in a stand-alone program (tests/native/sanglobal.cpp)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import golden_io as G
from tests import test_sanitizers as S
from tests.ref_helpers import np_ranks
from tests.test_sweep_core import REF_PCTS, boundary_array, keys_of
from wavelettransforms_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SO = os.path.join(BUILD, "libglobalcore.so")
SRC = os.path.join(HERE, "native", "globalcore.cpp")
CSRC = os.path.join(HERE, "..", "wavelettransforms_amd", "csrc")


def _stale(target):
    deps = [SRC, os.path.join(HERE, "..", "include", "wtprune.h")] + [
        os.path.join(CSRC, h) for h in ("wt_global_core.h", "wt_sweep_core.h", "wt_dwt_core.h")]
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def core():
    os.makedirs(BUILD, exist_ok=True)
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    u32p, i32p, i64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
    f64p = ctypes.POINTER(ctypes.c_double)
    L.global_core_pool.argtypes = [i64p, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong)]
    L.global_core_select.argtypes = [u32p, i64p, ctypes.c_int, u32p, ctypes.c_int, u32p, i32p, u32p]
    L.global_core_thresholds.argtypes = [u32p, i64p, ctypes.c_int, u32p, i32p, f64p, ctypes.c_int, f64p,
                                         ctypes.POINTER(ctypes.c_float), u32p]
    L.global_core_record.argtypes = [ctypes.POINTER(N.WtpResult), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_uint32,
                                     ctypes.c_uint32]
    L.global_core_record.restype = ctypes.c_longlong
    return L


def _u32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _lens(pieces):
    return (ctypes.c_longlong * len(pieces))(*[len(p) for p in pieces])


def check_pool(core, pieces, pcts):
    """The pooled passes over `pieces` (float32 arrays) select np.sort's keys of the concatenation
    and give the oracle's percentile of it, for `pcts` in one selection."""
    pool = np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in pieces])
    keys = keys_of(pool)
    srt = np.sort(keys)
    n, k = len(keys), len(pcts)
    rk = [np_ranks(n, p) for p in pcts]
    ranks = []
    for r0, above, _ in rk:
        ranks += [r0, r0 if above else r0 + 1]
    ranks = np.asarray(ranks, np.uint32)
    got = np.zeros(len(ranks), np.uint32)
    slots, mk = (ctypes.c_int * 2)(), ctypes.c_uint32()
    assert core.global_core_select(_u32(keys), _lens(pieces), len(pieces), _u32(ranks), len(ranks), _u32(got), slots,
                                   ctypes.byref(mk)) == 0
    assert np.array_equal(got, srt[ranks]), (got, srt[ranks])
    assert mk.value == int(srt[-1])
    assert 1 <= slots[0] <= slots[1] <= len(ranks)
    r0 = np.array([r[0] for r in rk], np.uint32)
    above = (ctypes.c_int * k)(*[r[1] for r in rk])
    gamma = (ctypes.c_double * k)(*[r[2] for r in rk])
    t64, t32 = (ctypes.c_double * k)(), (ctypes.c_float * k)()
    assert core.global_core_thresholds(_u32(keys), _lens(pieces), len(pieces), _u32(r0), above, gamma, k, t64, t32,
                                       ctypes.byref(mk)) == 0
    for p, a, b in zip(pcts, t64, t32):
        want, mx = O.percentile_abs(pool, p)
        assert G.f64_bits_equal(a, want), (p, a, want)
        assert (math.isnan(b) and math.isnan(want)) or G.f32_bits(b) == G.f32_bits(np.float32(want)), (p, b, want)
    return (slots[0], slots[1])


def _split(rng, x, npieces):
    cuts = np.sort(rng.integers(0, len(x) + 1, npieces - 1))
    return np.split(x, cuts)


@pytest.mark.parametrize("seed", range(6))
def test_random_pools_in_1_to_30_pieces(core, seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 70000))
    kind = seed % 3
    if kind == 0:
        x = (rng.standard_normal(n) * 0.05).astype(np.float32)
    elif kind == 1:  # every bit pattern below the NaNs
        x = rng.integers(0, 0x7F800000, n, dtype=np.uint32).view(np.float32)
    else:            # 70 % zeros and a few values
        x = np.array([0.01, -0.02, 0.5, -3.0], np.float32)[rng.integers(0, 4, n)]
        x[rng.random(n) < 0.7] = 0.0
    for npieces in (1, int(rng.integers(2, 30)), 30):
        pieces = _split(rng, x, npieces)
        assert len(pieces) == npieces
        check_pool(core, pieces, REF_PCTS)
        check_pool(core, pieces, [0.0, 23.599999999999998, 50.0, 99.9, 100.0])


@pytest.mark.parametrize("second_digit", [False, True])
def test_boundary_heavy_keys_across_pieces(core, second_digit):
    """the median ranks on both sides of a digit boundary, the two sides in different pieces, in
    one piece, and scattered over thirty"""
    x = boundary_array(second_digit)
    order = np.argsort(keys_of(x), kind="stable")
    lo, hi = x[order[:501]], x[order[501:]]
    want = (2, 2) if not second_digit else (1, 2)
    for pieces in ([lo, hi], [hi, lo], [x], _split(np.random.default_rng(3), x, 30)):
        assert check_pool(core, pieces, [50]) == want
        check_pool(core, pieces, [49.9, 50, 50.1, 100, 0])
    # beside pieces of ordinary weights the boundary keys are a minority of the pool
    w = G.W.synth_numpy((5000,), 95, 1, G.W.sigma_exponent(0.05))
    check_pool(core, [w[:1234], lo, w[1234:], hi], REF_PCTS)


def test_ties_nan_and_tiny_pools(core):
    check_pool(core, [np.full(4000, 0.0371, np.float32), np.full(1, 0.0371, np.float32), np.zeros(70, np.float32)],
               [0, 10, 50, 90, 100])
    check_pool(core, [np.array([0.25], np.float32)], [0, 50, 100])
    check_pool(core, [np.array([-0.5], np.float32), np.array([0.125], np.float32)], REF_PCTS)
    x = (np.random.default_rng(9).standard_normal(3000) * 0.05).astype(np.float32)
    x[100:103] = np.inf
    check_pool(core, [x[:7], x[7:]], [0, 50, 99.99, 100])
    y = x.copy()
    y[2999] = np.nan  # a NaN in the last piece makes every threshold NaN
    check_pool(core, [y[:1500], y[1500:]], [0, 50, 100])


def test_pooled_count_and_the_overflow_rule(core):
    def pool(pops):
        t = ctypes.c_ulonglong()
        ok = core.global_core_pool((ctypes.c_longlong * max(1, len(pops)))(*pops), len(pops), ctypes.byref(t))
        return ok, t.value

    big = 2 ** 31 - 1
    assert pool([]) == (1, 0)
    assert pool([5, 0, 7]) == (1, 12)
    assert pool([big, big, 1]) == (1, 2 ** 32 - 1)
    assert pool([big, big, 2]) == (0, 2 ** 32)
    assert pool([2 ** 31, 2 ** 31]) == (0, 2 ** 32)
    assert pool([big] * 30) == (0, 30 * big)


def test_which_record_reads_what(core):
    npct, nt = 3, 4
    recs = (N.WtpResult * (npct * nt))()
    for k in range(npct):
        for t in range(nt):
            ri = core.global_core_record(recs, k, nt, t, 10 + t, 20 + t, t % 2, 0.25 * (k + 1), 0x3C000000 + k, 0x3F800000)
            assert ri == k * nt + t
    for k in range(npct):
        for t in range(nt):
            r = recs[k * nt + t]
            assert (r.numel, r.coeff_numel, r.eff_level, r.zero_count) == (10 + t, 20 + t, t % 2, 0)  # the tensor's own
            assert (r.thr64, r.thr32_bits, r.max_abs_bits) == (0.25 * (k + 1), 0x3C000000 + k, 0x3F800000)  # the pool's
            assert r.path == 7


@pytest.mark.timeout(600)
def test_global_core_asan_ubsan():
    out = S._build_and_run("g++", "sanglobal.cpp", "sanglobal", ["-std=c++17", "-ffp-contract=off"])
    assert "cases clean" in out

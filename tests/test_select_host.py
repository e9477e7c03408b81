"""CPU side of the selection's unit harness (tests/native/selcheck.hip): it cross-compiles for the
library's target, so a header change that breaks it is seen without a GPU; the bin functions
key_bin / bin_lo_key / bin_hi_key (__host__ __device__, csrc/wtp_internal.h) hold their round trip
and a numpy restatement through the harness's host entry; and the host builder of the state
k_collect leaves (the one tests/test_gpu_select_units.py feeds select_body) agrees with numpy."""
import numpy as np
import pytest

from tests import selcheck_shim as S
from tests.ref_helpers import SEL_NB
from tests.selcheck_shim import EDGE_KEYS, bins_checks, round_trip_keys

@pytest.fixture(scope="module")
def lib():
    return S.load()


def test_harness_cross_compiles(lib):
    assert S.const(lib, "NB") == SEL_NB
    assert not S.stale()


def test_bin_functions_host(lib):
    keys, lo0, hi0 = round_trip_keys()
    bin_ = np.zeros(len(keys), np.int32)
    lo, hi = np.zeros(SEL_NB, np.uint32), np.zeros(SEL_NB, np.uint32)
    lib.sc_bins_host(S.ptr(keys), len(keys), S.ptr(bin_), S.ptr(lo), S.ptr(hi))
    bins_checks(keys, bin_, lo, hi)
    e = len(EDGE_KEYS)
    assert np.array_equal(bin_[e:e + SEL_NB], np.arange(SEL_NB))            # key_bin(bin_lo_key(b)) == b
    assert np.array_equal(bin_[e + SEL_NB:e + 2 * SEL_NB], np.arange(SEL_NB))  # key_bin(bin_hi_key(b) - 1) == b


@pytest.mark.parametrize("nsub_log2,cap", [(6, 8), (10, 3)])
def test_host_state_builder(lib, nsub_log2, cap):
    rng = np.random.default_rng(nsub_log2)
    x = (rng.standard_normal(5000) * 0.05).astype(np.float32)
    x[:7] = 0.0
    keys = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    srt = np.sort(keys)
    kl, kh = int(srt[1000]), int(srt[3000])
    nsub = 1 << nsub_log2
    sums, sub, cand = np.zeros(5, np.int64), np.zeros(nsub, np.uint32), np.zeros(nsub * cap, np.uint32)
    assert lib.sc_build_state(S.ptr(x), len(x), kl, kh, nsub_log2, cap, S.ptr(sums), S.ptr(sub), S.ptr(cand)) == 0
    span_bits = int(kh - kl - 1).bit_length()
    sh = max(0, span_bits - nsub_log2)
    assert list(sums) == [int((keys < kl).sum()), int((keys == kl).sum()), int(keys.max()), 0, sh]
    inside = keys[(keys > kl) & (keys <= kh)].astype(np.int64)
    b = (inside - kl - 1) >> sh
    assert np.array_equal(sub, np.bincount(b, minlength=nsub))
    for j in range(nsub):
        want = inside[b == j][:cap]
        assert np.array_equal(cand[j * cap:j * cap + len(want)], want)

"""tests/native/selcheck.hip (the selection's device steps behind one wrapper each, and the host
builder of the state k_collect leaves) built as tests/_build/libselcheck.so with the library's own
compiler, target and parity flags, and loaded through ctypes: shared by tests/test_select_host.py
(the cross-compile, the host entries) and tests/test_gpu_select_units.py (every device step)."""
import ctypes
import glob
import os
import subprocess
import time

import numpy as np

from tests.ref_helpers import SEL_NB, np_key_bin
from wavelettransforms_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libselcheck.so")
SRC = os.path.join(HERE, "native", "selcheck.hip")
FLAGS = ["--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-ffp-contract=off"]
BUILD_SECONDS = None  # of this session's build, None when the library was up to date

_lib = None


def stale(so=SO, csrc=B.CSRC):
    deps = [SRC] + glob.glob(os.path.join(csrc, "*"))
    return not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps)


def compile_to(so, csrc=B.CSRC):
    """csrc: the directory the harness takes the selection's headers from (an edited copy: mutants)"""
    os.makedirs(os.path.dirname(so), exist_ok=True)
    tmp = so + ".tmp"
    subprocess.check_call([B.HIPCC] + FLAGS + ["-fPIC", "-shared", "-I" + os.path.abspath(csrc), "-o", tmp, SRC])
    os.replace(tmp, so)
    return so


def _p(t):
    return ctypes.POINTER(t)


def bind(path):
    # torch first, as wavelettransforms_amd/_native.py does: the harness's libamdhip64 dependency then
    # binds to the HIP runtime torch has loaded (one HIP runtime per process, whichever test runs first)
    import torch  # noqa: F401
    L = ctypes.CDLL(path)
    u32p, i32p, i64p, u64p, f32p = _p(ctypes.c_uint32), _p(ctypes.c_int), _p(ctypes.c_int64), _p(ctypes.c_uint64), _p(ctypes.c_float)
    i, i64, u32, dbl = ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_double
    L.sc_constant.argtypes = [ctypes.c_char_p]
    L.sc_bins_host.argtypes = [u32p, i, i32p, u32p, u32p]
    L.sc_bins_host.restype = None
    L.sc_bins.argtypes = [u32p, i, i32p, u32p, u32p]
    L.sc_wave_prims.argtypes = [u32p, u64p, i, u32p, u32p, u64p]
    L.sc_pick_digit.argtypes = [u32p, i64p, i, i32p, i64p]
    L.sc_find_bin.argtypes = [u32p, i32p, i, i32p]
    L.sc_find_bins_flat.argtypes = [u32p, i32p, i32p, i, i32p, i32p]
    L.sc_window.argtypes = [i, u32p, i64p, i, u32p]
    L.sc_wave_select.argtypes = [u32p, i, u32, u32, u32p]
    L.sc_select_in_range.argtypes = [u32p, i64, u32, u32, i64p, i, u32p]
    L.sc_block_hist.argtypes = [u32p, i, u32, i, i32p, i32p, i, u32p, u32p, i, i64p]
    L.sc_find_buckets.argtypes = [u32p, i, i64p, i, i32p, i64p]
    L.sc_build_state.argtypes = [f32p, i64, u32, u32, i, i, i64p, u32p, u32p]
    L.sc_select_body.argtypes = [f32p, i64, i64, i, dbl, i, i, i, u32, u32, i, i, i, i, f32p, i32p, i64p, _p(dbl), u32p, f32p]
    L.sc_collect_body.argtypes = [f32p, i, i, i, u32, u32, i, i, i64p, u32p, u32p]
    return L


def load():
    global _lib, BUILD_SECONDS
    if _lib is None:
        if stale():
            t0 = time.time()
            compile_to(SO)
            BUILD_SECONDS = time.time() - t0
        _lib = bind(SO)
    return _lib


def const(L, name):
    v = L.sc_constant(name.encode())
    assert v != -1, name
    return v


def ptr(a):
    """the ctypes pointer of a C-contiguous numpy array of one of the harness's element types"""
    t = {np.dtype(np.uint32): ctypes.c_uint32, np.dtype(np.int32): ctypes.c_int, np.dtype(np.int64): ctypes.c_int64,
         np.dtype(np.uint64): ctypes.c_uint64, np.dtype(np.float32): ctypes.c_float, np.dtype(np.float64): ctypes.c_double}[a.dtype]
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(t))


# 0, 1, the largest subnormal, either side of 2^-26 and of 2^6, the largest finite, inf, NaNs
EDGE_KEYS = np.array([0, 1, 0x007FFFFF, 0x327FFFFF, 0x32800000, 0x427FFFFF, 0x42800000, 0x7F7FFFFF, 0x7F800000,
                      0x7FC00000, 0x7FFFFFFF], np.uint32)


def bins_checks(keys, bin_, lo, hi):
    """what both the host and the device entry must satisfy"""
    NB = SEL_NB
    assert np.array_equal(bin_[:len(EDGE_KEYS)], np_key_bin(EDGE_KEYS)), (bin_[:len(EDGE_KEYS)], np_key_bin(EDGE_KEYS))
    assert list(bin_[:len(EDGE_KEYS)]) == [0, 1, 1, 1, 2, NB - 2, NB - 1, NB - 1, NB - 1, NB - 1, NB - 1]
    assert np.array_equal(bin_, np_key_bin(keys))
    assert np.all(np.diff(bin_[np.argsort(keys, kind="stable")]) >= 0)  # monotone in the key
    assert np.all(np.diff(lo.astype(np.int64)) > 0)  # bin_lo_key is increasing
    assert np.array_equal(hi[:-1], lo[1:]) and hi[-1] == 0xFFFFFFFF
    assert lo[0] == 0 and lo[1] == 1 and lo[2] == 0x32800000 and lo[NB - 1] == 0x42800000


def round_trip_keys():
    """EDGE_KEYS, then for every bin its lowest key and the key below the next bin's lowest, then random keys"""
    L = load()
    n = SEL_NB
    lo, hi, b = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(1, np.int32)
    L.sc_bins_host(ptr(np.zeros(1, np.uint32)), 1, ptr(b), ptr(lo), ptr(hi))
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 1 << 31, 4096, dtype=np.uint32)
    return np.ascontiguousarray(np.concatenate([EDGE_KEYS, lo, hi - np.uint32(1), rnd])), lo, hi

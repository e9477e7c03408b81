"""CPU check of the tiny-image kernel's per-image routine (csrc/wt_abs_core.h: abs_image, the
body of k_abs_tiny, compiled for the host here) against the oracle at unclamped levels: lines
shorter than the filter, every shape class up to 8 x 8, the arena layout at a lane stride."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libabscore.so")
CSRC = os.path.join(HERE, "..", "wavelettransforms_amd", "csrc")


@pytest.fixture(scope="module")
def core():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "native", "abscore.cpp")
    deps = [src, os.path.join(CSRC, "wt_abs_core.h"), os.path.join(CSRC, "wt_dwt_core.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, src])
    L = ctypes.CDLL(SO)
    fp = ctypes.POINTER(ctypes.c_float)
    L.abs_core_lanes_log2.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int]
    L.abs_core_run.argtypes = [fp, fp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, fp,
                               ctypes.c_float, ctypes.c_int]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def test_wrap_is_the_modulo(core):
    for m in (1, 2, 3, 4, 6, 8):
        for t in range(-128, 129):
            assert core.abs_core_mod(t, m) == t % m, (t, m)


def _oracle(x, wavelet, level, thr32):
    return O.waverec2_packed(O.wavedec2_packed(x, wavelet, level), x.shape, wavelet, level, thr32)


@pytest.mark.parametrize("wavelet", ["haar", "db2", "bior3.3", "rbio2.2", "db8", "sym11", "db20", "dmey", "coif17"])
def test_image_routine_matches_oracle(core, wavelet):
    rng = np.random.default_rng(11)
    taps = np.ascontiguousarray(O.filters(wavelet))
    F = taps.shape[1]
    shapes = [(h, w) for h in range(1, 9) for w in range(1, 9) if (h, w) in
              {(1, 1), (3, 3), (5, 5), (7, 7), (8, 8), (2, 3), (3, 2), (1, 8), (8, 1), (6, 5), (4, 7), (7, 8), (6, 6)}]
    for (h, w) in shapes:
        for level in (0, 1, 2, 5):
            x = rng.standard_normal((5, h, w)).astype(np.float32)
            thr32 = np.float32(0.6745)
            for nl in (1, 4):
                out = np.empty_like(x)
                words = core.abs_core_run(_p(x), _p(out), 5, h, w, level, F, _p(taps), thr32, nl)
                lg = core.abs_core_lanes_log2(h, w, level)
                assert lg >= 0 and (words << lg) <= core.abs_core_wave_words(), "the planner's lanes fit the arena"
                ref = _oracle(x, wavelet, level, thr32)
                assert np.array_equal(out, ref), (h, w, level, nl)


def test_planner_lane_choice(core):
    """abs_lanes_log2 is what plan_abs (csrc/host_methods.hip) calls: 64 images a wave while their areas
    fit the arena (16 KB less the wave's copy of the four filters), else the next power of two
    that fits; a side above 8 is not a tiny image."""
    assert core.abs_core_wave_words() == 4096 - 4 * 102 == 3688
    assert core.abs_core_lanes_log2(3, 3, 5) == 6      # 57 words: 3648 of 3688
    assert core.abs_core_lanes_log2(1, 1, 5) == 6
    assert core.abs_core_lanes_log2(3, 3, 6) == 5      # 60 words: 3840 do not fit
    assert core.abs_core_lanes_log2(7, 7, 5) == 4      # 198 words
    assert core.abs_core_lanes_log2(8, 8, 5) == 4
    assert core.abs_core_lanes_log2(8, 8, 0) == 5      # 64 words: 4096 do not fit beside the filters
    assert core.abs_core_lanes_log2(8, 8, 32) == 3     # 279 words
    assert core.abs_core_lanes_log2(8, 9, 3) == core.abs_core_lanes_log2(9, 8, 3) == -1
    for h in range(1, 9):
        for w in range(1, 9):
            for level in range(0, 33):
                lg = core.abs_core_lanes_log2(h, w, level)
                words = abs_words(h, w, level)
                assert lg >= 0 and (words << lg) <= 3688 and (lg == 6 or (words << (lg + 1)) > 3688)


def abs_words(h, w, level):
    """wt_abs_core.h's areas restated: image / approximation, two half transforms, coefficients"""
    if level == 0:
        return h * w
    r1, c1 = (h + 1) // 2, (w + 1) // 2
    words = max(h * w, 4 * r1 * c1) + 2 * r1 * max(w, 2 * c1)
    r, c = h, w
    for _ in range(level):
        r, c = (r + 1) // 2, (c + 1) // 2
        words += 3 * r * c
    return words + r * c


def test_level_32_fits_and_matches(core):
    """the deepest level the entry accepts: 8 x 8 needs 279 words, so a wave holds 8 images"""
    taps = np.ascontiguousarray(O.filters("bior3.3"))
    x = np.random.default_rng(3).standard_normal((3, 8, 8)).astype(np.float32)
    out = np.empty_like(x)
    words = core.abs_core_run(_p(x), _p(out), 3, 8, 8, 32, taps.shape[1], _p(taps), np.float32(0.5), 8)
    assert words == 279 == abs_words(8, 8, 32) and core.abs_core_lanes_log2(8, 8, 32) == 3
    ref = _oracle(x, "bior3.3", 32, np.float32(0.5))
    assert np.array_equal(out, ref)


def test_special_values(core):
    """a NaN threshold keeps everything, +inf zeroes every finite coefficient, and float32(0.7) is
    not below 0.7 rounded to float32 (level 0: the plain mask)"""
    taps = np.ascontiguousarray(O.filters("haar"))
    x = np.array([[[0.7, -0.7], [0.69999, -0.0]]], np.float32)
    out = np.empty_like(x)
    core.abs_core_run(_p(x), _p(out), 1, 2, 2, 0, 2, _p(taps), np.float32(0.7), 1)
    assert out.ravel().tolist() == [np.float32(0.7), np.float32(-0.7), 0.0, 0.0]
    core.abs_core_run(_p(x), _p(out), 1, 2, 2, 1, 2, _p(taps), np.float32("nan"), 1)
    assert np.array_equal(out, _oracle(x, "haar", 1, None))
    core.abs_core_run(_p(x), _p(out), 1, 2, 2, 1, 2, _p(taps), np.float32("inf"), 1)
    assert not out.any()

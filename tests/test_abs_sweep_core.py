"""CPU check of the absolute-threshold sweep's per-image routines (csrc/wt_abs_sweep_core.h:
abs_forward_raw and abs_inverse_masked, the body of k_abs_tiny_sweep, compiled for the host here):
ONE forward leaves the raw coefficients in the arena, then every threshold's inverse runs over
that same arena.  Each result must equal the oracle and abs_image run afresh; an implementation
that masks the coefficient area in place fails at the second threshold (+inf comes first and
would leave nothing).  The same source is built a second time as a stand-alone ASan + UBSan
program over an exactly sized arena."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_build")
SO = os.path.join(OUT, "libabssweepcore.so")
SRC = os.path.join(HERE, "native", "abssweepcore.cpp")
CSRC = os.path.join(HERE, "..", "wavelettransforms_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("wt_abs_sweep_core.h", "wt_abs_core.h", "wt_tiny_arena.h",
                                                "wt_dwt_core.h")]

THRS = np.array([np.inf, 0.3, np.nan, 0.6745, 0.3, 0.0], np.float32)  # in this order
SHAPES = [(1, 1), (3, 3), (5, 5), (7, 7), (8, 8), (2, 3), (3, 2), (1, 8), (8, 1), (6, 5), (4, 7), (7, 8), (6, 6)]


@pytest.fixture(scope="module")
def core():
    os.makedirs(OUT, exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    fp = ctypes.POINTER(ctypes.c_float)
    L.abs_sweep_core_run.argtypes = [fp, fp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     fp, fp, ctypes.c_int, ctypes.c_int]
    L.abs_sweep_core_image.argtypes = [fp, fp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, fp, ctypes.c_float, ctypes.c_int]
    L.abs_sweep_core_image.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _oracle(x, wavelet, level, thr32):
    return O.waverec2_packed(O.wavedec2_packed(x, wavelet, level), x.shape, wavelet, level, thr32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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


def _sweep(core, x, level, taps, nl, thrs=THRS):
    b, h, w = x.shape
    outs = np.full((len(thrs),) + x.shape, -55.0, np.float32)
    words = core.abs_sweep_core_run(_p(x), _p(outs), b, h, w, level, taps.shape[1], _p(taps), _p(thrs), len(thrs), nl)
    return outs, words


@pytest.mark.parametrize("wavelet", ["haar", "db2", "bior3.3", "rbio2.2", "db8", "sym11", "db20", "dmey", "coif17"])
def test_one_forward_then_every_threshold(core, wavelet):
    rng = np.random.default_rng(12)
    taps = np.ascontiguousarray(O.filters(wavelet))
    F = taps.shape[1]
    for (h, w) in SHAPES:
        for level in (0, 1, 2, 5):
            x = rng.standard_normal((5, h, w)).astype(np.float32)
            refs = {}
            for thr in THRS:  # the duplicate 0.3 shares its reference
                key = int(thr.view(np.uint32))
                if key not in refs:
                    refs[key] = _oracle(x, wavelet, level, thr)
            for nl in (1, 4):
                outs, words = _sweep(core, x, level, taps, nl)
                assert words == abs_words(h, w, level) == core.abs_sweep_core_words(h, w, level), "the arena does not grow"
                for k, thr in enumerate(THRS):
                    tag = (wavelet, h, w, level, nl, k, float(thr))
                    assert np.array_equal(_bits(outs[k]), _bits(refs[int(thr.view(np.uint32))])), tag
                    img = np.empty_like(x)
                    core.abs_sweep_core_image(_p(x), _p(img), 5, h, w, level, F, _p(taps), thr, nl)
                    assert np.array_equal(_bits(outs[k]), _bits(img)), tag
            if level:
                assert not refs[int(THRS[0].view(np.uint32))].any(), "+inf leaves nothing ..."
                assert refs[int(THRS[1].view(np.uint32))].any(), "... and the thresholds after it still see the coefficients"


def test_level_32_fits_and_matches(core):
    """the deepest level the entry accepts: 8 x 8 needs 279 words, so a wave holds 8 images"""
    taps = np.ascontiguousarray(O.filters("bior3.3"))
    x = np.random.default_rng(3).standard_normal((11, 8, 8)).astype(np.float32)
    outs, words = _sweep(core, x, 32, taps, 8)
    assert words == 279 == abs_words(8, 8, 32)
    for k, thr in enumerate(THRS):
        assert np.array_equal(_bits(outs[k]), _bits(_oracle(x, "bior3.3", 32, thr))), k


@pytest.mark.timeout(600)
def test_asan_ubsan_standalone(tmp_path):
    """the routines as a stand-alone program under ASan + UBSan (no Python in the process): the
    shape grid, levels 0, 1, 2, 5 and 32, NL 1 and 4, an arena of exactly abs_tiny_words * NL
    heap words, every threshold's result compared with abs_image run afresh"""
    exe = os.path.join(OUT, "abssweepcore_san")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-DABS_SWEEP_MAIN", "-o", exe, SRC])
    taps = np.ascontiguousarray(O.filters("bior3.3"), np.float32)
    tap_file = tmp_path / "taps.f32"
    taps.tofile(tap_file)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, str(tap_file), str(taps.shape[1])], capture_output=True, text=True, env=env, timeout=500)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "0 cases differ" in p.stdout
    # 5 images of every shape x 5 levels x 2 strides x 6 thresholds
    assert int(p.stdout.split()[3]) == sum(5 * h * w for h, w in SHAPES) * 5 * 2 * len(THRS)

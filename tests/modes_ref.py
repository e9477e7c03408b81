"""The extension modes' reference chain: the host build of the shared header
(tests/native/modescore.cpp, record 3) for the packed array, the oracle's percentile over it,
np.float32 of that threshold, and record 3 again with it.  tests/test_modes_ext_ref.py shows that
this chain reproduces every transformed tensor of the PyWavelets goldens (modes_manifest.json) bit
for bit, so it stands in for pywt at shapes that have no pywt golden
(tools/gen_golden_modes_ext.py).  Also the build / run plumbing of modescore for the CPU tests."""
import os
import subprocess

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "native", "modescore.cpp")
CSRC = os.path.join(HERE, "..", "wavelettransforms_amd", "csrc")
MODE_ID = {"periodization": 0, "zero": 1, "constant": 2, "symmetric": 3, "reflect": 4, "periodic": 5}
MODES = ["zero", "constant", "symmetric", "reflect", "periodic"]


def build(name="modescore", flags=("-O2",)):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("wt_modes_core.h", "wt_tiny_arena.h", "wt_dwt_core.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + list(flags) + ["-o", exe, SRC])
    return exe


def run(exe, words, tag):
    fin, fout = os.path.join(BUILD, tag + ".in"), os.path.join(BUILD, tag + ".out")
    np.concatenate([np.asarray(w).reshape(-1).view(np.uint32) for w in words]).tofile(fin)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")  # as tests/test_sanitizers.py
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    return np.fromfile(fout, np.uint32)


def ints(*v):
    return np.array(v, np.int32)


def lanes_log2(H, W, L, F):
    """wtm_tiny_lanes_log2 (record 4): log2 of the lanes a wave of k_mtiny_* gives the tensor's
    images, -1 when the tensor runs in the per-level kernels"""
    return int(run(build(), [ints(4, H, W, L, F)], "lanes").view(np.int32)[0])


def waves(B, lg):
    """the images each wave of a tiny tensor holds"""
    nl = 1 << lg
    return [min(nl, B - b0) for b0 in range(0, B, nl)]


def image_record(x, taps, L, mode, thr32):
    """the words of one record 3 and the (B, H, W) they describe"""
    H, Wd = x.shape[-2:]
    B = int(np.prod(x.shape[:-2], dtype=np.int64))
    words = [ints(3, MODE_ID[mode], taps.shape[1], B, H, Wd, L), np.array([thr32], np.float32), taps,
             np.ascontiguousarray(x, np.float32)]
    return words, (B, H, Wd)


def split_image(out, pos, x, B, H, Wd):
    """(packed, result, next position) of one record 3's output at word `pos`"""
    PR, PC = int(out[pos]), int(out[pos + 1])
    n = B * PR * PC
    packed = out[pos + 2:pos + 2 + n].view(np.float32).reshape(x.shape[:-2] + (PR, PC))
    res = out[pos + 2 + n:pos + 2 + n + B * H * Wd].view(np.float32).reshape(x.shape)
    return packed, res, pos + 2 + n + B * H * Wd


def core(x, wavelet, L, mode, thr32):
    """wavedec2 + coeffs_to_array of x (ndim >= 2) at level L >= 1 as given, np.where(|c| < thr32,
    0, c), waverec2 and the crop, by the shared header alone; returns (packed, out)"""
    x = np.ascontiguousarray(x, np.float32)
    words, (B, H, Wd) = image_record(x, O.filters(wavelet), L, mode, thr32)
    out = run(build(), words, "core")
    packed, res, pos = split_image(out, 0, x, B, H, Wd)
    assert pos == out.size
    return packed.copy(), res.copy()


def chain(x, wavelet, level, mode, pct):
    """One tensor of multi_resolution_analysis under `mode`; returns (packed, thr64, thr32,
    max_abs, out, eff_level).  The level is clamped as the reference clamps it; level 0 (and a
    tensor of fewer than two dimensions) is the same in every mode and goes through the oracle."""
    x = np.ascontiguousarray(x, np.float32)
    eff = level
    if x.ndim >= 2:
        eff = min(level, O.dwt_max_level(min(x.shape[-2:]), O.dec_len(wavelet)))
    if x.ndim < 2 or eff == 0:
        out, d, packed = O.prune_tensor(x, wavelet, 0, pct, want_coeffs=True)
        return packed, d["thr64"], np.float32(d["thr32"]), np.float32(d["max_abs"]), out, eff
    packed, _ = core(x, wavelet, eff, mode, 0.0)
    thr64, max_abs = O.percentile_abs(packed, pct)
    thr32 = np.float32(thr64)
    _, out = core(x, wavelet, eff, mode, thr32)
    return packed, thr64, thr32, np.float32(max_abs), out, eff

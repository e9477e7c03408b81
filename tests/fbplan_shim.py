"""tests/native/fbplan.cpp (csrc/fb_plan.h compiled for the host) built as a shared library and
loaded through ctypes: shared by tests/test_fb_plan.py and tests/test_interior_algebra.py."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_build", "libfbplan.so")
SRC = os.path.join(HERE, "native", "fbplan.cpp")
CSRC = os.path.join(ROOT, "wavelettransforms_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("fb_plan.h", "fb_index.h", "wt_dwt_core.h")]
FIXTURE = os.path.join(HERE, "golden", "fb_plan.json")

LW = 18  # numbers per launch (fbplan.cpp, FBP_LW)
GENERAL, INTERIOR, EDGE = 0, 1, 2
# csrc/wtp_internal.h: words per wave slot, and the items of one level a fused launch group holds
FSL_WORDS, SEG_PER_LAUNCH = 64, 24


def load_shim():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, SRC])
    lib = ctypes.CDLL(SO)
    i64, i32 = ctypes.c_int64, ctypes.c_int
    lib.fbp_tiled_ok.argtypes = [i64, i64, i64, i32]
    lib.fbp_fwd_interior.argtypes = [i32, i32, i32, i64, i32, ctypes.POINTER(i32)]
    lib.fbp_inv_interior.argtypes = [i32, i32, i32, i32, i64, i64, i32, ctypes.POINTER(i32)]
    lib.fbp_inv_axis.argtypes = [i32, i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.fbp_level.argtypes = [i32, i32, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), i32]
    lib.fbp_cover.argtypes = [i32, i32, i32, i32, ctypes.POINTER(i32), i32, i32, i32]
    return lib


def consts(lib):
    out = (ctypes.c_int64 * 32)()
    n = lib.fbp_consts(out)
    names = ["FB_THREADS", "FR", "FC", "IR", "IC", "FB_UNI", "FB_MAX_LDS", "FB_ONE_LAUNCH_TILES"]
    c = dict(zip(names, out[:len(names)]))
    c["spec"] = list(out[len(names):n])
    return c


def per_filter(lib, F):
    out = (ctypes.c_int64 * 10)()
    lib.fbp_filter(F, out)
    return dict(zip(["fwd_lds", "fwd_lds_alias", "fwd_int_lds", "inv_lds", "inv_lds_alias", "spec", "s0", "tp", "lhh",
                     "inv_win"], out))


def level(lib, d, F, mode, items):
    """The launches of one case: [(n, the LW numbers, item indices)]."""
    flat = [v for it in items for v in it]
    cap = 4 * (len(items) + 2) * (LW + 2 + len(items))
    out = (ctypes.c_int64 * cap)()
    nl = lib.fbp_level(d, F, mode, len(items), (ctypes.c_int64 * len(flat))(*flat), out, cap)
    assert nl >= 0
    res, o = [], 0
    for _ in range(nl):
        n = out[o]
        res.append((n, list(out[o + 1:o + 1 + LW]), list(out[o + 1 + LW:o + 1 + LW + n])))
        o += 1 + LW + n
    return res

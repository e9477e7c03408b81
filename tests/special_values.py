"""Special-value inputs for the transform paths and the one comparison rule they are held to (pure
NumPy; shared by tests/test_special_values_ref.py, tests/test_gpu_special_values.py, the k_small
kinds of tests/test_gpu_small.py and tools/gen_golden_special_modes.py).

cases(shape, seed, tid): the synthetic weights of W.synth_numpy at sigma 0.05 with blocks of +0.0
and -0.0, as a constant, scaled into the subnormals, scaled to max |x| = 2^126, with one NaN inside
an interior tile or at the corner that wraps to all four edges, with +inf on the repeated sample of
an odd extent and -inf inside, and scaled above / below the range of the fused window's bins.  The
positions are those of a (1, 2, 161, 464) tensor, scaled to the extent of other shapes.

assert_same_bits(got, ref, tag): identical NaN masks, and everywhere else identical words -- so the
sign of a zero counts, which np.array_equal (-0.0 == 0.0) does not see, and a NaN's payload does
not (x86 gives inf - inf the sign bit, the GPU does not; either is a NaN to everything after it).
"""
import hashlib

import numpy as np

from wavelettransforms_amd import workloads as W

SIGMA = 0.05
REF_H, REF_W = 161, 464  # the extent the positions below are written for
NAMES = ["zero_blocks", "constant", "subnormal", "huge", "nan_interior", "nan_corner", "infs", "scaled_up",
         "scaled_down"]
NEG_ZERO_BITS = 0x80000000
QNAN_BITS = 0x7FC00000


def plain(shape, seed, tid):
    """the unmodified base of every case"""
    return W.synth_numpy(tuple(shape), seed, tid, W.sigma_exponent(SIGMA))


def _r(shape, row):
    return row * shape[-2] // REF_H


def _c(shape, col):
    return col * shape[-1] // REF_W


def _images(x):
    """x as (images, H, W), a view; the second image is the first where there is only one"""
    v = x.reshape((-1,) + x.shape[-2:])
    return v, 0, 1 % v.shape[0]


def cases(shape, seed, tid):
    """{name: float32 array of `shape`} (ndim >= 2), every one built from plain(shape, seed, tid)"""
    shape = tuple(shape)
    base = plain(shape, seed, tid)
    H, Wd = shape[-2:]
    out = {}

    x = base.copy()
    v, i0, i1 = _images(x)
    v[i0, _r(shape, 20):_r(shape, 120), _c(shape, 60):_c(shape, 400)] = np.float32(0.0)
    v[i1, :_r(shape, 40), :] = np.float32(-0.0)
    v[i1, _r(shape, 100):, _c(shape, 200):] = np.float32(-0.0)
    out["zero_blocks"] = x

    out["constant"] = np.full(shape, 0.0371, np.float32)
    out["subnormal"] = base * np.float32(2.0 ** -126)
    b64 = base.astype(np.float64)
    out["huge"] = (b64 * (2.0 ** 126 / np.abs(b64).max())).astype(np.float32)

    x = base.copy()
    _images(x)[0][0, _r(shape, 70), _c(shape, 230)] = np.nan
    out["nan_interior"] = x

    x = base.copy()
    v, i0, i1 = _images(x)
    v[i1, 0, 0] = np.nan
    out["nan_corner"] = x

    x = base.copy()
    v, i0, i1 = _images(x)
    v[i0, H - 1, Wd - 1] = np.inf
    v[i1, _r(shape, 75), _c(shape, 100)] = -np.inf
    out["infs"] = x

    out["scaled_up"] = base * np.float32(2.0 ** 12)
    out["scaled_down"] = base * np.float32(2.0 ** -30)
    assert sorted(out) == sorted(NAMES) and all(a.dtype == np.float32 and a.shape == shape for a in out.values())
    return out


def neg_zero_words(a):
    """how many float32 words of `a` are -0.0"""
    return int((np.ascontiguousarray(a, np.float32).view(np.uint32) == NEG_ZERO_BITS).sum())


_WORD = {np.float16: np.uint16, np.float32: np.uint32, np.float64: np.uint64}


def assert_same_bits(got, ref, tag=""):
    """NaN masks identical; everywhere else the words are equal (float16, float32 or float64, any
    shape)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.dtype.type in _WORD, (tag, got.dtype, ref.dtype)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    if not np.array_equal(gn, rn):
        diff = np.argwhere(gn != rn)
        raise AssertionError("%r: NaN masks differ at %d cells (got %d NaN, want %d), first %s" % (
            tag, len(diff), int(gn.sum()), int(rn.sum()), tuple(diff[0])))
    u = _WORD[got.dtype.type]
    bad = (got.view(u) != ref.view(u)) & ~rn
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError("%r: %d of %d words differ, first at %s: got %r (%#x), want %r (%#x)" % (
            tag, int(bad.sum()), bad.size, k, got[k], int(got.view(u)[k]), ref[k], int(ref.view(u)[k])))


def f32_from_bits(bits):
    return np.array(bits, np.uint32).view(np.float32)


def canon_nan(a):
    """a float32 copy of `a` with every NaN the quiet pattern 0x7FC00000; zeros keep their sign"""
    a = np.array(a, dtype=np.float32, copy=True)
    a.view(np.uint32)[np.isnan(a)] = np.uint32(QNAN_BITS)
    return a


def bits_hash(a):
    """SHA-256 of canon_nan(a)'s words: equal hashes mean what assert_same_bits asserts"""
    return hashlib.sha256(canon_nan(a).tobytes()).hexdigest()


def assert_same_record(r, rr, tag=""):
    """A decoded wtp_result `r` against the oracle's record `rr`: the float64 threshold, its float32
    rounding and max |c| by assert_same_bits, the counts and the level exactly."""
    assert_same_bits(np.float64(r["thr64"]), np.float64(rr["thr64"]), (tag, "thr64"))
    assert_same_bits(f32_from_bits(r["thr32_bits"]), np.float32(rr["thr32"]), (tag, "thr32"))
    assert_same_bits(f32_from_bits(r["max_abs_bits"]), np.float32(rr["max_abs"]), (tag, "max_abs"))
    for f in ("zero_count", "eff_level", "coeff_numel"):
        assert r[f] == rr[f], (tag, f, r[f], rr[f])


# ---- float16 weights that get a transform (widened, the float32 path, narrowed once) ----

F16_NAMES = ["zero_blocks", "nan_interior", "nan_corner", "infs", "half_subnormal", "overflow"]
F16_SEED, F16_PCT = 97, 61.8
# (shape, wavelet, level), tensor id = position; the last is tiled.  tests/test_special_values_ref.py
# shows that the two scales below do at each what the cases are named for.
F16_SETTINGS = [((4, 3, 7, 7), "haar", 2), ((8, 4, 3, 3), "haar", 1), ((16, 40), "rbio2.2", 1),
                ((1, 2, 161, 464), "db8", 2)]
F16_SYMMETRIC = ((6, 5, 8, 8), "db2", 1)  # tensor id len(F16_SETTINGS), under the symmetric extension
HALF_SUBNORMAL_SCALE = 2.0 ** -16  # sigma 0.05 x 2^-16 = 7.6e-7: 12.5 steps of the half subnormals' 2^-24
OVERFLOW_MAX, OVERFLOW_SCALE = 60000.0, 2.0  # max |x| scaled to 2 x 60000, then clipped to +-60000
HALF_TINY = 2.0 ** -14  # the smallest normal half


def cases_f16(shape, seed, tid):
    """{name: float16 array}: cases() narrowed to float16, the base scaled so that most inputs are
    half subnormals, and the base scaled and clipped so that a share of the inputs sits at +-60000
    (every input finite) and the pruned reconstruction overshoots the largest half in places"""
    cs = cases(shape, seed, tid)
    out = {name: cs[name].astype(np.float16) for name in F16_NAMES[:4]}
    base = plain(shape, seed, tid)
    out["half_subnormal"] = (base * np.float32(HALF_SUBNORMAL_SCALE)).astype(np.float16)
    b64 = base.astype(np.float64) * (OVERFLOW_SCALE * OVERFLOW_MAX / np.abs(base.astype(np.float64)).max())
    out["overflow"] = np.clip(b64, -OVERFLOW_MAX, OVERFLOW_MAX).astype(np.float32).astype(np.float16)
    assert sorted(out) == sorted(F16_NAMES) and all(a.dtype == np.float16 and a.shape == tuple(shape) for a in out.values())
    return out

"""References and constants that more than one GPU test file needs: the absolute-threshold
method's yardstick and path ids (tests/test_gpu_abs_threshold.py, tests/test_gpu_special_values.py),
the reference of a transformed float16 tensor (tests/test_special_values_ref.py and the GPU file),
k_fwin's patch origins (tests/test_gpu_fused_select.py, tests/test_gpu_special_values.py), and
np.percentile's ranks and the selection's key bins (tests/test_sweep_core.py,
tests/test_select_host.py, tests/test_gpu_select_units.py)."""
import math

import numpy as np

from oracle import oracle as O

ABS_MASK, ABS_TINY, ABS_CHAIN = 0, 1, 2  # include/wtprune.h, the path of a wtp_abs_result


def abs_oracle(x, wavelet, level, thr):
    """The unchanged oracle as the yardstick (tests/test_abs_threshold_host.py pins it to the goldens)."""
    thr32 = np.float32(thr)
    if x.ndim < 2:
        return np.where(np.abs(x) < thr32, np.float32(0), x)
    return O.waverec2_packed(O.wavedec2_packed(x, wavelet, level), x.shape, wavelet, level, thr32)


def f16_transformed_ref(x16, wavelet, level, pct):
    """A float16 tensor that gets a transform (periodization): the oracle on the widened input,
    narrowed once; returns (float32 result, float16 result, the oracle's record with the zeros
    counted after the narrowing)."""
    with np.errstate(all="ignore"):
        out32, d = O.prune_tensor(x16.astype(np.float32), wavelet, level, pct)
        out16 = out32.astype(np.float16)
    return out32, out16, dict(d, zero_count=int((out16 == 0).sum()))


def patch_origins(R, C):
    """k_fwin's patch origins (csrc/select.inc): rows at 1/8, 3/8, 5/8, 7/8 and columns at 3/8,
    7/8, 1/8, 5/8 of the free range, FWIN_PS = 128"""
    return [((R - 128) * lr // 8, (C - 128) * lc // 8) for lr, lc in zip((1, 3, 5, 7), (3, 7, 1, 5))]


def np_ranks(n, pct):
    """np.percentile's two order statistics (NumPy 1.x, linear): (r0, above, gamma)."""
    vi = (n - 1) * (pct / 100.0)
    if vi >= n - 1:
        return n - 1, 1, vi + 1.0
    fl = math.floor(vi)
    return int(fl), 0, vi - fl


SEL_NB = 4099  # csrc/wtp_internal.h: zero, under, 32 octaves of 128 bins from 2^-26, over


def np_key_bin(keys):
    """The selection's bin of a key (the float32 bit pattern of |x|), stated on the float's value:
    0 for zero, 1 below 2^-26, the last bin from 2^6 up (inf and NaN included), else 2 + 128 *
    (octave above 2^-26) + the 128th of the octave the value lies in."""
    keys = np.asarray(keys, np.uint32)
    with np.errstate(invalid="ignore"):
        return _np_key_bin(keys)


def _np_key_bin(keys):
    f = keys.view(np.float32).astype(np.float64)
    out = np.empty(keys.shape, np.int64)
    nan = np.isnan(f)
    fin = np.where(nan, 1.0, f)
    m, e = np.frexp(fin)  # fin = m 2^e, m in [0.5, 1)
    inside = 2 + 128 * (e - 1 + 26) + np.floor((2.0 * m - 1.0) * 128.0).astype(np.int64)
    out[...] = inside
    out[fin < 2.0 ** -26] = 1
    out[keys == 0] = 0
    out[nan | (fin >= 2.0 ** 6)] = SEL_NB - 1
    return out

"""References and constants that more than one GPU test file needs: the absolute-threshold
method's yardstick and path ids (tests/test_gpu_abs_threshold.py, tests/test_gpu_special_values.py)
and k_fwin's patch origins (tests/test_gpu_fused_select.py, tests/test_gpu_special_values.py)."""
import numpy as np

from oracle import oracle as O

ABS_MASK, ABS_TINY, ABS_CHAIN = 0, 1, 2  # include/wtprune.h, the path of a wtp_abs_result


def abs_oracle(x, wavelet, level, thr):
    """The unchanged oracle as the yardstick (tests/test_abs_threshold_host.py pins it to the goldens)."""
    thr32 = np.float32(thr)
    if x.ndim < 2:
        return np.where(np.abs(x) < thr32, np.float32(0), x)
    return O.waverec2_packed(O.wavedec2_packed(x, wavelet, level), x.shape, wavelet, level, thr32)


def patch_origins(R, C):
    """k_fwin's patch origins (csrc/select.inc): rows at 1/8, 3/8, 5/8, 7/8 and columns at 3/8,
    7/8, 1/8, 5/8 of the free range, FWIN_PS = 128"""
    return [((R - 128) * lr // 8, (C - 128) * lc // 8) for lr, lc in zip((1, 3, 5, 7), (3, 7, 1, 5))]

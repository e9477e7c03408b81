"""An independent float64 check of the extension modes' shared header (csrc/wt_modes_core.h) at
every wavelet of the tap table, not only the five that have PyWavelets goldens: one analysis level
of a line (tests/native/modescore.cpp, record 1) against np.pad of the float64 line and np.convolve
with the taps, sampled at the odd sites.

The tolerance is derived, not measured: an output is F products and F - 1 additions in float32, so
its error is at most (F + 1) 2^-24 sum_j |f[j]| |x~[i - j]| to first order (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: gamma_F on the sum of magnitudes; the input and the
taps are float32 on both sides, so they add no error of their own).  Perfect reconstruction is not
asserted: dmey and some biorthogonal filters do not reconstruct exactly."""
import json
import os

import numpy as np

from oracle import oracle as O
from tests import modes_ref as R
from wavelettransforms_amd import workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
PAD = {"zero": "constant", "constant": "edge", "symmetric": "symmetric", "reflect": "reflect", "periodic": "wrap"}


def _lines():
    with open(os.path.join(HERE, "..", "wavelettransforms_amd", "wavelets.json")) as fh:
        names = sorted(json.load(fh)["wavelets"])
    e = W.sigma_exponent(0.05)
    for wi, name in enumerate(names):
        taps = O.filters(name)
        F = taps.shape[1]
        if F & 1:
            continue
        for mi, mode in enumerate(R.MODES):
            for N in sorted({1, 2, 3, 5, 8, 13, F - 1, F, 2 * F + 1}):
                if mode == "reflect" and N == 1:
                    continue  # undefined (wtm_line_ok)
                yield name, taps, F, mode, N, W.synth_numpy((N,), 3000 + mi, 1000 * wi + N, e)


def test_analysis_of_every_wavelet_against_float64():
    lines = list(_lines())
    assert len({l[0] for l in lines}) == 106 and len(lines) >= 4400
    words = []
    for name, taps, F, mode, N, x in lines:
        words += [R.ints(1, R.MODE_ID[mode], F, N), taps, x]
    out = R.run(R.build(), words, "f64")
    pos, worst, worst_at = 0, 0.0, None
    for name, taps, F, mode, N, x in lines:
        M = (N + F - 1) // 2
        assert int(out[pos]) == M, (name, mode, N)
        got = out[pos + 1:pos + 1 + 2 * M].view(np.float32).astype(np.float64).reshape(2, M)
        K = int(out[pos + 1 + 2 * M])
        assert K == 2 * M - F + 2
        pos += 2 + 2 * M + K
        xp = np.pad(x.astype(np.float64), F - 1, PAD[mode])
        sites = 2 * np.arange(M) + 1 + (F - 1)  # i = 2o + 1 of the line, in the padded line's full convolution
        for band in (0, 1):
            f = taps[band].astype(np.float64)
            ref = np.convolve(xp, f)[sites]
            bound = (F + 1) * 2.0 ** -24 * np.convolve(np.abs(xp), np.abs(f))[sites]
            err = np.abs(got[band] - ref)
            assert np.all(err <= bound), (name, mode, N, band, float((err / np.maximum(bound, 1e-300)).max()))
            nz = bound > 0
            if nz.any() and (err[nz] / bound[nz]).max() > worst:
                worst, worst_at = float((err[nz] / bound[nz]).max()), (name, mode, N, band)
    assert pos == out.size
    print("worst error / bound over %d lines: %.3f at %s" % (len(lines), worst, worst_at))

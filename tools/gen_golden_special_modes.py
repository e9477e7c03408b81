"""Golden fixture of the extension modes over the special-value cases of tests/special_values.py:
blocks of +0.0 and -0.0, subnormal input, one NaN at the corner, +inf and -inf, in the one-launch
tiny kernels (k_mtiny_*) and the per-level kernels (k_mdwt_* / k_midwt_*) of csrc/modes.hip.

Needs no PyWavelets: the expected values come from the reference chain of tests/modes_ref.py, as
tools/gen_golden_modes_ext.py takes them (tests/test_modes_ext_ref.py anchors that chain to pywt).
    python tools/gen_golden_special_modes.py

Writes tests/golden/special_modes_manifest.json and special_modes_cases.npz.  A record is one call
of engine.prune([x], wavelet, level, pct, carry_level=False, mode=mode) with x =
special_values.cases(shape, SEED, tid)[case].  The outputs are stored as arrays; the packed array
as the SHA-256 of its words (special_values.canon_nan / bits_hash, which the GPU test uses too).
Every NaN is set to the one quiet pattern 0x7FC00000 first (x86 gives inf - inf the sign bit, the
GPU does not), zeros keep their sign: equal hashes mean equal NaN masks and equal words everywhere
else, the rule of special_values.assert_same_bits.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import golden_io as G  # noqa: E402
from tests import modes_ref as R  # noqa: E402
from tests import special_values as SV  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MODES = R.MODES
SEED, PCT = 97, 61.8
# (name, wavelet, level, shape): the tiny kernels, then the per-level kernels
SETTINGS = [
    ("tiny_haar", "haar", 2, (4, 3, 7, 7)),
    ("tiny_db2", "db2", 1, (4, 3, 7, 7)),
    ("level_db8", "db8", 1, (2, 1, 30, 33)),
    ("level_bior33", "bior3.3", 1, (1, 2, 14, 17)),
]
CASES = ["zero_blocks", "subnormal", "nan_corner", "infs"]


def generate():
    """(manifest, arrays) of the fixture, in memory"""
    cases, arrays = {}, {}
    for si, (name, wavelet, level, shape) in enumerate(SETTINGS):
        inputs = SV.cases(shape, SEED, si)
        for case in CASES:
            for mode in MODES:
                with np.errstate(all="ignore"):
                    packed, thr64, thr32, max_abs, out, eff = R.chain(inputs[case], wavelet, level, mode, PCT)
                    zero_count = int((out == 0).sum())
                key = "%s/%s/%s" % (name, case, mode)
                cases[key] = dict(wavelet=wavelet, level=level, pct=PCT, mode=mode, case=case, shape=list(shape),
                                  tid=si, eff_level=int(eff), packed_shape=list(packed.shape),
                                  coeff_numel=int(packed.size), thr64_hex=float(thr64).hex(),
                                  thr32_bits=G.f32_bits(SV.canon_nan(thr32)), max_abs_bits=G.f32_bits(SV.canon_nan(max_abs)),
                                  packed_hash=SV.bits_hash(packed), packed_nan=int(np.isnan(packed).sum()),
                                  packed_inf=int(np.isinf(packed).sum()),
                                  packed_subnormal=int(((np.abs(packed) < np.float32(2.0 ** -126)) & (packed != 0)).sum()),
                                  neg_zero_words=SV.neg_zero_words(packed) + SV.neg_zero_words(out),
                                  zero_count=zero_count)
                arrays[key + "/out"] = SV.canon_nan(out)
    manifest = {"generator": "tools/gen_golden_special_modes.py", "seed": SEED, "cases": cases}
    return manifest, arrays


def main():
    manifest, arrays = generate()
    with open(os.path.join(OUT, "special_modes_manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=0, sort_keys=True)
    np.savez_compressed(os.path.join(OUT, "special_modes_cases.npz"), **arrays)
    size = sum(os.path.getsize(os.path.join(OUT, f)) for f in ("special_modes_manifest.json", "special_modes_cases.npz"))
    print("%d cases, %d arrays, %d bytes" % (len(manifest["cases"]), len(arrays), size))


if __name__ == "__main__":
    main()

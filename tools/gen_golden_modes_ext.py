"""Golden fixtures for the extension modes beyond the PyWavelets grid of tools/gen_golden_modes.py:
tiny images over several waves, percentiles over a population with a zero plateau, long and
unfamiliar filters in the per-level kernels, the component entries at unclamped levels.

Needs no PyWavelets: the expected values come from the reference chain of tests/modes_ref.py (the
host build of csrc/wt_modes_core.h, the oracle's percentile, np.float32 of the threshold), which
tests/test_modes_ext_ref.py anchors to the pywt goldens bit for bit.
    python tools/gen_golden_modes_ext.py

Writes tests/golden/modes_ext_manifest.json and modes_ext_cases.npz.  A case is one call of
engine.prune(list, wavelet, level, pct, carry_level=False, mode=mode); its tensor records carry the
fields of modes_manifest.json, a tiny tensor also lanes_log2 and waves (the images of each of its
waves), a percentile case also the packed array's count of exact zeros, its smallest non-zero
magnitude and the hash of the unthresholded round trip.  Outputs are stored as arrays up to
ARRAY_BUDGET bytes of float32 in the order of GROUP_ORDER, smallest tensors first within a group
(the two files stay under 1 MB together); every output is also pinned by its out_hash, which the
tests compare either way.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import golden_io as G  # noqa: E402
from tests import modes_ref as R  # noqa: E402
from wavelettransforms_amd import workloads as W  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MODES = R.MODES
SIGMA = 0.05
SEG_PER_LAUNCH = 24  # csrc/wtp_internal.h
ARRAY_BUDGET = 800 * 1024
GROUP_ORDER = ["comp", "tiny", "group", "long", "pct"]

# (name, wavelet, requested level, pct, shapes): one call per wavelet, several multi-wave segments a
# table.  Every mode prunes the same input, so a tensor's zero count tells the modes apart -- where
# it has zeros at all: an output sample is an exact zero only when every coefficient under it was
# pruned, 16 of them under db2 at level 1, which pct = 50 does to one sample in 2^16 and pct = 90 to
# one in five.
TINY = [
    ("tiny_haar", "haar", 2, 50.0, [(70, 3, 3, 3), (9, 5, 7, 7), (5, 13, 8, 6), (2, 2, 9, 9), (4, 4, 1, 5)]),
    ("tiny_db2", "db2", 1, 90.0, [(11, 7, 8, 8), (3, 43, 6, 8), (4, 3, 3, 3)]),
]
# more than one launch group; the second starts with a multi-wave tiny tensor, more tiny ones after it
GROUP_MODES = ["symmetric", "periodic"]
GROUP = ("group_haar", "haar", 2,
         [(4, 3, 3, 3), (2, 2, 9, 9), (3, 2, 8, 8), (6, 10), (2, 1, 7, 7), (5, 2, 1, 5)] * 4
         + [(70, 3, 3, 3), (2, 2, 9, 9), (9, 5, 7, 7), (3, 2, 3, 3), (6, 10)])
PCT = [
    ("p96x100", "bior3.3", 3, (96, 100)),
    ("p3x3", "haar", 1, (70, 3, 3, 3)),
    ("p8x6", "haar", 2, (5, 13, 8, 6)),
]
PCTS = [0.0, 5.0, 50.0, 99.9, 100.0]
LONG = [
    ("db8_30x33", "db8", 1, (2, 3, 30, 33)),
    ("db8_64x70", "db8", 2, (2, 2, 64, 70)),
    ("bior33_14x17", "bior3.3", 1, (2, 2, 14, 17)),
    ("sym3_12x10", "sym3", 1, (2, 5, 12, 10)),
    ("coif1_10x12", "coif1", 1, (2, 2, 10, 12)),
    ("bior13_10x11", "bior1.3", 1, (2, 2, 10, 11)),
    ("dmey_124x130", "dmey", 1, (1, 2, 124, 130)),
]
# the component entries take the level as given: lines shorter than the filter
COMP = [
    ("db8_3x3", "db8", 2, (3, 3)),
    ("bior33_2x5", "bior3.3", 3, (2, 2, 2, 5)),
    ("haar_1x7", "haar", 2, (1, 7)),
]


def reflect_undefined(shape2, F, level, mode):
    """whether some level would analyse a one-sample line under reflect (no reference exists)"""
    if mode != "reflect":
        return False
    h, w = shape2
    for _ in range(level):
        if h == 1 or w == 1:
            return True
        h, w = (h + F - 1) // 2, (w + F - 1) // 2
    return False


def record(x, wavelet, level, mode, pct, packed=None):
    """one tensor through the chain: (record with the fields of modes_manifest.json, out, packed)"""
    if packed is None:
        packed, thr64, thr32, max_abs, out, eff = R.chain(x, wavelet, level, mode, pct)
    else:  # the packed array of an earlier chain over the same tensor, level and mode
        eff = level
        thr64, max_abs = O.percentile_abs(packed, pct)
        thr32, max_abs = np.float32(thr64), np.float32(max_abs)
        _, out = R.core(x, wavelet, eff, mode, thr32)
    rec = dict(shape=list(x.shape), eff_level=int(eff), packed_shape=list(packed.shape), coeff_numel=int(packed.size),
               thr64_hex=float(thr64).hex(), thr32_bits=G.f32_bits(thr32), max_abs_bits=G.f32_bits(max_abs),
               packed_hash=G.canon_hash(packed), mask_hash=G.mask_hash(np.abs(packed) < np.float32(thr32)),
               out_hash=G.canon_hash(out), zero_count=int((out == 0).sum()))
    if x.ndim >= 2 and eff > 0:
        lg = R.lanes_log2(x.shape[-2], x.shape[-1], eff, O.dec_len(wavelet))
        if lg >= 0:
            rec["lanes_log2"] = lg
            rec["waves"] = R.waves(int(np.prod(x.shape[:-2])), lg)
    return rec, out, packed


def list_case(cases, outs, group, name, wavelet, level, shapes, mode, seed, e, pct=50.0):
    recs = []
    for ti, shape in enumerate(shapes):
        rec, out, _ = record(W.synth_numpy(tuple(shape), seed, ti, e), wavelet, level, mode, pct)
        rec["synth"] = [seed, ti, e]
        recs.append(rec)
        outs.append((group, "case/%s/%s/%d/out" % (name, mode, ti), out))
    cases["%s/%s" % (name, mode)] = dict(group=group, wavelet=wavelet, level=level, pct=pct, mode=mode, tensors=recs)


def generate():
    """(manifest, arrays) of the fixture, in memory"""
    e = W.sigma_exponent(SIGMA)
    cases, comps, outs, arrays = {}, {}, [], {}
    for ci, (name, wavelet, level, pct, shapes) in enumerate(TINY):
        for mode in MODES:
            list_case(cases, outs, "tiny", name, wavelet, level, shapes, mode, 1700 + 10 * ci, e, pct)
    name, wavelet, level, shapes = GROUP
    assert len(shapes) > SEG_PER_LAUNCH
    for mode in GROUP_MODES:
        list_case(cases, outs, "group", name, wavelet, level, shapes, mode, 1740 + MODES.index(mode), e)
    for ci, (name, wavelet, level, shape) in enumerate(LONG):
        for mi, mode in enumerate(MODES):
            list_case(cases, outs, "long", name, wavelet, level, [shape], mode, 1800 + 10 * ci + mi, e)
    for ci, (name, wavelet, level, shape) in enumerate(PCT):
        for mi, mode in enumerate(MODES):
            seed = 1900 + 10 * ci + mi
            x = W.synth_numpy(shape, seed, 0, e)
            packed, rt = R.core(x, wavelet, level, mode, 0.0)
            mag = np.abs(packed).ravel()
            n, z = mag.size, int((mag == 0).sum())
            # the last rank on the zero plateau; half way between it and the smallest non-zero
            pcts = sorted(set(PCTS + ([100.0 * (z - 1) / (n - 1), 100.0 * (z - 0.5) / (n - 1)] if z else [])))
            for pi, pct in enumerate(pcts):
                rec, out, _ = record(x, wavelet, level, mode, pct, packed=packed)
                rec.update(synth=[seed, 0, e], zeros_packed=z, min_nonzero_bits=G.f32_bits(mag[mag > 0].min()),
                           rt_hash=G.canon_hash(rt))
                cname = "%s/%s/%d" % (name, mode, pi)
                cases[cname] = dict(group="pct", wavelet=wavelet, level=level, pct=pct, mode=mode, tensors=[rec])
                outs.append(("pct", "case/%s/0/out" % cname, out))
    for ci, (name, wavelet, level, shape) in enumerate(COMP):
        for mi, mode in enumerate(MODES):
            key = "%s/%s" % (name, mode)
            seed = 2000 + 10 * ci + mi
            base = dict(wavelet=wavelet, level=level, mode=mode, shape=list(shape), synth=[seed, 0, e])
            if reflect_undefined(shape[-2:], O.dec_len(wavelet), level, mode):
                comps[key] = dict(base, error=True)
                continue
            x = W.synth_numpy(shape, seed, 0, e)
            packed, y0 = R.core(x, wavelet, level, mode, 0.0)
            # a threshold that prunes most coefficients and keeps some (far past the clamp most of the
            # packed array is padding and rounding noise: its median prunes nothing that matters)
            thr32 = np.float32(O.percentile_abs(packed, 90.0)[0])
            _, y1 = R.core(x, wavelet, level, mode, thr32)
            assert 0 < thr32 <= np.abs(packed).max() and not np.array_equal(y0, y1)
            comps[key] = dict(base, error=False, packed_shape=list(packed.shape), packed_hash=G.canon_hash(packed),
                              thr32_bits=G.f32_bits(thr32), out0_hash=G.canon_hash(y0), out1_hash=G.canon_hash(y1))
            arrays["comp/%s/packed" % key], arrays["comp/%s/out0" % key], arrays["comp/%s/out1" % key] = packed, y0, y1
    left = ARRAY_BUDGET - sum(a.nbytes for a in arrays.values())
    for group in GROUP_ORDER:
        for _, key, out in sorted((o for o in outs if o[0] == group), key=lambda o: (o[2].size, o[1])):
            if out.nbytes <= left:
                arrays[key] = out
                left -= out.nbytes
    manifest = {"generator": "tools/gen_golden_modes_ext.py", "cases": cases, "components": comps}
    return manifest, arrays


def main():
    manifest, arrays = generate()
    with open(os.path.join(OUT, "modes_ext_manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=0, sort_keys=True)
    np.savez_compressed(os.path.join(OUT, "modes_ext_cases.npz"), **arrays)
    size = sum(os.path.getsize(os.path.join(OUT, f)) for f in ("modes_ext_manifest.json", "modes_ext_cases.npz"))
    print("%d cases, %d component cases, %d arrays, %d bytes" % (len(manifest["cases"]), len(manifest["components"]),
                                                                  len(arrays), size))


if __name__ == "__main__":
    main()

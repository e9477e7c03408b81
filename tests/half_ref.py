"""The float16 fixtures (tests/golden/f16_manifest.json, f16_cases.npz; tools/gen_golden_f16.py):
loading, and the inputs rebuilt from their stored seeds.  make_input is what the generator itself
calls, so the tests feed the tensors the oracle saw.  NumPy only: the generator imports this file
under the oracle interpreter."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STORE_MAX = 1024  # outputs of at most this many words are stored, larger ones as a hash
_manifest = None
_arrays = None


def make_input(rec, synth_numpy):
    """The float16 input of a tensor record: workloads.synth_numpy from the stored seed, scaled by
    2**rec['scale'], with the record's special pattern, narrowed to float16."""
    seed, tid, e = rec["synth"]
    x = synth_numpy(tuple(rec["shape"]), seed, tid, e)
    x = (x * np.float32(2.0 ** rec.get("scale", 0))).astype(np.float32)
    special = rec.get("special")
    if special == "zeros":
        x = x * np.float32(0)
    elif special == "tied":  # every second weight has the same magnitude
        flat = x.reshape(-1)
        flat[::2] = np.where(flat[::2] < 0, np.float32(-0.03125), np.float32(0.03125))
    x16 = x.astype(np.float16)
    assert np.isfinite(x16).all() and np.abs(x16.astype(np.float64)).max(initial=0) < 65000
    return x16


def words_hash(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16).tobytes()).hexdigest()


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(GOLDEN, "f16_manifest.json")) as fh:
            _manifest = json.load(fh)
    return _manifest


def arrays():
    global _arrays
    if _arrays is None:
        _arrays = dict(np.load(os.path.join(GOLDEN, "f16_cases.npz")))
    return _arrays


def np_ranks(n, pct):
    """np.percentile's lower rank, whether the percentile is the maximum, and gamma (as
    host_plan.hip's seg_ranks)."""
    vi = (n - 1) * (pct / 100.0)
    if vi >= n - 1:
        return n - 1, 1, vi + 1.0
    lo = int(np.floor(vi))
    return lo, 0, vi - lo


NAN_KEY_MIN = 0x7C01  # keys above +inf's (0x7C00) are NaN


def kind_b_ref(words, pct):
    """One tensor that gets no transform, by NumPy 1.26.4's rule for a float16 array written out in
    scalar steps (np.percentile itself changed with NumPy 2): the generator's rule_b, with the two
    lines that the float32 oracle's or_percentile_abs restates for special values -- a NaN in the
    population makes the percentile NaN, and the 100th percentile runs the same difference and
    blend with a = b = max, so an infinite maximum gives inf - inf.  Holds for every finite
    |w| < 65000, +-inf and NaN.  `words` are the uint16 words; returns a dict: out (uint16 words),
    thr64, cmp (np.float16(thr64), the value the compare uses), max (float16), zero_count."""
    words = np.ascontiguousarray(words, np.uint16).reshape(-1)
    n = len(words)
    keys = np.sort(words & np.uint16(0x7FFF))  # the order of |w|, NaN above inf
    s = keys.view(np.float16)
    lo, above, g = np_ranks(n, pct)
    with np.errstate(all="ignore"):
        if int(keys[n - 1]) >= NAN_KEY_MIN:
            thr64 = np.float64(np.nan)
        else:
            a, b = (s[n - 1], s[n - 1]) if above else (s[lo], s[lo + 1])
            d = np.float16(np.float32(b) - np.float32(a))
            a64, b64, d64 = np.float64(a), np.float64(b), np.float64(d)
            thr64 = b64 - d64 * np.float64(1 - g) if g >= 0.5 else a64 + d64 * np.float64(g)
        cmp16 = np.float16(thr64)
        mask = np.abs(words.view(np.float16)) < cmp16
    out = np.where(mask, np.uint16(0), words)
    return dict(out=out, thr64=np.float64(thr64), cmp=cmp16, max=s[n - 1],
                zero_count=int((out & np.uint16(0x7FFF) == 0).sum()))


# ---- populations with special values (tests/test_half_core.py, tests/test_gpu_f16.py) ----

QNAN, SNAN, NEG_QNAN, INF, NEG_INF, NEG_ZERO = 0x7E00, 0x7C01, 0xFE00, 0x7C00, 0xFC00, 0x8000
SPECIAL_PCTS = [0.0, 23.6, 50.0, 61.8, 90.0, 100.0]
SPECIAL_NS = [1, 2, 3, 37, 2000]


def base_words(n, seed):
    """n finite float16 words of both signs, sigma 0.05"""
    x = (np.random.default_rng(seed).standard_normal(n) * 0.05).astype(np.float16)
    assert np.isfinite(x).all()
    return x.view(np.uint16).copy()


def put(words, at):
    """a copy of `words` with the words of the dict `at` {position: word} written in"""
    w = np.array(words, np.uint16)
    for pos, word in at.items():
        w[pos] = word
    return w


def infs_from_rank(words, r):
    """a copy with every word of rank r and above (ascending |w|, stable) made +-inf in turn"""
    w = np.array(words, np.uint16)
    order = np.argsort(w & np.uint16(0x7FFF), kind="stable")
    for k, pos in enumerate(order[r:]):
        w[pos] = NEG_INF if k % 2 else INF
    return w


def special_populations():
    """[(name, uint16 words)] at 1, 2, 3, 37 and 2000 weights: ordinary values; one NaN (quiet,
    signalling, negative) at the first, a middle and the last position; nothing but +-inf; inf
    beside a NaN; +-inf from rank lo + 1 on for each percentile of SPECIAL_PCTS; blocks of -0.0;
    half subnormals throughout.  inf_above_* hold one or three infs that stay above rank lo + 1 at
    every percentile of SPECIAL_PCTS strictly between 0 and 100."""
    pops = []
    for n in SPECIAL_NS:
        b = base_words(n, 100 + n)
        pops.append(("plain_%d" % n, b))
        for pname, pos in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            for wname, word in (("q", QNAN), ("s", SNAN), ("negq", NEG_QNAN)):
                pops.append(("nan_%s_%s_%d" % (pname, wname, n), put(b, {pos: word})))
        pops.append(("all_inf_%d" % n, infs_from_rank(b, 0)))
        pops.append(("inf_and_nan_%d" % n, put(infs_from_rank(b, n // 2), {n - 1: QNAN})))
        if n >= 2:
            # inf from rank lo + 1 on for each percentile below the 100th: at that percentile rank
            # lo is finite and rank lo + 1 is inf, at the higher ones both ranks are inf
            for r in sorted({np_ranks(n, p)[0] + 1 for p in SPECIAL_PCTS[:-1]}):
                pops.append(("inf_from_rank_%d_%d" % (r, n), infs_from_rank(b, r)))
        if n >= 37:
            pops.append(("inf_above_one_%d" % n, infs_from_rank(b, n - 1)))
            pops.append(("inf_above_three_%d" % n, infs_from_rank(b, n - 3)))
            z = b.copy()
            z[:n // 3] = NEG_ZERO
            z[n // 3:n // 3 + 2] = 0
            pops.append(("neg_zero_block_%d" % n, z))
            pops.append(("neg_zero_block_inf_%d" % n, infs_from_rank(z, n - 2)))
        rng = np.random.default_rng(200 + n)
        sub = (rng.integers(1, 0x400, n) | (rng.integers(0, 2, n) << 15)).astype(np.uint16)
        pops.append(("subnormal_%d" % n, sub))
        pops.append(("subnormal_and_zero_%d" % n, put(sub, {0: NEG_ZERO})))
    return pops

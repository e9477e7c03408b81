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

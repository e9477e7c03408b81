"""Record the host-side behaviour of libwtprune.so: tests/golden/host_plan.json.

Every call made here returns before the library's first HIP call, so it runs without a GPU: the
size queries, the prune entries with workspace = NULL (a validation error, or WTP_EWORKSPACE whose
text carries the bytes the layout needs), the component entries at level >= 1 or with invalid
arguments (level 0 copies before it looks at the workspace), wtp_random_prune_f32 where validation
fails.  Per call the fixture keeps the return value (or size), wtp_last_error() and
wtp_last_error_tensor(); tests/test_host_plan.py replays the calls and compares record by record.

The fixture pins what a refactor of the host side must keep, so it is generated from the library of
the commit BEFORE the change and left alone afterwards:

    git worktree add <dir> <commit>
    python -m wavelettransforms_amd.build --csrc <dir>/wavelettransforms_amd/csrc --out <dir>/libwtprune.so
    WTP_LIB_PATH=<dir>/libwtprune.so python tools/gen_golden_host_plan.py --commit <commit>
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "host_plan.json")

WAVELETS = ["haar", "db2", "db8", "bior3.3", "dmey", None]  # None: wavelet id -1
LEVELS = [-1, 0, 1, 2, 5, 33]
FLAGS = list(range(9))
MODES = list(range(-1, 10))
PCTS = [50.0, -1.0, 100.5, float("nan")]
FRACTIONS = [0.0, 0.3, 1.0, 1.5, -0.5, float("nan")]
IMAGES = [(16, 3, 3), (4, 32, 32), (2, 40, 40), (2, 33, 17), (1, 1, 8), (3, 1, 1), (0, 4, 4), (1, 0, 4)]


def tensor_lists():
    """name -> [shape or {"shape", "ndim", "null"}]: a bare shape has valid (never read) pointers."""
    from wavelettransforms_amd import workloads as W
    convs = [list(s) for _, s in W.RESNET18_CONVS]
    return {
        "resnet18": convs,
        "mlp": [[256, 784], [256], [128, 256], [128], [10, 128], [10]],
        "two_groups": [[4, 4, 32, 32]] * 13 + [[16, 3, 3, 3], [8, 8, 5, 5]] * 8,   # 29 tensors
        "fused": [[64, 4096, 4096]] * 3,
        "crop4": [[4, 4, 33, 17]],
        "crop2": [[8, 8, 3, 3], [33, 17]],
        "crop5": [[2, 2, 2, 18, 33]],
        "small": [[8, 8], [4, 4, 3, 3], [2, 5, 5], [1, 1], [16, 2, 2], [8, 4, 8, 8]],
        "lines": [[100], [7], [1]],
        "empty4": [[8, 8, 3, 3], [4, 0, 3, 3]],
        "empty1": [[8, 8, 3, 3], [0]],
        "ndim0": [[]],
        "ndim9": [[8, 8, 3, 3], {"shape": [2] * 8, "ndim": 9}],
        "negdim": [[4, -1, 3, 3]],
        "nullptr": [[8, 8, 3, 3], {"shape": [4, 4, 3, 3], "null": True}],
        "nullptr_empty": [{"shape": [0], "null": True}, [4, 4]],
    }


def calls():
    """The grid, thinned: every list meets every entry point, and every wavelet, level, flag, mode,
    percentile and fraction of the grid is crossed with every list at least along one axis."""
    lists = tensor_lists()
    out = []
    for ln in lists:
        for w in WAVELETS:
            for lv in LEVELS:
                if w in ("haar", "bior3.3") or lv in (2, 5):
                    out.append(["wtp_workspace_size", ln, w, lv])
                if w == "haar" or (lv == 2 and w in ("db8", "dmey", None)):
                    out.append(["wtp_prune_f32", ln, w, lv, 50.0])
                    out.append(["wtp_prune_layers_f32", ln, w, lv, 50.0])
                    out.append(["wtp_abs_workspace_size", ln, w, lv])
                    out.append(["wtp_prune_abs_f32", ln, w, lv, 0.01])
        for fl in FLAGS:
            out.append(["wtp_workspace_size_ex", ln, "haar", 2, fl])
            out.append(["wtp_prune_ex_f32", ln, "haar", 2, 50.0, fl])
        for fl in (0, 1, 2):
            out.append(["wtp_workspace_size_ex", ln, "db8", 5, fl])
        for pct in PCTS[1:]:
            out.append(["wtp_prune_ex_f32", ln, "haar", 2, pct, 1])
            out.append(["wtp_prune_f32", ln, "db2", 2, pct])
        for m in MODES:
            out.append(["wtp_workspace_size_mode", ln, "haar", 2, 0, m])
            out.append(["wtp_prune_mode_f32", ln, "haar", 2, 50.0, 0, m])
        for m in (1, 2, 3, 4, 5):
            out.append(["wtp_workspace_size_mode", ln, "db2", 5, 1, m])
        for m in (0, 3):
            out.append(["wtp_workspace_size_mode", ln, "haar", 2, 2, m])
        out.append(["wtp_workspace_size_mode", ln, "bior3.3", 1, 0, 4])
        out.append(["wtp_workspace_size_mode", ln, None, 2, 0, 3])
        out.append(["wtp_workspace_size_mode", ln, "haar", 2, 8, 3])
        out.append(["wtp_prune_mode_f32", ln, "haar", 2, -1.0, 0, 3])
        out.append(["wtp_prune_mode_f32", ln, "haar", 2, 50.0, 6, 3])
        for fr in FRACTIONS:
            out.append(["wtp_min_prune_workspace_size", ln, fr])
            out.append(["wtp_min_prune_f32", ln, fr])
    # random pruning: only where validation fails, before its first memset
    for ln in ("ndim9", "negdim", "nullptr"):
        out.append(["wtp_random_prune_f32", ln, True])
    out.append(["wtp_random_prune_f32", "lines", False])  # no prune counts
    for n in (100, 0, -1):
        for pct in PCTS:
            out.append(["wtp_threshold_f32", n, pct])
    for (B, H, Wd) in IMAGES:
        for lv in LEVELS:
            if lv <= 32:  # the plain query takes the level as given: its geometry holds 32 levels
                out.append(["wtp_dwt_workspace_size", B, H, Wd, lv])
            for w in WAVELETS:
                if lv != 0 and (w == "haar" or lv == 2):
                    out.append(["wtp_wavedec2_f32", B, H, Wd, w, lv])
                    out.append(["wtp_waverec2_f32", B, H, Wd, w, lv])
            for m in MODES:
                if lv in (0, 1, 2, 5) or m == 3:
                    out.append(["wtp_dwt_workspace_size_mode", B, H, Wd, "haar", lv, m])
                if lv in (1, 2) or (lv != 0 and m == 3):
                    out.append(["wtp_wavedec2_mode_f32", B, H, Wd, "haar", lv, m])
                    out.append(["wtp_waverec2_mode_f32", B, H, Wd, "haar", lv, m])
        for w in ("db2", "bior3.3", None):
            for m in (0, 3, 4):
                out.append(["wtp_dwt_workspace_size_mode", B, H, Wd, w, 2, m])
                out.append(["wtp_wavedec2_mode_f32", B, H, Wd, w, 2, m])
                out.append(["wtp_waverec2_mode_f32", B, H, Wd, w, 2, m])
    for (H, Wd) in ((3, 3), (33, 17), (1, 8), (0, 4)):
        for lv in LEVELS:
            out.append(["wtp_packed_shape", H, Wd, lv])
            for m in MODES:
                if lv in (0, 1, 2) or m == 3:
                    out.append(["wtp_packed_shape_mode", H, Wd, "haar", lv, m])
        for w in ("db2", None):
            for m in (0, 3, 4):
                out.append(["wtp_packed_shape_mode", H, Wd, w, 2, m])
    out += [["wtp_set_resident", 2], ["wtp_set_pipeline", -1], ["wtp_set_fused_select", 2],
            ["wtp_set_resident_early", 3], ["wtp_set_stage_events", 9]]
    # the calls of one entry point on one list (or batch) together: the fixture groups them
    first = {}
    for c in out:
        first.setdefault((c[0], repr(c[1])), len(first))
    out.sort(key=lambda c: first[(c[0], repr(c[1]))])
    return lists, out


class Runner:
    """Makes one recorded call against the loaded library and returns [value, error text, tensor]."""

    def __init__(self, lists):
        from wavelettransforms_amd import _native as N
        self.N, self.L = N, N.lib()
        self.lists = {k: self._tensors(v) for k, v in lists.items()}
        self.fake = ctypes.c_void_p(0x7000)  # a device pointer the library must not read

    def _tensors(self, specs):
        arr = (self.N.WtpTensor * len(specs))()
        for t, sp in enumerate(specs):
            if isinstance(sp, list):
                sp = {"shape": sp}
            shape = sp["shape"]
            arr[t].ndim = sp.get("ndim", len(shape))
            for d, n in enumerate(shape):
                arr[t].shape[d] = n
            if not sp.get("null"):
                arr[t].in_ = 0x100000 + 0x1000 * t
                arr[t].out = 0x900000 + 0x1000 * t
        return arr

    def wid(self, w):
        return -1 if w is None else self.L.wtp_wavelet_id(w.encode())

    def run(self, call):
        L, fn, a = self.L, call[0], call[1:]
        L.wtp_prune_f32(None, 0, 0, 0, 50.0, None, 0, None, None)  # clears the thread's error state
        f = getattr(L, fn)
        if isinstance(a[0], str) and a[0] in self.lists:
            ts, n = self.lists[a[0]], len(self.lists[a[0]])
            a = a[1:]
        if fn in ("wtp_workspace_size", "wtp_abs_workspace_size"):
            v = f(ts, n, self.wid(a[0]), a[1])
        elif fn in ("wtp_workspace_size_ex", "wtp_workspace_size_mode"):
            v = f(ts, n, self.wid(a[0]), *a[1:])
        elif fn in ("wtp_prune_f32", "wtp_prune_layers_f32", "wtp_prune_abs_f32"):
            v = f(ts, n, self.wid(a[0]), a[1], a[2], None, 0, self.fake, None)
        elif fn == "wtp_prune_ex_f32":
            v = f(ts, n, self.wid(a[0]), a[1], a[2], a[3], None, 0, self.fake, None)
        elif fn == "wtp_prune_mode_f32":
            v = f(ts, n, self.wid(a[0]), a[1], a[2], a[3], a[4], None, 0, self.fake, None)
        elif fn == "wtp_min_prune_workspace_size":
            v = f(ts, n, a[0])
        elif fn == "wtp_min_prune_f32":
            v = f(ts, n, a[0], None, 0, self.fake, None)
        elif fn == "wtp_random_prune_f32":
            counts = (ctypes.c_int64 * n)(*([1] * n)) if a[0] else None
            v = f(ts, n, counts, 7, self.fake, None)
        elif fn == "wtp_threshold_f32":
            v = f(self.fake, self.fake, a[0], a[1], None, 0, self.fake, None)
        elif fn == "wtp_dwt_workspace_size":
            v = f(*a)
        elif fn == "wtp_dwt_workspace_size_mode":
            v = f(a[0], a[1], a[2], self.wid(a[3]), a[4], a[5])
        elif fn == "wtp_wavedec2_f32":
            v = f(self.fake, self.fake, a[0], a[1], a[2], self.wid(a[3]), a[4], None, 0, None)
        elif fn == "wtp_waverec2_f32":
            v = f(self.fake, self.fake, a[0], a[1], a[2], self.wid(a[3]), a[4], None, None, 0, None)
        elif fn == "wtp_wavedec2_mode_f32":
            v = f(self.fake, self.fake, a[0], a[1], a[2], self.wid(a[3]), a[4], a[5], None, 0, None)
        elif fn == "wtp_waverec2_mode_f32":
            v = f(self.fake, self.fake, a[0], a[1], a[2], self.wid(a[3]), a[4], a[5], None, None, 0, None)
        elif fn in ("wtp_packed_shape", "wtp_packed_shape_mode"):
            r, c = ctypes.c_int64(-7), ctypes.c_int64(-7)
            b = a if fn == "wtp_packed_shape" else [a[0], a[1], self.wid(a[2]), a[3], a[4]]
            v = [f(*b, ctypes.byref(r), ctypes.byref(c)), r.value, c.value]
        elif fn == "wtp_set_stage_events":
            v = f(None, a[0])
        else:  # the setters, with a value they reject
            v = f(a[0])
        return [v, L.wtp_last_error().decode(errors="replace"), L.wtp_last_error_tensor()]


def records(fixture):
    """The fixture's records, flat: (call, value, error text, tensor).  The file groups them by entry
    point and first argument to stay small: ["fn", first, [[more args..., value, error index, tensor], ...]]."""
    for fn, first, rows in fixture["groups"]:
        for r in rows:
            yield [fn, first] + r[:-3], r[-3], fixture["errors"][r[-2]], r[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="hash of the commit whose library WTP_LIB_PATH names")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if not os.environ.get("WTP_LIB_PATH"):
        sys.exit("set WTP_LIB_PATH to the library to record")
    lists, cs = calls()
    run = Runner(lists)
    errors, groups = [], []
    for c in cs:
        v, err, t = run.run(c)
        if err not in errors:
            errors.append(err)
        if not groups or groups[-1][:2] != c[:2] or len(groups[-1][2]) >= 48:
            groups.append([c[0], c[1], []])
        groups[-1][2].append(c[2:] + [v, errors.index(err), t])
    dump = lambda x: json.dumps(x, separators=(",", ":"))  # NaN is written as NaN and read back as such
    with open(a.out, "w") as fh:
        fh.write('{"commit":%s,\n"lists":%s,\n"errors":%s,\n"groups":[\n%s\n]}\n'
                 % (dump(a.commit), dump(lists), json.dumps(errors, indent=0), ",\n".join(dump(g) for g in groups)))
    print("%s: %d records in %d groups, %d distinct messages, %d bytes"
          % (a.out, len(cs), len(groups), len(errors), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()

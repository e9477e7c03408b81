"""Time the percentile path on float16 weights (wtp_prune_f16) on the ResNet-18 conv list, one call
per model as wavelet_pruning issues it, beside the float32 call of the same list:

    bior3.3, level 5, 50th percentile   every conv clamps to level 0: the float16 selection and mask
    haar, level 2, 50th percentile      transformed tensors (widen, float32 path, narrow) plus the
                                        three 1 x 1 convs at level 0

    python tools/half_bench.py [--seconds 2.0] [--out profiles/half_resnet18.json]

Before it times anything it checks parity: every level-0 tensor against the fixtures' rule restated
in NumPy (float16 difference, float64 blend, float16 compare), every transformed tensor against the
float32 call's output narrowed once.  Then the forms alternate in one process (rounds of back-to-back
calls between device events, after a warm-up of each), with a device copy of the float16 tensors
as the floor.  Appends one JSON line per process to --out: run it twice for two processes.  Kernel
times come from a separate run under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wavelettransforms_amd import engine  # noqa: E402
from wavelettransforms_amd import workloads as W  # noqa: E402

PCT = 50.0
CONFIGS = [("bior3.3", 5), ("haar", 2)]
HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def timed(fn, seconds, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total_ms, calls = 0.0, 0
    while total_ms < seconds * 1e3:
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        total_ms += a.elapsed_time(b)
        calls += batch
    return total_ms / calls * 1e3


def rule_b(x16, pct):
    """(output, zero count) of a float16 tensor that gets no transform, by the fixtures' rule"""
    a = np.abs(x16.reshape(-1))
    s = np.sort(a)
    n = s.size
    vi = (n - 1) * (pct / 100.0)
    if vi >= n - 1:
        thr = float(s[-1])
    else:
        lo = int(np.floor(vi))
        g = vi - lo
        d = float(np.float16(np.float32(s[lo + 1]) - np.float32(s[lo])))
        thr = float(s[lo + 1]) - d * (1 - g) if g >= 0.5 else float(s[lo]) + d * g
    out = np.where(a < np.float16(thr), np.float16(0), x16.reshape(-1)).reshape(x16.shape)
    return out, thr, int((out == 0).sum())


def check_parity(xs16, xs32, wavelet, level):
    outs16, recs16 = engine.prune(xs16, wavelet, level, PCT, carry_level=False)
    outs32, recs32 = engine.prune(xs32, wavelet, level, PCT, carry_level=False)
    kinds = {"A": 0, "B": 0}
    for x, o, r, o32, r32 in zip(xs16, outs16, recs16, outs32, recs32):
        got = o.cpu().numpy()
        if r["path"] == engine.MODE_HALF:
            want, thr, zeros = rule_b(x.cpu().numpy(), PCT)
            assert r["thr64"] == thr and r["zero_count"] == zeros, (r, thr, zeros)
            kinds["B"] += 1
        else:
            want = o32.cpu().numpy().astype(np.float16)
            assert r["thr64"] == r32["thr64"] and r["zero_count"] == int((want == 0).sum()), (r, r32)
            kinds["A"] += 1
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), r
    return kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="device time per form and configuration")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ts = W.resnet18_tensors(0)
    xs32 = [engine.synth(s, seed, tid, e) for _, s, seed, tid, e in ts]
    xs16 = [x.half() for x in xs32]
    xs32 = [x.float() for x in xs16]  # the same values in both forms
    outs32 = [torch.empty_like(x) for x in xs32]
    outs16 = [torch.empty_like(x) for x in xs16]
    weights = sum(x.numel() for x in xs16)

    def copy16():
        for o, x in zip(outs16, xs16):
            o.copy_(x)

    line = {"workload": "resnet18_convs", "pct": PCT, "tensors": len(xs16), "weights": weights,
            "device": torch.cuda.get_device_name(0), "pid": os.getpid(),
            "hbm_roof_us_at_4B_per_weight": round(weights * 4 / HBM_BYTES_PER_S * 1e6, 2), "configs": {}}
    for wavelet, level in CONFIGS:
        kinds = check_parity(xs16, xs32, wavelet, level)
        forms = {
            "float16": lambda: engine.launch(xs16, wavelet, level, PCT, outs=outs16, carry_level=False),
            "float32": lambda: engine.launch(xs32, wavelet, level, PCT, outs=outs32, carry_level=False),
            "copy_float16": copy16,
        }
        for fn in forms.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                rounds[k].append(timed(fn, args.seconds / args.rounds, args.batch))
        cfg = {"parity": "ok", "transformed_tensors": kinds["A"], "level0_tensors": kinds["B"]}
        for k in forms:
            cfg[k] = {"us_per_call": round(sum(rounds[k]) / len(rounds[k]), 2),
                      "us_per_call_rounds": [round(v, 2) for v in rounds[k]]}
        cfg["float16_over_float32"] = round(cfg["float16"]["us_per_call"] / cfg["float32"]["us_per_call"], 3)
        line["configs"]["%s_L%d" % (wavelet, level)] = cfg
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

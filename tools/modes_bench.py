"""Time the percentile path under an extension mode on the ResNet-18 conv list (haar, level 2,
50th percentile, one call per model as wavelet_pruning issues it) beside the same list under
periodization.

    python tools/modes_bench.py [--mode symmetric] [--seconds 2.0] [--out profiles/modes_resnet18.json]
    WTP_LIB_PATH=tools/ab/libwtprune_base.so python tools/modes_bench.py --mode periodization

In one process the two modes alternate (rounds of back-to-back calls between device events, after
a warm-up of both); with WTP_LIB_PATH naming a library of an older revision (tools/build_base.sh)
only periodization exists, and the same script times it alone.  Prints one JSON line: us per call
of each, the rounds, the tensors that took the tiny-image launches (both sides <= 8 and level >= 1)
and the packed coefficients per second.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from wavelettransforms_amd import engine  # noqa: E402
from wavelettransforms_amd import workloads as W  # noqa: E402

WAVELET, LEVEL, PCT = "haar", 2, 50.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="symmetric")
    ap.add_argument("--seconds", type=float, default=2.0, help="device time per mode")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ts = W.resnet18_tensors(0)
    xs = [engine.synth(s, seed, tid, e) for _, s, seed, tid, e in ts]
    outs = [torch.empty_like(x) for x in xs]
    modes = ["periodization"] if args.mode == "periodization" else [args.mode, "periodization"]

    def call(mode):
        if mode == "periodization":  # the entry an older library has too
            engine.launch(xs, WAVELET, LEVEL, PCT, outs=outs, carry_level=False)
        else:
            engine.launch(xs, WAVELET, LEVEL, PCT, outs=outs, carry_level=False, mode=mode)

    recs = {}
    for m in modes:
        for _ in range(10):
            call(m)
        torch.cuda.synchronize()
        recs[m] = engine.decode(call_records(xs, outs, m), len(xs))
    rounds = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            rounds[m].append(timed(lambda: call(m), args.seconds / args.rounds, args.batch))
    line = {"workload": "resnet18_convs", "wavelet": WAVELET, "level": LEVEL, "pct": PCT, "tensors": len(xs),
            "weights": sum(x.numel() for x in xs), "device": torch.cuda.get_device_name(0),
            "library": os.path.relpath(os.environ["WTP_LIB_PATH"], ROOT) if os.environ.get("WTP_LIB_PATH")
            else "working tree"}
    for m in modes:
        us = sum(rounds[m]) / len(rounds[m])
        coeffs = sum(r["coeff_numel"] for r in recs[m])
        line[m] = {"us_per_call": round(us, 2), "us_per_call_rounds": [round(v, 2) for v in rounds[m]],
                   "packed_coeffs": coeffs, "packed_coeffs_per_s": round(coeffs / (us * 1e-6), 1),
                   "zero_count": sum(r["zero_count"] for r in recs[m]),
                   "tiny_tensors": sum(1 for x, r in zip(xs, recs[m])
                                       if r["eff_level"] >= 1 and x.shape[-1] <= 8 and x.shape[-2] <= 8)}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


def call_records(xs, outs, mode):
    if mode == "periodization":
        _, res = engine.launch(xs, WAVELET, LEVEL, PCT, outs=outs, carry_level=False)
    else:
        _, res = engine.launch(xs, WAVELET, LEVEL, PCT, outs=outs, carry_level=False, mode=mode)
    torch.cuda.synchronize()
    return res


if __name__ == "__main__":
    main()

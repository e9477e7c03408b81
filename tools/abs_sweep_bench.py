"""Time the absolute-threshold sweep on the ResNet-18 conv list, bior3.3 level 5, at the eight
thresholds 0.0125 x (0.1, 0.236, 0.382, 0.5, 0.618, 0.786, 0.9, 1.0) (the grid main_pruning.py
notes, scaled to the method's headline threshold) beside eight consecutive engine.launch_abs
calls into eight output sets.

    python tools/abs_sweep_bench.py [--seconds 2.0] [--out profiles/abs_sweep_resnet18.json]
    python tools/abs_sweep_bench.py --child    # one process's measurement (what a profiler wraps)

Device events go around batches of calls; the two forms alternate in one process after a warm-up
of both, and the process first checks that they computed the same thing.  The parent starts two
such processes one after the other, each under a time limit of its own (it never opens the GPU
itself; the second is not started when the first failed), and prints one JSON line with both.  The
yardstick of the sweep is the eight ordinary calls of the same process.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVELET, LEVEL = "bior3.3", 5
THRESHOLDS = [0.0125 * f for f in (0.1, 0.236, 0.382, 0.5, 0.618, 0.786, 0.9, 1.0)]


def timed(fn, seconds, batch):
    import torch
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


def child(args):
    import torch

    from wavelettransforms_amd import engine
    from wavelettransforms_amd import workloads as W

    torch.cuda.set_device(0)
    ts = W.resnet18_tensors(0)
    xs = [engine.synth(s, seed, tid, e) for _, s, seed, tid, e in ts]
    outs = [[torch.empty_like(x) for x in xs] for _ in THRESHOLDS]
    outs2 = [[torch.empty_like(x) for x in xs] for _ in THRESHOLDS]

    def sweep():
        return engine.launch_abs_sweep(xs, WAVELET, LEVEL, THRESHOLDS, outs=outs)

    def eight():
        for thr, o in zip(THRESHOLDS, outs2):
            res = engine.launch_abs(xs, WAVELET, LEVEL, thr, outs=o)
        return res

    forms = {"sweep": sweep, "eight_calls": eight}
    for fn in forms.values():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    # the two forms computed the same thing: outputs bit for bit, records equal
    _, recs = engine.prune_abs_sweep(xs, WAVELET, LEVEL, THRESHOLDS, outs=outs)
    pruned = []
    for k, (thr, o) in enumerate(zip(THRESHOLDS, outs2)):
        _, r1 = engine.prune_abs(xs, WAVELET, LEVEL, thr, outs=o)
        assert r1 == recs[k], (k, thr)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs[k], o)), (k, thr)
        assert all(r["path"] == engine.ABS_PATH_TINY and r["level"] == LEVEL for r in r1)
        pruned.append(sum(r["pruned"] for r in r1))
    rounds = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            rounds[name].append(timed(fn, args.seconds / args.rounds, args.batch))
    line = {"tensors": len(xs), "weights": sum(x.numel() for x in xs), "device": torch.cuda.get_device_name(0),
            "wavelet": WAVELET, "level": LEVEL, "thresholds": THRESHOLDS, "pruned": pruned}
    for name in forms:
        us = sum(rounds[name]) / len(rounds[name])
        line[name] = {"us_per_call": round(us, 2), "us_per_call_rounds": [round(v, 2) for v in rounds[name]]}
    line["eight_calls_over_sweep"] = round(line["eight_calls"]["us_per_call"] / line["sweep"]["us_per_call"], 3)
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="device time per form")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", action="store_true", help="run one process's measurement and print its JSON line")
    ap.add_argument("--child-timeout", type=float, default=180.0, help="time limit of each process, seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    procs = []
    for i in range(2):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(args.seconds), "--batch",
               str(args.batch), "--rounds", str(args.rounds)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            sys.exit("abs_sweep_bench: process %d failed with status %d" % (i, out.returncode))
        procs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    line = {"workload": "resnet18_convs", "library": "working tree", "processes": procs}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

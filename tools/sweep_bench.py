"""Time the percentile sweep on the ResNet-18 conv list at the reference's eight percentiles
(main_pruning.py:186: threshold * 100 for 0.1, 0.236, 0.382, 0.5, 0.618, 0.786, 0.9, 1.0) beside
eight consecutive engine.launch(..., carry_level=False) calls into eight output sets, under
bior3.3 level 5 (every tensor at level 0) and under haar level 2.

    python tools/sweep_bench.py [--seconds 2.0] [--out profiles/sweep_resnet18.json] [--tie]
    python tools/sweep_bench.py --child        # one process's measurement (what a profiler wraps)

Device events go around batches of calls; the two forms alternate in one process after a warm-up
of both; the parent starts two such processes one after the other (it never opens the GPU itself)
and prints one JSON line with both.  --tie adds one timing of a quantised (tie-heavy) 4096 x 4096
tensor under haar level 2 through thresholds_only, for the record beside tools/tie_path.py.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PCTS = [t * 100 for t in (0.1, 0.236, 0.382, 0.5, 0.618, 0.786, 0.9, 1.0)]
WORKLOADS = [("bior3.3", 5), ("haar", 2)]


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
    outs = [[torch.empty_like(x) for x in xs] for _ in PCTS]
    line = {"tensors": len(xs), "weights": sum(x.numel() for x in xs), "device": torch.cuda.get_device_name(0),
            "pcts": PCTS, "workloads": {}}
    for wavelet, level in WORKLOADS:
        def sweep():
            return engine.launch_sweep(xs, wavelet, level, PCTS, outs=outs, carry_level=False)

        def eight():
            for p, o in zip(PCTS, outs):
                res = engine.launch(xs, wavelet, level, p, outs=o, carry_level=False)
            return res

        def thresholds():
            return engine.launch_sweep(xs, wavelet, level, PCTS, carry_level=False, thresholds_only=True)

        def eight_three_launch():  # the same eight calls without the resident launch (window / collect / mask-select)
            for p, o in zip(PCTS, outs):
                res = engine.launch(xs, wavelet, level, p, outs=o, carry_level=False, no_resident=True)
            return res

        forms = {"sweep": sweep, "eight_calls": eight, "eight_calls_three_launch": eight_three_launch,
                 "sweep_thresholds_only": thresholds}
        zeros = {}
        for name, fn in forms.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        # the two forms computed the same thing: every percentile's zero counts agree
        _, res = sweep()
        blocks = res.view(len(PCTS), -1)
        zeros["sweep"] = [sum(r["zero_count"] for r in engine.decode(blocks[k], len(xs))) for k in range(len(PCTS))]
        zeros["eight_calls"] = []
        for p, o in zip(PCTS, outs):  # prune() re-runs a tensor whose resident launch was not co-resident
            _, r1 = engine.prune(xs, wavelet, level, p, outs=o, carry_level=False)
            zeros["eight_calls"].append(sum(r["zero_count"] for r in r1))
        assert zeros["sweep"] == zeros["eight_calls"], zeros
        rounds = {name: [] for name in forms}
        faults = 0
        for _ in range(args.rounds):
            for name, fn in forms.items():
                rounds[name].append(timed(fn, args.seconds / args.rounds, args.batch))
                if name == "eight_calls":  # the last call's records: a timed-out resident launch distorts the figure
                    faults += int(engine.fault_mask(fn()[1], len(xs)).sum())
        w = {"levels": sorted(set(r["eff_level"] for r in engine.decode(blocks[0], len(xs)))), "zero_count": zeros["sweep"],
             "eight_calls_fault_records": faults}
        for name in forms:
            us = sum(rounds[name]) / len(rounds[name])
            w[name] = {"us_per_call": round(us, 2), "us_per_call_rounds": [round(v, 2) for v in rounds[name]]}
        w["eight_calls_over_sweep"] = round(w["eight_calls"]["us_per_call"] / w["sweep"]["us_per_call"], 3)
        w["eight_calls_three_launch_over_sweep"] = round(
            w["eight_calls_three_launch"]["us_per_call"] / w["sweep"]["us_per_call"], 3)
        line["workloads"]["%s_L%d" % (wavelet, level)] = w
    if args.tie:
        sigma = 1.0 / 64
        x = engine.synth((4096, 4096), 5, 3, W.sigma_exponent(sigma))
        x = (torch.round(x * (4 / sigma)) * (sigma / 4)).contiguous()  # a few dozen distinct values
        for _ in range(2):
            engine.launch_sweep([x], "haar", 2, PCTS, thresholds_only=True)
        torch.cuda.synchronize()
        us = timed(lambda: engine.launch_sweep([x], "haar", 2, PCTS, thresholds_only=True), 1e-6, 5)
        line["tie_4096x4096_haar_L2_thresholds_only_us"] = round(us, 1)
        line["tie_distinct_values"] = int(torch.unique(x).numel())
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="device time per form and workload")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--tie", action="store_true")
    ap.add_argument("--child", action="store_true", help="run one process's measurement and print its JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    procs = []
    for i in range(2):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(args.seconds), "--batch",
               str(args.batch), "--rounds", str(args.rounds)] + (["--tie"] if args.tie and i == 0 else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            sys.exit("sweep_bench: process %d failed with status %d" % (i, out.returncode))
        procs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    line = {"workload": "resnet18_convs", "library": "working tree", "processes": procs}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

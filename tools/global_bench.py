"""Time the global percentile on the ResNet-18 conv list at the reference's eight percentiles
(main_pruning.py:186: threshold * 100 for 0.1, 0.236, 0.382, 0.5, 0.618, 0.786, 0.9, 1.0) beside
one engine.launch_sweep call of the same list and percentiles, under bior3.3 level 5 (every tensor
at level 0) and under haar level 2.

    python tools/global_bench.py [--seconds 2.0] [--out profiles/global_resnet18.json]
    python tools/global_bench.py --child        # one process's measurement (what a profiler wraps)

Before anything is timed the global call is held to its rule: the pool's thresholds are computed
on the host from the sweep entry's own coefficients (engine.wavedec2_packed of a transformed
tensor, the raw values of the others) with NumPy's float64 arithmetic written out (no
np.percentile: its NumPy 2.x lerp differs in the last bit), and every record's threshold, and every
output's zero count against a float32 compare of those coefficients for the untransformed tensors,
must agree.  Device events go around batches of calls; the two forms alternate in one process after
a warm-up of both; the parent starts two such processes one after the other (it never opens the GPU
itself) and prints one JSON line with both.
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


def rule_thr64(pool_abs_sorted, pct):
    """NumPy 1.x's linear percentile of the sorted float32 magnitudes: the difference in float32,
    the blend in float64, from the upper end when gamma >= 0.5."""
    import numpy as np
    n = pool_abs_sorted.size
    vi = (n - 1) * (pct / 100.0)
    if vi >= n - 1:
        lo = hi = pool_abs_sorted[-1]
        gamma = vi + 1.0
    else:
        r0 = int(np.floor(vi))
        lo, hi, gamma = pool_abs_sorted[r0], pool_abs_sorted[r0 + 1], vi - np.floor(vi)
    diff = np.float32(hi) - np.float32(lo)
    if gamma >= 0.5:
        return np.float64(hi) - np.float64(diff) * (1.0 - gamma)
    return np.float64(lo) + np.float64(diff) * gamma


def check_parity(engine, xs, wavelet, level, outs):
    """The global call against the rule; returns its per-percentile zero counts and thresholds."""
    import numpy as np
    import torch
    _, recs = engine.prune_global(xs, wavelet, level, PCTS, outs=outs, carry_level=False)
    pool = []
    for x, r in zip(xs, recs[0]):
        if x.dim() >= 2 and r["eff_level"] >= 1:
            c = engine.wavedec2_packed(x.reshape(-1, x.shape[-2], x.shape[-1]), wavelet, r["eff_level"])
            assert c.numel() == r["coeff_numel"], (c.shape, r)
        else:
            c = x
        pool.append(c.detach().abs().reshape(-1).cpu().numpy())
    srt = np.sort(np.concatenate(pool))
    assert not np.isnan(srt[-1])
    for k, p in enumerate(PCTS):
        want = rule_thr64(srt, p)
        for x, o, r in zip(xs, outs[k], recs[k]):
            assert r["path"] == engine.MODE_GLOBAL
            assert np.float64(r["thr64"]).tobytes() == np.float64(want).tobytes(), (wavelet, p, r["thr64"], want)
            assert r["zero_count"] == int((o == 0).sum())
            if not (x.dim() >= 2 and r["eff_level"] >= 1):
                thr32 = torch.tensor(np.float32(want), device=x.device)
                assert torch.equal(o, torch.where(x.abs() < thr32, torch.zeros_like(x), x)), (wavelet, p, tuple(x.shape))
    return [sum(r["zero_count"] for r in recs[k]) for k in range(len(PCTS))], [recs[k][0]["thr64"] for k in range(len(PCTS))]


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
        def glob():
            return engine.launch_global(xs, wavelet, level, PCTS, outs=outs, carry_level=False)

        def sweep():
            return engine.launch_sweep(xs, wavelet, level, PCTS, outs=outs, carry_level=False)

        def glob_thresholds():
            return engine.launch_global(xs, wavelet, level, PCTS, carry_level=False, thresholds_only=True)

        def sweep_thresholds():
            return engine.launch_sweep(xs, wavelet, level, PCTS, carry_level=False, thresholds_only=True)

        zeros, thr64 = check_parity(engine, xs, wavelet, level, outs)
        forms = {"global": glob, "sweep": sweep, "global_thresholds_only": glob_thresholds,
                 "sweep_thresholds_only": sweep_thresholds}
        for fn in forms.values():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        rounds = {name: [] for name in forms}
        for _ in range(args.rounds):
            for name, fn in forms.items():
                rounds[name].append(timed(fn, args.seconds / args.rounds, args.batch))
        _, res = glob()
        torch.cuda.synchronize()
        recs = engine.decode(res.view(len(PCTS), -1)[0], len(xs))
        w = {"levels": sorted(set(r["eff_level"] for r in recs)), "pool_keys": sum(r["coeff_numel"] for r in recs),
             "zero_count": zeros, "thr64": thr64, "parity": "ok"}
        for name in forms:
            us = sum(rounds[name]) / len(rounds[name])
            w[name] = {"us_per_call": round(us, 2), "us_per_call_rounds": [round(v, 2) for v in rounds[name]]}
        w["global_over_sweep"] = round(w["global"]["us_per_call"] / w["sweep"]["us_per_call"], 3)
        w["global_over_sweep_thresholds_only"] = round(
            w["global_thresholds_only"]["us_per_call"] / w["sweep_thresholds_only"]["us_per_call"], 3)
        line["workloads"]["%s_L%d" % (wavelet, level)] = w
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="device time per form and workload")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", action="store_true", help="run one process's measurement and print its JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    procs = []
    for i in range(2):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(args.seconds), "--batch",
               str(args.batch), "--rounds", str(args.rounds)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            sys.exit("global_bench: process %d failed with status %d" % (i, out.returncode))
        procs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    line = {"workload": "resnet18_convs", "library": "working tree", "processes": procs}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

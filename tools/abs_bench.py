"""Time the absolute-threshold method on its headline workload: the 20 ResNet-18 conv weights,
bior3.3 level 5, threshold 0.0125, one wtp_prune_abs_f32 call (one k_abs_tiny launch).

    python tools/abs_bench.py [--seconds 0.5] [--out profiles/abs_resnet18.json]

In the same process the call alternates with a device-to-device copy of the same 20 tensors into
the same outputs: the read-plus-write floor of this box on this day.  Both are timed with device
events around batches of back-to-back calls, after a warm-up.  Prints one JSON line: us per
call, weight-coeffs/s, the copy's us, their ratio, the flop count and bytes computed from the
shapes, and both roofs (HBM at the spec rate, VALU at the measured no-FMA rate of
profiles/r03_valu_nofma_rate.txt).  The kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/abs_bench.py` run.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from wavelettransforms_amd import _native as N  # noqa: E402
from wavelettransforms_amd import engine  # noqa: E402
from wavelettransforms_amd import workloads as W  # noqa: E402

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec
VALU_NOFMA_TFLOPS = 128.0   # measured, separate multiplies and adds (profiles/r03_valu_nofma_rate.txt)
WAVELET, LEVEL, THRESHOLD = "bior3.3", 5, 0.0125


def image_flops(H, W_, L, F):
    """Multiplies and adds (no FMA) of one image: per level the column and the row analysis
    (every tap feeds two bands: 4 flop) and the row and the column synthesis (F taps per output
    over the two bands: 2 flop each), every wrapped tap counted as the kernel computes it."""
    flops = 0
    dims = [(H, W_)]
    for _ in range(L):
        r, c = dims[-1]
        dims.append(((r + 1) // 2, (c + 1) // 2))
    for k in range(1, L + 1):
        (r0, c0), (r, c) = dims[k - 1], dims[k]
        flops += 4 * F * r * c0          # columns: (r x c0) outputs, two bands
        flops += 2 * 4 * F * r * c       # rows of both half transforms
        oh, ow = (H, W_) if k == 1 else (2 * r, 2 * c)
        flops += 2 * 2 * F * r * 2 * c   # row synthesis of lo and hi
        flops += 2 * F * oh * ow         # column synthesis (the last level cropped)
    return flops


def timed(fn, seconds, batch):
    """us per call: batches of `batch` calls between two events until `seconds` of device time."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total_ms, calls, best = 0.0, 0, float("inf")
    while total_ms < seconds * 1e3:
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        total_ms += ms
        calls += batch
        best = min(best, ms / batch)
    return total_ms / calls * 1e3, best * 1e3, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the call and the copy")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ts = W.resnet18_tensors(0)
    xs = [engine.synth(s, seed, tid, e) for _, s, seed, tid, e in ts]
    outs = [torch.empty_like(x) for x in xs]
    F = N.lib().wtp_dec_len(engine.wavelet_id(WAVELET))
    weights = sum(x.numel() for x in xs)
    flops = sum(x.numel() // (x.shape[-2] * x.shape[-1]) * image_flops(x.shape[-2], x.shape[-1], LEVEL, F) for x in xs)
    nbytes = 8 * weights

    def call():
        engine.launch_abs(xs, WAVELET, LEVEL, THRESHOLD, outs=outs)

    def copy():
        for x, o in zip(xs, outs):
            o.copy_(x)

    for _ in range(10):  # warm-up: the workspace, the code objects, the clocks
        call()
        copy()
    torch.cuda.synchronize()
    _, recs = engine.prune_abs(xs, WAVELET, LEVEL, THRESHOLD, outs=outs)
    assert all(r["path"] == engine.ABS_PATH_TINY and r["level"] == LEVEL for r in recs)
    call_us, copy_us, call_best, copy_best, calls = [], [], [], [], 0
    for _ in range(args.rounds):
        m, b, n = timed(call, args.seconds / args.rounds, args.batch)
        call_us.append(m)
        call_best.append(b)
        calls += n
        m, b, _ = timed(copy, args.seconds / args.rounds, args.batch)
        copy_us.append(m)
        copy_best.append(b)
    us = sum(call_us) / len(call_us)
    cus = sum(copy_us) / len(copy_us)
    line = {
        "workload": "resnet18_convs", "wavelet": WAVELET, "level": LEVEL, "threshold": THRESHOLD,
        "tensors": len(xs), "weights": weights, "device": torch.cuda.get_device_name(0),
        "us_per_call": round(us, 2), "us_per_call_best_batch": round(min(call_best), 2), "calls_timed": calls,
        "us_per_call_rounds": [round(v, 2) for v in call_us],
        "weight_coeffs_per_s": round(weights / (us * 1e-6), 1),
        "copy_us": round(cus, 2), "copy_us_best_batch": round(min(copy_best), 2),
        "copy_us_rounds": [round(v, 2) for v in copy_us],
        "ratio_to_copy": round(us / cus, 3),
        "flops": flops, "flop_per_weight": round(flops / weights, 1), "bytes": nbytes,
        "flop_per_byte": round(flops / nbytes, 2),
        "hbm_roof_us": round(nbytes / (HBM_PEAK_GBS * 1e9) * 1e6, 2),
        "valu_roof_us": round(flops / (VALU_NOFMA_TFLOPS * 1e12) * 1e6, 2),
        "hbm_peak_gbs": HBM_PEAK_GBS, "valu_nofma_tflops": VALU_NOFMA_TFLOPS,
        "achieved_gbs": round(nbytes / (us * 1e-6) / 1e9, 1), "achieved_tflops": round(flops / (us * 1e-6) / 1e12, 2),
        "pruned": sum(r["pruned"] for r in recs),
    }
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

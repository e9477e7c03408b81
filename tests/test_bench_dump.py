"""bench.py --dump-outputs: the files a run leaves (host logic only, CPU tensors): whole tensors
within the budget, a fixed seeded sample of each beyond it, float32 / float64, the same bytes from
run to run; and the options a plain run and a --full run are started with."""
import os
import sys

import numpy as np
import torch

import bench

REC = {"numel": 6, "zero_count": 3, "coeff_numel": 6, "thr64": 0.25, "thr32_bits": 0x3E800000,
       "max_abs_bits": 0x3F800000, "eff_level": 0, "path": 1}


def _tensors():
    g = torch.Generator().manual_seed(7)
    return [torch.randn(2, 3, generator=g), torch.randn(5, 7, 3, generator=g), torch.randn(4, generator=g)]


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole(tmp_path):
    ts = _tensors()
    bench.dump_outputs(str(tmp_path / "a"), ts, [REC] * len(ts))
    got = _load(tmp_path / "a")
    assert sorted(got) == ["out_000.npy", "out_001.npy", "out_002.npy", "records.npy"]
    for i, t in enumerate(ts):
        a = got["out_%03d.npy" % i]
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.numpy())
    r = got["records.npy"]
    assert r.dtype == np.float64 and r.shape == (3, len(bench.RECORD_COLUMNS))
    assert r[0].tolist() == [6, 3, 6, 0.25, 0.25, 1.0, 0, 1]


def test_dump_sampled_is_fixed(tmp_path, monkeypatch):
    ts = _tensors()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 3 * 10)  # 10 elements a tensor
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), ts, [REC] * len(ts))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b)
    for f in a:
        assert a[f].tobytes() == b[f].tobytes()
    assert a["out_000.npy"].shape == (2, 3) and a["out_002.npy"].shape == (4,)   # at most 10: whole
    s = a["out_001.npy"]
    assert s.dtype == np.float32 and s.shape == (10,)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED + 1).integers(0, 105, size=10))
    assert np.array_equal(s, ts[1].reshape(-1).numpy()[idx])
    assert sum(v.nbytes for k, v in a.items() if k.startswith("out_")) <= 4 * 3 * 10


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    # the rocprofv3 child: warmup, side-stream step, two warm replays, the steps; no lead-in
    a.steps, a.warmup, a.graph_steps, a.no_graph = 200, 5, 10, False
    assert bench.child_steps(a) == 5 + 200 + 1 + 2 * 10

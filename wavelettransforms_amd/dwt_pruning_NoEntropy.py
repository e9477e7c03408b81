"""Drop-in counterpart of ResNet/dwt_pruning_NoEntropy.py (iAmGiG/WaveletTransforms) on MI355X:
wavelet pruning with an ABSOLUTE threshold.

Same public names, arguments, return values and printed lines as the reference module; the
arithmetic runs in libwtprune.so (HIP, gfx950; wtp_prune_abs_f32) on device-resident tensors:

  multi_resolution_analysis    dwt_pruning_NoEntropy.py:12-62
  multi_resolution_analysis_sweep   the same at a grid of thresholds, one device call (an addition)
  prune_layer_weights          dwt_pruning_NoEntropy.py:65-91
  wavelet_pruning              dwt_pruning_NoEntropy.py:94-138

This is not dwt_pruning.py with another threshold.  The level is NOT clamped to
pywt.dwt_max_level: PyWavelets only warns (the same UserWarning is raised here) and transforms
lines shorter than the filter, so ResNet-18's 3 x 3 kernels really go through five levels.  The
threshold is the given number, compared in float32 as NumPy 1.x compares a float32 array with a
Python float.  A layer is pruned with ALL its parameters, the bias included (a 1-D tensor is
masked as it is), odd shapes are cropped with a generic slice (no error for 2-D tensors), and
the counts are count_nonzero(before) - count_nonzero(after).

Differences by design, as in dwt_pruning.py: `wavelet_pruning` prunes every Conv2d of the model
in ONE batched call instead of a per-layer loop (results and logs are identical); weights that
live on the CPU are moved to the current CUDA device for the computation and the results come
back on the weight's own device; only mode='periodization' exists; float32 weights only.
"""
import os
import warnings
from typing import List, Tuple

import torch
import torch.nn as nn

from . import engine
from . import _native as N
from .utils import (append_to_experiment_log, check_and_set_pruned_instance_path, log_pruning_details,
                    save_model, setup_csv_writer)

__all__ = ["multi_resolution_analysis", "multi_resolution_analysis_sweep", "prune_layer_weights", "wavelet_pruning"]


def _cuda(x):
    if x.is_cuda:
        return x
    return x.to(torch.device("cuda", torch.cuda.current_device()))


def _warn_levels(weights, wavelet, level):
    # pywt._multilevel._check_level: wavedec2 warns when the level exceeds dwt_max_level of the
    # shorter transformed axis and carries on
    wid = engine.wavelet_id(wavelet)
    if wid < 0 or int(level) < 0:
        return  # the call itself raises pywt's ValueError
    L = N.lib()
    dec_len = L.wtp_dec_len(wid)
    for w in weights:
        if w.dim() >= 2 and w.numel() and int(level) > L.wtp_max_level(int(min(w.shape[-2:])), dec_len):
            warnings.warn("Level value of {} is too high: all coefficients will experience boundary "
                          "effects.".format(level), UserWarning, stacklevel=3)


def _run(weights, wavelet, level, threshold):
    """One batched call for the whole list: (pruned tensors on the weights' devices, with their
    dtype and shape; the decoded records)."""
    _warn_levels(weights, wavelet, level)
    devs = [w.device for w in weights]
    with torch.no_grad():
        outs, recs = engine.prune_abs([_cuda(w.detach()) for w in weights], wavelet, level, threshold)
        outs = [o.to(d).to(dtype=w.dtype).view(w.shape) for o, d, w in zip(outs, devs, weights)]
    return outs, recs


def multi_resolution_analysis(weights: List[torch.Tensor], wavelet: str, level: int, threshold: float,
                              mode: str = "periodization") -> Tuple[List[torch.Tensor], int]:
    """Wavelet-domain pruning of each tensor with an absolute threshold
    (dwt_pruning_NoEntropy.py:12-62).  Returns (pruned tensors, total pruned count): the count is
    the sum over the tensors of count_nonzero(weight) - count_nonzero(pruned)."""
    if mode != "periodization":
        raise NotImplementedError("only mode='periodization' is implemented (the reference's only mode)")
    weights = list(weights)
    if len(weights) == 0:
        return [], 0
    outs, recs = _run(weights, wavelet, level, threshold)
    return outs, int(sum(r["nonzero_in"] - r["nonzero_out"] for r in recs))


def multi_resolution_analysis_sweep(weights: List[torch.Tensor], wavelet: str, level: int,
                                    thresholds) -> List[Tuple[List[torch.Tensor], int]]:
    """multi_resolution_analysis at several thresholds in one device call (the reference's
    experiment runs the same model and wavelet at a grid of thresholds).  Returns a list over
    `thresholds` of (pruned tensors, total pruned count), each entry what
    multi_resolution_analysis(weights, wavelet, level, thresholds[k]) returns; every tensor is read
    and transformed forward once for all of them (engine.prune_abs_sweep; at most
    engine.WTP_ABS_SWEEP_MAX_THR thresholds a call, longer grids run in several).  The level
    warning is raised as multi_resolution_analysis raises it."""
    thresholds = list(thresholds)
    weights = list(weights)
    if len(weights) == 0:
        return [([], 0) for _ in thresholds]
    _warn_levels(weights, wavelet, level)
    result = []
    with torch.no_grad():
        devs = [w.device for w in weights]
        dev_w = [_cuda(w.detach()) for w in weights]
        for i in range(0, len(thresholds), engine.WTP_ABS_SWEEP_MAX_THR):
            outs, recs = engine.prune_abs_sweep(dev_w, wavelet, level, thresholds[i:i + engine.WTP_ABS_SWEEP_MAX_THR])
            for o, r in zip(outs, recs):
                pruned = [y.to(d).to(dtype=w.dtype).view(w.shape) for y, d, w in zip(o, devs, weights)]
                result.append((pruned, int(sum(x["nonzero_in"] - x["nonzero_out"] for x in r))))
    return result


def _copy_back(params, pruned):
    with torch.no_grad():
        for param, new in zip(params, pruned):
            if param.requires_grad:  # :88-89
                param.copy_(new)


def prune_layer_weights(layer: nn.Module, wavelet: str, level: int, threshold: float) -> Tuple[int, int, int]:
    """Prune ALL parameters of `layer` in place (the bias too; parameters that do not require
    grad are left as they are).  Returns (parameter count, non-zero parameters BEFORE pruning,
    pruned count) -- the second value is the reference's (dwt_pruning_NoEntropy.py:79-91)."""
    params = [p for p in layer.parameters()]
    original_param_count = sum(p.numel() for p in params)
    if not params:
        return 0, 0, 0
    outs, recs = _run(params, wavelet, level, threshold)
    non_zero_params = int(sum(r["nonzero_in"] for r in recs))
    layer_pruned_count = int(sum(r["nonzero_in"] - r["nonzero_out"] for r in recs))
    _copy_back(params, outs)
    return original_param_count, non_zero_params, layer_pruned_count


def wavelet_pruning(model, wavelet: str, level: int, threshold: float, csv_path: str, guid: str) -> str:
    """Prune every parameter of every Conv2d of `model`, log per layer, save the model and append
    the run to the experiment log; returns the per-layer log path
    (dwt_pruning_NoEntropy.py:94-138).  All layers' parameters go through ONE batched call."""
    total_pruned_count = 0
    total_non_zero_params = 0
    selective_pruned_dir = check_and_set_pruned_instance_path(
        f"{wavelet}_threshold-{threshold}_level-{level}_guid-{guid[:4]}/selective_pruned")
    selective_log_path = os.path.join(selective_pruned_dir, "log.csv")
    writer, fh = setup_csv_writer(os.path.normpath(selective_log_path), mode="w")
    layers = [(name, m) for name, m in model.named_modules() if isinstance(m, nn.Conv2d)]
    params, spans = [], []
    for _, m in layers:
        ps = [p for p in m.parameters()]
        spans.append((len(params), len(params) + len(ps)))
        params += ps
    outs, recs = _run(params, wavelet, level, threshold) if params else ([], [])
    _copy_back(params, outs)
    for (name, _), (a, b) in zip(layers, spans):
        original_param_count = sum(p.numel() for p in params[a:b])
        non_zero_params = int(sum(r["nonzero_in"] for r in recs[a:b]))
        layer_pruned_count = int(sum(r["nonzero_in"] - r["nonzero_out"] for r in recs[a:b]))
        total_pruned_count += layer_pruned_count
        total_non_zero_params += non_zero_params
        log_pruning_details(writer, guid, wavelet, level, threshold, "selective", original_param_count,
                            non_zero_params, layer_pruned_count, name)
    fh.close()
    save_model(model, selective_pruned_dir)
    append_to_experiment_log(os.path.normpath(csv_path), guid, wavelet, level, threshold, "selective",
                             total_pruned_count, total_non_zero_params, selective_pruned_dir)
    print(f"Selectively pruned model saved at {selective_pruned_dir}")
    return selective_log_path

"""Device-resident execution of the DWT -> percentile-threshold -> IDWT path for torch tensors.

`launch()` issues one batched launch sequence (libwtprune.so) for a list of CUDA float32
tensors on the current stream and returns the outputs plus the device-side result records;
`prune()` additionally waits and decodes them.  Nothing here computes on the CPU: the
numbers come from the HIP kernels, the host only packs pointers and decodes results.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _native as N

RESULT_DTYPE = np.dtype([("numel", "<i8"), ("zero_count", "<i8"), ("coeff_numel", "<i8"), ("thr64", "<f8"),
                         ("thr32_bits", "<u4"), ("max_abs_bits", "<u4"), ("eff_level", "<i4"), ("path", "<i4")])
assert RESULT_DTYPE.itemsize == N.RESULT_BYTES

_workspaces = {}


def wavelet_id(name):
    return N.lib().wtp_wavelet_id(str(name).encode()) if isinstance(name, str) else -1


def workspace(device, nbytes, stream=None, kind=None):
    """Grow-only, zero-initialised workspace per (device, stream, kind): the selection, barrier and
    parity state of a call live in it, so calls on distinct streams need distinct workspaces
    (include/wtprune.h).  The library keeps it clean between calls on its stream.  Each stream
    ever used keeps its workspace (at the largest size it needed: a cfg5-sized call holds the
    packed coefficients of its images) until release_workspaces() drops it.  kind=None is the
    workspace of the selection entries, whose state the library keeps clean; an entry that uses its
    workspace as plain scratch (launch_abs and launch_abs_sweep: kind="abs", launch_sweep: kind="sweep", launch_global: kind="global") gets one of its
    own, so it never writes over that state."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    if stream is None:
        stream = torch.cuda.current_stream(device)
    key = (device.index, stream.cuda_stream) if kind is None else (device.index, stream.cuda_stream, kind)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            # the zero-fill below becomes a node of the graph and re-zeroes the workspace on every
            # replay (correct, but a memset of the whole workspace per replay): warm the call up on
            # the capturing stream first (torch.cuda.graph(g, stream=s) after a call on s)
            warnings.warn("wavelettransforms_amd: workspace allocated inside a graph capture; its "
                          "zero-fill is replayed with the graph", RuntimeWarning, stacklevel=3)
        # allocated (and zeroed) on the call's stream, so the caching allocator ties the block to it
        with torch.cuda.stream(stream):
            ws = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def release_workspaces(device=None, stream=None):
    """Drop the cached workspaces (all, one device's, or one (device, stream)'s): their memory goes
    back to torch's caching allocator.  Call it after the stream's work has been waited for or
    when retiring a stream whose handle may be recycled; the next call allocates a zeroed one."""
    for key in list(_workspaces):
        if device is not None and key[0] != torch.device(device).index:
            continue
        if stream is not None and key[1] != stream.cuda_stream:
            continue
        del _workspaces[key]


def _results(n, device, stream):
    with torch.cuda.stream(stream):
        return torch.empty(n * N.RESULT_BYTES, dtype=torch.uint8, device=device)


def check_outs(tensors, outs, dtype=torch.float32):
    """Caller-supplied outputs must be dense CUDA tensors of the inputs' dtype (float32; float16
    where the entry takes it) shaped like their inputs: the library writes numel contiguous words
    from out.data_ptr()."""
    if len(outs) != len(tensors):
        raise ValueError("wavelettransforms_amd: %d outputs for %d tensors" % (len(outs), len(tensors)))
    for i, (x, y) in enumerate(zip(tensors, outs)):
        if not isinstance(y, torch.Tensor) or not y.is_cuda or y.dtype != dtype:
            raise TypeError("wavelettransforms_amd: outs[%d] must be a %s CUDA tensor"
                            % (i, str(dtype).replace("torch.", "")))
        if y.device != x.device or y.numel() != x.numel():
            raise ValueError("wavelettransforms_amd: outs[%d] has %d elements on %s, input %d on %s"
                             % (i, y.numel(), y.device, x.numel(), x.device))
        if not y.is_contiguous():
            raise ValueError("wavelettransforms_amd: outs[%d] is not contiguous" % i)


def _as_desc(tensors, outs):
    arr = (N.WtpTensor * max(1, len(tensors)))()
    for i, (x, y) in enumerate(zip(tensors, outs)):
        d = arr[i]
        d.in_ = x.data_ptr() if x.numel() else None
        d.out = y.data_ptr() if y.numel() else None
        d.ndim = x.dim()
        for j, s in enumerate(x.shape):
            d.shape[j] = s
    return arr


def _prepare(tensors, outs, nsets=None, sets_of=None, no_outs=False, allow_half=False):
    """What every launcher starts with: the checked tensors made contiguous, the default or checked
    outputs (one list; under nsets a list of nsets lists, one per `sets_of`; none under no_outs),
    the tensor count, their device and the descriptor array -- the last two None for an empty
    list, which the caller answers before it touches a device.  A sweep's descriptors carry the
    inputs alone: its outputs go to the library as _out_ptrs.  allow_half: the entry takes a list
    of float16 tensors too (launch(); its outputs are then float16)."""
    dtype = check_tensors(tensors, allow_half=allow_half)
    tensors = [x.contiguous() for x in tensors]
    if no_outs:
        outs = None
    elif nsets is None:
        if outs is None:
            outs = [torch.empty_like(x) for x in tensors]
        else:
            check_outs(tensors, outs, dtype)
    elif outs is None:
        outs = [[torch.empty_like(x) for x in tensors] for _ in range(nsets)]
    else:
        if len(outs) != nsets:
            raise ValueError("wavelettransforms_amd: %d output sets for %d %s" % (len(outs), nsets, sets_of))
        for o in outs:
            check_outs(tensors, o)
    n = len(tensors)
    if n == 0:
        return tensors, outs, 0, None, None
    return tensors, outs, n, tensors[0].device, _as_desc(tensors, tensors if nsets is not None else outs)


def _current(device, stream):
    return torch.cuda.current_stream(device) if stream is None else stream


def _out_ptrs(outs, n):
    """A sweep's output pointers, set-major: set k of tensor t at [k * n + t]."""
    return (ctypes.c_void_p * max(1, len(outs) * n))(*[y.data_ptr() if y.numel() else None for o in outs for y in o])


def _decode_blocks(res, nsets, n, nbytes, decode_fn):
    """A sweep's records, one decoded block of n per set."""
    if res is None:
        return [[] for _ in range(nsets)]
    blocks = res.view(nsets, n * nbytes)
    return [decode_fn(blocks[k], n) for k in range(nsets)]


def raise_for(code, tensors, wavelet):
    """Map a library status to the exception the reference path raises at that point."""
    L = N.lib()
    msg = N.last_error()
    t = L.wtp_last_error_tensor()
    if code == N.WTP_EBADWAVELET:
        raise ValueError("Unknown wavelet name '%s', check wavelist() for the list of available builtin "
                         "wavelets." % wavelet)
    if code in (N.WTP_EBADLEVEL, N.WTP_EBADPCT):
        raise ValueError(msg)
    if code == N.WTP_EEMPTY:
        raise IndexError(msg)
    if code == N.WTP_ECROP:
        x = tensors[t] if 0 <= t < len(tensors) else None
        if x is not None and x.dim() > 4:
            raise RuntimeError("shape '%s' is invalid for input of size %d" % (list(x.shape), _recon_numel(x)))
        raise IndexError(msg)
    raise RuntimeError("libwtprune: %s (status %d)" % (msg, code))


def _recon_numel(x):
    # size of the waverec2 output after the reference's 4-index crop (for the error message)
    shape = list(x.shape)
    h, w = shape[-2], shape[-1]
    shape[-1] = 2 * ((w + 1) // 2)
    if x.dim() >= 6:
        shape[-2] = 2 * ((h + 1) // 2)
    n = 1
    for s in shape:
        n *= s
    return n


def check_tensors(tensors, allow_half=False):
    """Every tensor a float32 CUDA tensor; under allow_half (the percentile path of launch() /
    prune()) a list whose tensors are ALL float16 passes too.  Returns the list's dtype."""
    dtype = list_dtype(tensors, allow_half)
    for x in tensors:
        if not isinstance(x, torch.Tensor):
            raise TypeError("expected torch.Tensor, got %r" % type(x))
        if not x.is_cuda:
            raise ValueError("wavelettransforms_amd runs on the GPU: tensor on %s (move it to cuda)" % x.device)
        check_dtype(x, dtype)
    return dtype


def list_dtype(tensors, allow_half=False):
    """The dtype a list is held to: float32, or float16 when the entry takes it and some tensor is one."""
    if allow_half and any(isinstance(x, torch.Tensor) and x.dtype == torch.float16 for x in tensors):
        return torch.float16
    return torch.float32


def check_dtype(x, dtype):
    """TypeError unless x has the list's dtype (bfloat16 and float64 never pass: the reference's
    .numpy() refuses the first, and the path is not built for the second)."""
    if x.dtype != dtype:
        if dtype == torch.float16:
            raise TypeError("wavelettransforms_amd: float16 and %s weights in one call (all float16 or all "
                            "float32)" % x.dtype)
        raise TypeError("wavelettransforms_amd: float32 weights only (got %s)" % x.dtype)


WTP_CARRY_LEVEL, WTP_FLATTEN, WTP_NO_RESIDENT = 1, 2, 4  # include/wtprune.h


MODES = ("periodization", "zero", "constant", "symmetric", "reflect", "periodic")  # WTP_MODE_* 0..5


def mode_id(mode):
    """WTP_MODE_* id of a PyWavelets mode name (include/wtprune.h).  A name pywt rejects raises
    pywt's ValueError; smooth, antisymmetric and antireflect raise NotImplementedError."""
    if mode == MODES[0]:
        return 0
    mid = N.lib().wtp_mode_id(mode.encode()) if isinstance(mode, str) else -1
    if mid < 0:
        raise ValueError("Unknown mode name '%s'." % (mode,))
    if mid >= len(MODES):
        raise NotImplementedError("mode=%r is not implemented (implemented: %s)" % (mode, ", ".join(MODES)))
    return mid


def launch(tensors, wavelet, level, pct, outs=None, carry_level=True, stream=None, flatten=False,
           no_resident=False, results=None, mode="periodization"):
    """Enqueue the path for `tensors` (CUDA float32) on `stream` (default: current stream).
    Returns (outs, results_dev) without synchronising; results_dev is a uint8 CUDA tensor of
    len(tensors) wtp_result records.  carry_level=True is multi_resolution_analysis over a
    list (the clamped level carries over, dwt_pruning.py:64-65); False is one call per layer
    (prune_layer_weights / wavelet_pruning).  flatten=True: the 1-D flattened mode (WTP_FLATTEN).
    A record whose path reads MODE_FAULT was not computed (the resident launch's grid was not
    co-resident; nothing was stored for that tensor): prune() re-runs such tensors itself.
    mode: the PyWavelets signal-extension mode of the transform (wtp_prune_mode_f32).
    A list of float16 tensors (all of them: model.half()) runs wtp_prune_f16 and gives float16
    outputs, as the reference does with such weights; outs must then be float16 and flatten=True
    is a TypeError (the flattened mode is float32 only).
    results: optional uint8 CUDA tensor of len(tensors) records (8-byte aligned) to write into."""
    mid = mode_id(mode)
    if mid and flatten:
        raise ValueError("wavelettransforms_amd: flatten=True runs under mode='periodization' only")
    tensors, outs, n, device, desc = _prepare(tensors, outs, allow_half=True)
    half = n > 0 and tensors[0].dtype == torch.float16
    if half and flatten:
        raise TypeError("wavelettransforms_amd: flatten=True takes float32 weights only (got torch.float16)")
    if n == 0:
        return outs, None
    L = N.lib()
    wid = wavelet_id(wavelet)
    flags = ((WTP_CARRY_LEVEL if carry_level else 0) | (WTP_FLATTEN if flatten else 0)
             | (WTP_NO_RESIDENT if no_resident else 0))
    if half:
        nbytes = L.wtp_workspace_size_f16(desc, n, wid, int(level), flags, mid)
    elif mid:
        nbytes = L.wtp_workspace_size_mode(desc, n, wid, int(level), flags, mid)
    else:
        nbytes = L.wtp_workspace_size_ex(desc, n, wid, int(level), flags)
    stream = _current(device, stream)
    # the float16 entry's workspace is its own (include/wtprune.h)
    ws = workspace(device, nbytes if nbytes else 256, stream, kind="f16" if half else None)
    if results is None:
        res = _results(n, device, stream)
    else:
        if (results.dtype != torch.uint8 or not results.is_cuda or results.numel() < n * N.RESULT_BYTES
                or results.data_ptr() % 8):
            raise ValueError("wavelettransforms_amd: results must be %d 8-byte aligned CUDA bytes" % (n * N.RESULT_BYTES))
        res = results
    if half:
        rc = L.wtp_prune_f16(desc, n, wid, int(level), float(pct), flags, mid, ws.data_ptr(), ws.numel(),
                             res.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    elif mid:
        rc = L.wtp_prune_mode_f32(desc, n, wid, int(level), float(pct), flags, mid, ws.data_ptr(), ws.numel(),
                                  res.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    else:
        rc = L.wtp_prune_ex_f32(desc, n, wid, int(level), float(pct), flags, ws.data_ptr(), ws.numel(), res.data_ptr(),
                                ctypes.c_void_p(stream.cuda_stream))
    if rc != N.WTP_OK:
        raise_for(rc, tensors, wavelet)
    return outs, res


MODE_FAULT = 99  # WTP_PATH_FAULT: the resident launch timed out for this tensor and stored nothing
MODE_SMALL = 4   # WTP_PATH_SMALL: the whole call ran as one launch (csrc/small.hip)
MODE_HALF = 6    # WTP_PATH_HALF: a float16 tensor that got no transform (csrc/half.hip)


def carried_level(tensors, wavelet, level, flatten=False):
    """The level multi_resolution_analysis passes on after `tensors` (dwt_pruning.py:64-65: every
    tensor with ndim >= 2 clamps it to pywt.dwt_max_level of min(kh, kw) -- of numel in the
    flattened mode)."""
    L = N.lib()
    F = L.wtp_dec_len(wavelet_id(wavelet))
    lvl = int(level)
    for x in tensors:
        if x.dim() >= 2:
            n = x.numel() if flatten else min(x.shape[-2], x.shape[-1])
            lvl = min(lvl, int(L.wtp_max_level(int(n), int(F))))
    return lvl


def fault_mask(results_dev, n):
    """Per-tensor flags: True where the record reads MODE_FAULT (host copy of the records)."""
    host = results_dev.cpu().numpy().view(RESULT_DTYPE)[:n]
    return host["path"] == MODE_FAULT


def decode(results_dev, n):
    host = results_dev.cpu().numpy().view(RESULT_DTYPE)[:n]
    out = []
    if (host["path"] == MODE_FAULT).any():
        raise RuntimeError("wavelettransforms_amd: records of a resident launch that timed out (MODE_FAULT); "
                           "re-run those tensors with no_resident=True (prune() does this itself)")
    for r in host:
        d = {k: r[k].item() for k in RESULT_DTYPE.names}
        d["thr32"] = float(np.array(d["thr32_bits"], np.uint32).view(np.float32))
        d["max_abs"] = np.array(d["max_abs_bits"], np.uint32).view(np.float32)[()]
        if d["path"] == MODE_HALF:  # np.max of a float16 array
            d["max_abs"] = np.float16(d["max_abs"])
        d["nonzero"] = d["numel"] - d["zero_count"]
        out.append(d)
    return out


def set_resident(enabled):
    """Allow (default) or forbid the one-launch resident form of level-0 groups; returns the previous setting."""
    return bool(N.lib().wtp_set_resident(1 if enabled else 0))


def set_resident_early(mode):
    """Early stores of the resident launch (include/wtprune.h wtp_set_resident_early): True / 1 on
    (the default), False / 0 off, 2 on with the stores counted (resident_early_counts).  Identical
    results in every mode.  Returns the previous mode."""
    mode = (1 if mode else 0) if isinstance(mode, bool) else int(mode)
    prev = int(N.lib().wtp_set_resident_early(mode))
    if prev < 0:
        raise ValueError(N.last_error())
    return prev


def resident_early_counts(device="cuda", stream=None):
    """(early, deferred): the wave-wide float4 stores that resident launches on (device, stream)'s
    workspace issued on the bound / held back for the threshold since the last read, counted in
    mode 2 only; waits for the stream and clears the counters."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    if stream is None:
        stream = torch.cuda.current_stream(device)
    ws = workspace(device, 256, stream)
    a, b = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    rc = N.lib().wtp_resident_early_counts(ws.data_ptr(), ctypes.c_void_p(stream.cuda_stream), ctypes.byref(a),
                                           ctypes.byref(b))
    if rc != N.WTP_OK:
        raise RuntimeError("libwtprune: %s (status %d)" % (N.last_error(), rc))
    return int(a.value), int(b.value)


def set_pipeline(enabled):
    """Overlap each launch group's selection with the next group's forward transform on a side
    stream (True / 1, the default); False / 0 one stream (include/wtprune.h wtp_set_pipeline).
    Returns the previous mode."""
    mode = (1 if enabled else 0) if isinstance(enabled, bool) else int(enabled)
    return int(N.lib().wtp_set_pipeline(mode))


def set_fused_select(enabled):
    """Fused selection for launch groups of large wavelet-transformed tensors (True / 1, the
    default): the window from a transform of input patches before the forward, the forward
    classifying the coefficients it writes, no re-read of the packed array; False / 0 the
    window / collect / select passes over the packed array (include/wtprune.h
    wtp_set_fused_select).  Identical results either way.  Returns the previous mode."""
    return int(N.lib().wtp_set_fused_select(1 if enabled else 0))


def set_interior(enabled):
    """Filter-bank kernel choice (include/wtprune.h wtp_set_interior): 2 the interior tiles in the
    edge-free kernels and the frame around them in their edge form, True / 3 the same but a small
    level in one launch of the edge form (default), 1 the frame in the general kernel, False / 0
    every tile in the general kernel; returns the previous mode."""
    mode = (3 if enabled else 0) if isinstance(enabled, bool) else int(enabled)
    return int(N.lib().wtp_set_interior(mode))


def resident_capacity():
    """Workgroups (of 49152 weights) the resident launch can hold on the current device; 0: never used."""
    return int(N.lib().wtp_resident_capacity())


def prune(tensors, wavelet, level, pct, outs=None, carry_level=True, flatten=False, mode="periodization"):
    """launch() + wait + decoded per-tensor records (numel, zero_count, nonzero, thr64, ...).
    Tensors whose resident launch faulted (their inputs and outputs untouched) are re-run once in
    the three-launch form -- only those: a tensor pruned in place must not be pruned twice.  Under
    carry_level each one re-runs at the level the list carried into it (computed from the shapes
    of the tensors before it), as an independent call, grouped by that level."""
    outs, res = launch(tensors, wavelet, level, pct, outs=outs, carry_level=carry_level, flatten=flatten, mode=mode)
    if res is None:
        return outs, []
    n = len(tensors)
    bad = fault_mask(res, n)
    if bad.any():
        idx = [i for i in range(n) if bad[i]]
        groups = {}
        for i in idx:
            lvl = carried_level(tensors[:i], wavelet, level, flatten) if carry_level else int(level)
            groups.setdefault(lvl, []).append(i)
        merged = res.clone().view(n, N.RESULT_BYTES)
        for lvl, g in groups.items():
            _, res2 = launch([tensors[i] for i in g], wavelet, lvl, pct, outs=[outs[i] for i in g],
                             carry_level=False, flatten=flatten, no_resident=True, mode=mode)
            merged[g] = res2.view(len(g), N.RESULT_BYTES)
        res = merged.view(-1)
    return outs, decode(res, n)


ABS_RESULT_DTYPE = np.dtype([("numel", "<i8"), ("nonzero_in", "<i8"), ("nonzero_out", "<i8"), ("coeff_numel", "<i8"),
                             ("thr32_bits", "<u4"), ("level", "<i4"), ("path", "<i4"), ("reserved", "<i4")])
assert ABS_RESULT_DTYPE.itemsize == N.ABS_RESULT_BYTES
ABS_PATH_MASK, ABS_PATH_TINY, ABS_PATH_CHAIN = 0, 1, 2  # include/wtprune.h


def launch_abs(tensors, wavelet, level, threshold, outs=None, stream=None):
    """Enqueue the absolute-threshold method (dwt_pruning_NoEntropy.py:29-60, wtp_prune_abs_f32) for
    `tensors` (CUDA float32) on `stream` (default: the current stream): the wavelet transform at
    the requested level (no clamp), every packed coefficient with |c| < float32(threshold) set
    to zero, the inverse, the crop; ndim < 2 tensors are masked as they are.  Returns (outs,
    results_dev) without synchronising; results_dev is a uint8 CUDA tensor of len(tensors)
    wtp_abs_result records (decode_abs).  outs may be the inputs (in place)."""
    tensors, outs, n, device, desc = _prepare(tensors, outs)
    if n == 0:
        return outs, None
    L = N.lib()
    wid = wavelet_id(wavelet)
    stream = _current(device, stream)
    nbytes = L.wtp_abs_workspace_size(desc, n, wid, int(level))
    # scratch of this entry alone: never the selection entries' workspace (include/wtprune.h)
    ws = workspace(device, nbytes if nbytes else 256, stream, kind="abs")
    with torch.cuda.stream(stream):
        res = torch.empty(n * N.ABS_RESULT_BYTES, dtype=torch.uint8, device=device)
    rc = L.wtp_prune_abs_f32(desc, n, wid, int(level), float(threshold), ws.data_ptr(), ws.numel(), res.data_ptr(),
                             ctypes.c_void_p(stream.cuda_stream))
    if rc != N.WTP_OK:
        raise_for(rc, tensors, wavelet)
    return outs, res


def decode_abs(results_dev, n):
    """Host copies of n wtp_abs_result records as dicts (waits for the stream that wrote them)."""
    host = results_dev.cpu().numpy().view(ABS_RESULT_DTYPE)[:n]
    out = []
    for r in host:
        d = {k: r[k].item() for k in ABS_RESULT_DTYPE.names if k != "reserved"}
        d["thr32"] = float(np.array(d["thr32_bits"], np.uint32).view(np.float32))
        d["pruned"] = d["nonzero_in"] - d["nonzero_out"]
        out.append(d)
    return out


def prune_abs(tensors, wavelet, level, threshold, outs=None):
    """launch_abs() + wait + decoded per-tensor records (numel, nonzero_in, nonzero_out, pruned,
    coeff_numel, thr32, level, path)."""
    outs, res = launch_abs(tensors, wavelet, level, threshold, outs=outs)
    if res is None:
        return outs, []
    return outs, decode_abs(res, len(tensors))


WTP_ABS_SWEEP_MAX_THR = 8  # include/wtprune.h


def launch_abs_sweep(tensors, wavelet, level, thresholds, outs=None, stream=None):
    """Enqueue the absolute-threshold sweep (wtp_prune_abs_sweep_f32) for `tensors` (CUDA float32) on
    `stream` (default: the current stream): every tensor is read and transformed forward once,
    then each threshold's mask and inverse writes its output.  Returns (outs, results_dev) without
    synchronising: outs[k][t] is tensor t pruned at thresholds[k], bit for bit what
    launch_abs(tensors, wavelet, level, thresholds[k]) gives, and block k of results_dev
    (len(tensors) wtp_abs_result records) is that call's records.  At most eight thresholds; they
    may repeat and need not be sorted.  outs: a list over the thresholds of output lists; at most
    one output of a tensor may be the tensor itself."""
    thresholds = [float(v) for v in thresholds]
    nthr = len(thresholds)
    tensors, outs, n, device, desc = _prepare(tensors, outs, nthr, "thresholds")
    if n == 0:
        return outs, None
    L = N.lib()
    wid = wavelet_id(wavelet)
    stream = _current(device, stream)
    nbytes = L.wtp_abs_sweep_workspace_size(desc, n, wid, int(level), nthr)
    # scratch of the absolute-threshold entries alone: never the selection entries' workspace
    ws = workspace(device, nbytes if nbytes else 256, stream, kind="abs")
    with torch.cuda.stream(stream):
        res = torch.empty(max(1, nthr) * n * N.ABS_RESULT_BYTES, dtype=torch.uint8, device=device)
    tarr = (ctypes.c_double * max(1, nthr))(*thresholds)
    rc = L.wtp_prune_abs_sweep_f32(desc, n, wid, int(level), tarr, nthr, _out_ptrs(outs, n), ws.data_ptr(), ws.numel(),
                                   res.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    if rc != N.WTP_OK:
        raise_for(rc, tensors, wavelet)
    return outs, res


def prune_abs_sweep(tensors, wavelet, level, thresholds, outs=None):
    """launch_abs_sweep() + wait + decoded records: (outs, recs) with recs[k][t] the record of
    tensor t at thresholds[k] (decode_abs() of block k)."""
    thresholds = list(thresholds)
    outs, res = launch_abs_sweep(tensors, wavelet, level, thresholds, outs=outs)
    return outs, _decode_blocks(res, len(thresholds), len(tensors), N.ABS_RESULT_BYTES, decode_abs)


WTP_SWEEP_MAX_PCT, WTP_SWEEP_THRESHOLDS_ONLY, MODE_SWEEP = 8, 16, 5  # include/wtprune.h


def launch_sweep(tensors, wavelet, level, pcts, outs=None, carry_level=True, thresholds_only=False, stream=None):
    """Enqueue the percentile sweep (wtp_prune_sweep_f32) for `tensors` (CUDA float32) on `stream`
    (default: the current stream): one forward transform, one exact selection of every
    percentile's order statistics, then each percentile's mask or inverse.  Returns (outs,
    results_dev) without synchronising: outs[k][t] is tensor t pruned at pcts[k], bit for bit what
    launch(tensors, wavelet, level, pcts[k], carry_level=carry_level) gives, and block k of
    results_dev (len(tensors) wtp_result records) is that call's records with path == MODE_SWEEP.
    outs: a list over the percentiles of output lists; at most one output of a tensor may be the
    tensor itself.  thresholds_only=True stops after the selection: outs is None, the records
    carry the thresholds with zero_count 0."""
    pcts = [float(p) for p in pcts]
    npct = len(pcts)
    tensors, outs, n, device, desc = _prepare(tensors, outs, npct, "percentiles", no_outs=thresholds_only)
    if n == 0:
        return outs, None
    L = N.lib()
    wid = wavelet_id(wavelet)
    flags = (WTP_CARRY_LEVEL if carry_level else 0) | (WTP_SWEEP_THRESHOLDS_ONLY if thresholds_only else 0)
    stream = _current(device, stream)
    nbytes = L.wtp_sweep_workspace_size(desc, n, wid, int(level), npct, flags)
    # scratch of this entry alone: never the selection entries' workspace (include/wtprune.h)
    ws = workspace(device, nbytes if nbytes else 256, stream, kind="sweep")
    res = _results(max(1, npct) * n, device, stream)
    parr = (ctypes.c_double * max(1, npct))(*pcts)
    optr = None if outs is None else _out_ptrs(outs, n)
    rc = L.wtp_prune_sweep_f32(desc, n, wid, int(level), parr, npct, flags, optr, ws.data_ptr(), ws.numel(),
                               res.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    if rc != N.WTP_OK:
        raise_for(rc, tensors, wavelet)
    return outs, res


def prune_sweep(tensors, wavelet, level, pcts, outs=None, carry_level=True, thresholds_only=False):
    """launch_sweep() + wait + decoded records: (outs, recs) with recs[k][t] the record of tensor t
    at pcts[k] (decode() of block k)."""
    pcts = list(pcts)
    outs, res = launch_sweep(tensors, wavelet, level, pcts, outs=outs, carry_level=carry_level,
                             thresholds_only=thresholds_only)
    return outs, _decode_blocks(res, len(pcts), len(tensors), N.RESULT_BYTES, decode)


MODE_GLOBAL = 7  # include/wtprune.h: WTP_PATH_GLOBAL


def launch_global(tensors, wavelet, level, pcts, outs=None, carry_level=True, thresholds_only=False, stream=None):
    """Enqueue the global percentile (wtp_prune_global_f32) for `tensors` (CUDA float32) on `stream`
    (default: the current stream): one forward transform, then ONE threshold per percentile for
    the whole list -- the percentile of the pooled magnitudes of every tensor's coefficients (a
    tensor that gets no transform contributes its raw values) -- and each percentile's mask or
    inverse with it.  Returns (outs, results_dev) without synchronising, shaped as launch_sweep's:
    outs[k][t] is tensor t pruned at the pool's pcts[k]-th percentile, block k of results_dev holds
    len(tensors) wtp_result records with path == MODE_GLOBAL, whose thr64, thr32 and max_abs are
    the pool's (equal in every record of the block) and whose other fields are the tensor's own.
    At most eight percentiles; they may repeat and need not be sorted.  outs: a list over the
    percentiles of output lists; at most one output of a tensor may be the tensor itself.
    thresholds_only=True stops after the selection: outs is None, zero_count 0."""
    pcts = [float(p) for p in pcts]
    npct = len(pcts)
    tensors, outs, n, device, desc = _prepare(tensors, outs, npct, "percentiles", no_outs=thresholds_only)
    if n == 0:
        return outs, None
    L = N.lib()
    wid = wavelet_id(wavelet)
    flags = (WTP_CARRY_LEVEL if carry_level else 0) | (WTP_SWEEP_THRESHOLDS_ONLY if thresholds_only else 0)
    stream = _current(device, stream)
    nbytes = L.wtp_global_workspace_size(desc, n, wid, int(level), npct, flags)
    # scratch of this entry alone: never the selection entries' workspace (include/wtprune.h)
    ws = workspace(device, nbytes if nbytes else 256, stream, kind="global")
    res = _results(max(1, npct) * n, device, stream)
    parr = (ctypes.c_double * max(1, npct))(*pcts)
    optr = None if outs is None else _out_ptrs(outs, n)
    rc = L.wtp_prune_global_f32(desc, n, wid, int(level), parr, npct, flags, optr, ws.data_ptr(), ws.numel(),
                                res.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    if rc != N.WTP_OK:
        raise_for(rc, tensors, wavelet)
    return outs, res


def prune_global(tensors, wavelet, level, pcts, outs=None, carry_level=True, thresholds_only=False):
    """launch_global() + wait + decoded records: (outs, recs) with recs[k][t] the record of tensor t
    at the pool's pcts[k]-th percentile (decode() of block k)."""
    pcts = list(pcts)
    outs, res = launch_global(tensors, wavelet, level, pcts, outs=outs, carry_level=carry_level,
                              thresholds_only=thresholds_only)
    return outs, _decode_blocks(res, len(pcts), len(tensors), N.RESULT_BYTES, decode)


def min_prune(tensors, fraction, outs=None):
    """percentage_min_pruning (min_weight_pruning.py:66-74) of every tensor (CUDA float32) in one
    launch sequence: zero the int(numel * fraction) smallest |w|; ties at the boundary lowest
    flat index first.  Returns (outs, records); outs may be the inputs (in place)."""
    tensors, outs, n, device, desc = _prepare(tensors, outs)
    if n == 0:
        return outs, []
    L = N.lib()
    nbytes = L.wtp_min_prune_workspace_size(desc, n, float(fraction))
    ws = workspace(device, nbytes if nbytes else 256)
    res = torch.empty(n * N.RESULT_BYTES, dtype=torch.uint8, device=device)
    rc = L.wtp_min_prune_f32(desc, n, float(fraction), ws.data_ptr(), ws.numel(), res.data_ptr(),
                             ctypes.c_void_p(_current(device, None).cuda_stream))
    if rc != N.WTP_OK:
        msg = N.last_error()
        if rc == N.WTP_EARG and "NaN" in msg:
            raise ValueError(msg)
        if rc == N.WTP_EARG:
            raise RuntimeError(msg)  # torch.topk: "selected index k out of range"
        raise_for(rc, tensors, None)
    return outs, decode(res, n)


def random_prune(tensors, prune_counts, seed, outs=None):
    """random_pruning's per-layer step (random_pruning.py:53-56) for every tensor (CUDA float32)
    in one launch sequence: zero randperm(numel)[:k] -- k distinct flat positions of a keyed
    permutation (csrc/wt_perm.h; tensor index t keys tensor t).  Returns (outs, records)."""
    tensors, outs, n, device, desc = _prepare(tensors, outs)
    if n == 0:
        return outs, []
    if len(prune_counts) != n:
        raise ValueError("random_prune: %d prune counts for %d tensors" % (len(prune_counts), n))
    ks = (ctypes.c_int64 * n)(*[int(k) for k in prune_counts])
    res = torch.empty(n * N.RESULT_BYTES, dtype=torch.uint8, device=device)
    rc = N.lib().wtp_random_prune_f32(desc, n, ks, ctypes.c_uint64(int(seed) & (2**64 - 1)), res.data_ptr(),
                                      ctypes.c_void_p(_current(device, None).cuda_stream))
    if rc != N.WTP_OK:
        raise_for(rc, tensors, None)
    return outs, decode(res, n)


def count_small(x, thr):
    """#(|x| < thr) of a CUDA float32 tensor, thr rounded to float32 as torch's float compare does
    (calculate_sparsity, testing_suite/eval_model.py:14).  Returns a 0-d int64 CUDA tensor."""
    check_tensors([x])
    x = x.contiguous()
    cnt = torch.empty((), dtype=torch.int64, device=x.device)
    rc = N.lib().wtp_count_small_f32(x.data_ptr() if x.numel() else None, x.numel(), float(thr), cnt.data_ptr(),
                                     ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    if rc != N.WTP_OK:
        raise RuntimeError(N.last_error())
    return cnt


def threshold(x, pct, out=None):
    """percentile_based_thresholding (dwt_pruning.py:25-32) of a CUDA float32 tensor."""
    check_tensors([x])
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    else:
        check_outs([x], [out])
    L = N.lib()
    desc = _as_desc([x.reshape(-1)], [out.reshape(-1)])
    ws = workspace(x.device, L.wtp_workspace_size(desc, 1, -1, 0) or 256)
    res = torch.empty(N.RESULT_BYTES, dtype=torch.uint8, device=x.device)
    rc = L.wtp_threshold_f32(x.data_ptr() if x.numel() else None, out.data_ptr() if x.numel() else None,
                             x.numel(), float(pct), ws.data_ptr(), ws.numel(), res.data_ptr(),
                             ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    if rc != N.WTP_OK:
        raise_for(rc, [x], None)
    return out, decode(res, 1)[0]


def _wavedec2(x, wavelet, level, mid=None):
    """mid=None: the periodized C entries (which report an unknown wavelet differently); else WTP_MODE_*"""
    check_tensors([x])
    x = x.contiguous()
    L = N.lib()
    wid, level = wavelet_id(wavelet), int(level)
    H, W = x.shape[-2], x.shape[-1]
    B = x.numel() // max(1, H * W)
    pr, pc = ctypes.c_int64(), ctypes.c_int64()
    if mid is None:
        rc = L.wtp_packed_shape(H, W, level, ctypes.byref(pr), ctypes.byref(pc))
    else:
        rc = L.wtp_packed_shape_mode(H, W, wid, level, mid, ctypes.byref(pr), ctypes.byref(pc))
    if rc != 0:
        raise ValueError(N.last_error())
    P = torch.empty(tuple(x.shape[:-2]) + (pr.value, pc.value), dtype=torch.float32, device=x.device)
    ws = _component_ws(B, H, W, wid, level, mid, x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    if mid is None:
        rc = L.wtp_wavedec2_f32(x.data_ptr(), P.data_ptr(), B, H, W, wid, level, ws.data_ptr(), ws.numel(), stream)
    else:
        rc = L.wtp_wavedec2_mode_f32(x.data_ptr(), P.data_ptr(), B, H, W, wid, level, mid, ws.data_ptr(), ws.numel(), stream)
    if rc != 0:
        raise_for(rc, [x], wavelet)
    return P


def _waverec2(P, shape, wavelet, level, mid=None, thr32=None):
    L = N.lib()
    wid, level = wavelet_id(wavelet), int(level)
    H, W = shape[-2], shape[-1]
    B = 1
    for s in shape[:-2]:
        B *= s
    out = torch.empty(tuple(shape), dtype=torch.float32, device=P.device)
    ws = _component_ws(B, H, W, wid, level, mid, P.device)
    thr = None
    if thr32 is not None:
        thr = torch.tensor([thr32], dtype=torch.float32, device=P.device)
    thr_ptr = thr.data_ptr() if thr is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(P.device).cuda_stream)
    if mid is None:
        rc = L.wtp_waverec2_f32(P.contiguous().data_ptr(), out.data_ptr(), B, H, W, wid, level, thr_ptr, ws.data_ptr(),
                                ws.numel(), stream)
    else:
        rc = L.wtp_waverec2_mode_f32(P.contiguous().data_ptr(), out.data_ptr(), B, H, W, wid, level, mid, thr_ptr,
                                     ws.data_ptr(), ws.numel(), stream)
    if rc != 0:
        raise_for(rc, [P], wavelet)
    return out


def _component_ws(B, H, W, wid, level, mid, device):
    """the level temps of a component call"""
    L = N.lib()
    nb = L.wtp_dwt_workspace_size(B, H, W, level) if mid is None else L.wtp_dwt_workspace_size_mode(B, H, W, wid, level, mid)
    return torch.empty(max(nb, 256), dtype=torch.uint8, device=device)


def wavedec2_packed(x, wavelet, level):
    """pywt.coeffs_to_array(pywt.wavedec2(x, wavelet, level, 'periodization', axes=(-2,-1)))[0] on the GPU."""
    return _wavedec2(x, wavelet, level)


def waverec2_packed(P, shape, wavelet, level, thr32=None):
    """array_to_coeffs + waverec2 + crop to `shape` (optionally thresholding on load)."""
    return _waverec2(P, shape, wavelet, level, None, thr32)


def wavedec2_packed_mode(x, wavelet, level, mode):
    """pywt.coeffs_to_array(pywt.wavedec2(x, wavelet, mode, level, axes=(-2,-1)))[0] on the GPU
    (wtp_wavedec2_mode_f32: the level as given, padding cells zero)."""
    return _wavedec2(x, wavelet, level, mode_id(mode))


def waverec2_packed_mode(P, shape, wavelet, level, mode, thr32=None):
    """array_to_coeffs + waverec2(mode) + crop to `shape` (optionally thresholding on load)."""
    return _waverec2(P, shape, wavelet, level, mode_id(mode), thr32)


def synth(shape, seed, tensor_id, e, device="cuda"):
    """Synthetic weights on the device (csrc/wt_synth.h), identical to workloads.synth_numpy."""
    n = 1
    for s in shape:
        n *= s
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    rc = N.lib().wtp_synth_f32(out.data_ptr() if n else None, n, seed, tensor_id, int(e),
                               ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(N.last_error())
    return out

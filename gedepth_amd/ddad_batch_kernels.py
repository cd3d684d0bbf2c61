"""Wrappers of the batched DDAD entry points (csrc/infer.hip, csrc/eval.hip; include/gedepth_ddad_batch.h): ``infer_front_ddad_batch`` and
``depth_metric_sums_resized_batch`` — one launch (the metric sums: two) for up to ``BATCH_MAX`` frames, each frame with the bits of
``kernels.infer_front_ddad`` / ``kernels.depth_metric_sums_resized``.  ``kernels`` re-exports them; they launch through ``kernels._launch``
and live in a module of their own for the reason eval_kernels.py gives.  The frames' pointers and sizes go to the library as a host array of
``batch_kernels.GeBatchFrame``, as for the KITTI batch."""
import ctypes

import torch

from . import hip
from .batch_kernels import BATCH_MAX, _count, _table

_WS = {}                           # (device, stream, H, W) -> the partial-sum workspace of ge_depth_metrics_resized_batch, sized for BATCH_MAX images


def infer_front_ddad_batch(bgrs, pes, out, mean, std, to_rgb=True, pe_max=250.0, depth_scale=250.0):
    """DDAD test front end of n = ``len(bgrs)`` frames into the first n images of ``out`` (F, 5, Hd, Wd) f32, F >= n; the other images are
    not touched.  Per frame as ``kernels.infer_front_ddad``: ``bgrs[f]`` (H, W, 3) uint8, ``pes[f]`` (H, W) f32, the raw ground depth of
    that frame's camera; the frames may differ in size and in ground depth."""
    from .kernels import _front_args, _launch
    n = len(bgrs)
    _count(n, 'infer_front_ddad_batch')
    if len(pes) != n:
        raise ValueError(f'infer_front_ddad_batch: {n} frames and {len(pes)} ground depths')
    if out.dim() != 4 or out.shape[1] != 5 or out.shape[0] < n:
        raise ValueError(f'out must be (>= n = {n}, 5, Hd, Wd), got {tuple(out.shape)}')
    Hd, Wd = out.shape[2:]
    rows, nbytes = [], 0
    for bgr, pe in zip(bgrs, pes):
        H, W, m, s = _front_args(bgr, pe, mean, std)
        rows.append((hip.ptr(bgr, torch.uint8, 'bgr'), hip.ptr(pe, torch.float32, 'pe'), H, W, 0, 0))
        nbytes += 3 * H * W + 8 * Hd * Wd + 20 * Hd * Wd
    _launch(f'infer_front_ddad_batch[{n}]', nbytes, 'ge_infer_front_ddad_batch', ctypes.cast(_table(rows), ctypes.c_void_p), n,
            hip.ptr(out, torch.float32, 'out'), Hd, Wd, float(pe_max), ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
            float(depth_scale), int(bool(to_rgb)), hip.stream())
    return out


def depth_metric_sums_resized_batch(pred, gts, min_depth, max_depth, out):
    """The ten metric sums of n = ``len(gts)`` images under the DDAD protocol into the first n rows of ``out`` (>= n, 10) f64, on the
    current stream, without synchronising; the other rows are not touched.  ``pred``: (F, h, w) or (F, 1, h, w) f32, F >= n; ``gts[f]``:
    (H, W) f32 in metres, one size for all n (the library refuses mixed sizes as unsupported).  Every row carries the bits of
    ``kernels.depth_metric_sums_resized``."""
    from .kernels import _launch
    n = len(gts)
    _count(n, 'depth_metric_sums_resized_batch')
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 3 or pred.shape[0] < n:
        raise ValueError(f'pred must be (F, h, w) or (F, 1, h, w) with F >= {n} images, got {tuple(pred.shape)}')
    if out.dim() != 2 or out.shape[1] != 10 or out.shape[0] < n:
        raise ValueError(f'out must hold ten float64 sums for each of {n} images, got shape {tuple(out.shape)}')
    h, w = pred.shape[1:]
    p_pred, p_out = hip.ptr(pred, torch.float32, 'pred'), hip.ptr(out, torch.float64, 'out')
    rows = []
    for gt in gts:
        if gt.dim() != 2:
            raise ValueError(f'a ground truth must be (H, W), got {tuple(gt.shape)}')
        if gt.device != pred.device:
            raise RuntimeError(f'pred and a ground truth sit on {pred.device} and {gt.device}')
        rows.append((hip.ptr(gt, torch.float32, 'gt'), None, gt.shape[0], gt.shape[1], 0, 0))
    if out.device != pred.device:
        raise RuntimeError(f'pred and out sit on {pred.device} and {out.device}')
    H, W = gts[0].shape
    key = (pred.device, hip.stream(), H, W)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(hip.lib().ge_depth_metrics_resized_batch_workspace(BATCH_MAX, H, W) // 8, device=pred.device, dtype=torch.float64)
        _WS[key] = ws
    _launch(f'depth_metrics_resized_batch[{n}]', n * (4 * H * W + 4 * h * w) + 8 * ws.numel(), 'ge_depth_metrics_resized_batch', p_pred, h, w,
            ctypes.cast(_table(rows), ctypes.c_void_p), n, float(min_depth), float(max_depth), hip.ptr(ws), p_out, hip.stream())
    return out

"""Wrappers of the stratified KITTI metric sums (csrc/eval.hip; include/gedepth_strata.h): ``depth_metric_sums_strata`` and
``depth_metric_sums_strata_batch`` — the ten sums of ``kernels.depth_metric_sums`` per distance bin and per on / off ground class of the
ground truth, S = (len(edges) + 1) * (2 with a ground plane, else 1) rows per image, bin-major.  Row s carries the bits
``kernels.depth_metric_sums`` gives when the ground truth is 0 outside stratum s.  ``kernels`` re-exports them; they launch through
``kernels._launch`` and live in a module of their own for the reason eval_kernels.py gives."""
import ctypes
import math

import torch

from . import hip
from .batch_kernels import BATCH_MAX, _count, _table

MAX_EDGES = 7                      # GE_STRATA_MAX_EDGES of include/gedepth_strata.h
_WS = {}                           # (device, stream, Hc, Wc, S) -> the partial-sum workspace of ge_depth_metrics_strata (one image)
_WS_BATCH = {}                     # the same key -> that of ge_depth_metrics_strata_batch, sized for BATCH_MAX images


def strata_count(edges=(), ground=False):
    """S for these bin edges and with / without a ground plane."""
    S = hip.lib().ge_depth_strata_count(len(edges), int(bool(ground)))
    if S == 0:
        raise ValueError(f'strata take 0 .. {MAX_EDGES} bin edges, got {len(edges)}')
    return S


def _spec_args(edges, ground_tol):
    """The checks of the entry point in the caller's words -> (host float array or None, n_edges)."""
    edges = [float(e) for e in edges]
    if len(edges) > MAX_EDGES:
        raise ValueError(f'strata take 0 .. {MAX_EDGES} bin edges, got {len(edges)}')
    if any(not math.isfinite(e) for e in edges) or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f'bin edges must be finite and strictly ascending, got {edges}')
    if not 0.0 <= float(ground_tol) <= 1.0:                                # NaN fails both comparisons
        raise ValueError(f'ground_tol must lie in [0, 1], got {ground_tol}')
    return ((ctypes.c_float * len(edges))(*edges) if edges else None), len(edges)


def _workspace(cache, images, device, Hc, Wc, S):
    key = (device, hip.stream(), Hc, Wc, S)
    ws = cache.get(key)
    if ws is None:
        ws = torch.empty(hip.lib().ge_depth_metrics_strata_workspace(images, Hc, Wc, S) // 8, device=device, dtype=torch.float64)
        cache[key] = ws
    return ws


def depth_metric_sums_strata(pred, gt_raw, top, left, rect, depth_scale, min_depth, max_depth, out, edges=(), ground=None, ground_tol=0.1):
    """The ten metric sums of one image per stratum into ``out`` (S, 10) f64, on the current stream, without synchronising.

    ``pred``, ``gt_raw``, ``top``, ``left``, ``rect`` and the three depth parameters as in ``kernels.depth_metric_sums``.  ``edges``: up to
    seven finite, strictly ascending distances in metres; a ground truth on an edge belongs to the upper bin.  ``ground``: the frame's raw
    (H, W) f32 ground depth or None; a counted pixel is on the ground when ``g > 0 and |gt - g| <= ground_tol * g`` in float32.
    Stratum = bin * C + on_ground."""
    from .kernels import _launch
    if pred.dim() == 3 and pred.shape[0] == 1:
        pred = pred[0]
    if pred.dim() != 2 or gt_raw.dim() != 2:
        raise ValueError(f'pred must be (Hc, Wc) or (1, Hc, Wc) and gt_raw (H, W), got {tuple(pred.shape)} and {tuple(gt_raw.shape)}')
    c_edges, n_edges = _spec_args(edges, ground_tol)
    S = strata_count(edges, ground is not None)
    if tuple(out.shape) != (S, 10):
        raise ValueError(f'out must hold ten float64 sums for each of {S} strata, got shape {tuple(out.shape)}')
    if ground is not None and tuple(ground.shape) != tuple(gt_raw.shape):
        raise ValueError(f'ground must have the ground truth\'s shape {tuple(gt_raw.shape)}, got {tuple(ground.shape)}')
    Hc, Wc = pred.shape
    H, W = gt_raw.shape
    p_pred, p_gt, p_out = hip.ptr(pred, torch.float32, 'pred'), hip.ptr(gt_raw, torch.uint16, 'gt_raw'), hip.ptr(out, torch.float64, 'out')
    p_ground = hip.ptr(ground, torch.float32, 'ground')
    if not (pred.device == gt_raw.device == out.device) or (ground is not None and ground.device != pred.device):
        raise RuntimeError(f'pred, gt_raw, out and ground sit on {pred.device}, {gt_raw.device}, {out.device} and '
                           f'{None if ground is None else ground.device}')
    ws = _workspace(_WS, 1, pred.device, Hc, Wc, S)
    r0, r1, c0, c1 = (int(v) for v in rect)
    _launch(f'depth_metrics_strata[{S}]', S * 6 * Hc * Wc + 8 * ws.numel(),'ge_depth_metrics_strata', p_pred, p_gt, p_ground, H, W,
            int(top), int(left), Hc, Wc, r0, r1, c0, c1, float(depth_scale), float(min_depth), float(max_depth),
            ctypes.cast(c_edges, ctypes.c_void_p), n_edges, float(ground_tol), hip.ptr(ws), p_out, hip.stream())
    return out


def depth_metric_sums_strata_batch(pred, gts, tops, lefts, rect, depth_scale, min_depth, max_depth, out, edges=(), grounds=None,
                                   ground_tol=0.1):
    """``depth_metric_sums_strata`` of n = ``len(gts)`` images into the first n blocks of ``out`` (>= n, S, 10) f64, on the current stream,
    without synchronising; the other blocks are not touched.  ``pred``, ``gts``, ``tops``, ``lefts`` as in
    ``kernels.depth_metric_sums_batch``; ``grounds``: one (H, W) f32 ground depth per image, or None.  Each block carries the bits of
    ``depth_metric_sums_strata``."""
    from .kernels import _launch
    n = len(gts)
    _count(n, 'depth_metric_sums_strata_batch')
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 3 or pred.shape[0] < n or len(tops) != n or len(lefts) != n:
        raise ValueError(f'pred must be (F, Hc, Wc) or (F, 1, Hc, Wc) with F >= {n} images, one top and one left each, got {tuple(pred.shape)}')
    if grounds is not None and (len(grounds) != n or any(g is None for g in grounds)):
        raise ValueError(f'grounds must be None or one ground depth for each of {n} images')
    c_edges, n_edges = _spec_args(edges, ground_tol)
    S = strata_count(edges, grounds is not None)
    if out.dim() != 3 or tuple(out.shape[1:]) != (S, 10) or out.shape[0] < n:
        raise ValueError(f'out must hold ten float64 sums for each of {S} strata of {n} images, got shape {tuple(out.shape)}')
    Hc, Wc = pred.shape[1:]
    p_pred, p_out = hip.ptr(pred, torch.float32, 'pred'), hip.ptr(out, torch.float64, 'out')
    rows = []
    for f, (gt, top, left) in enumerate(zip(gts, tops, lefts)):
        ground = None if grounds is None else grounds[f]
        if gt.dim() != 2 or (ground is not None and tuple(ground.shape) != tuple(gt.shape)):
            raise ValueError(f'a ground truth must be (H, W) and its ground depth of the same shape, got {tuple(gt.shape)} and '
                             f'{None if ground is None else tuple(ground.shape)}')
        if gt.device != pred.device or (ground is not None and ground.device != pred.device):
            raise RuntimeError(f'pred and a ground truth or ground depth sit on {pred.device} and {gt.device}')
        rows.append((hip.ptr(gt, torch.uint16, 'gt_raw'), hip.ptr(ground, torch.float32, 'ground'), gt.shape[0], gt.shape[1], top, left))
    if out.device != pred.device:
        raise RuntimeError(f'pred and out sit on {pred.device} and {out.device}')
    ws = _workspace(_WS_BATCH, BATCH_MAX, pred.device, Hc, Wc, S)
    r0, r1, c0, c1 = (int(v) for v in rect)
    _launch(f'depth_metrics_strata_batch[{n},{S}]', n * S * 6 * Hc * Wc + 8 * ws.numel(), 'ge_depth_metrics_strata_batch', p_pred,
            ctypes.cast(_table(rows), ctypes.c_void_p), n, Hc, Wc, r0, r1, c0, c1, float(depth_scale), float(min_depth), float(max_depth),
            ctypes.cast(c_edges, ctypes.c_void_p), n_edges, float(ground_tol), hip.ptr(ws), p_out, hip.stream())
    return out

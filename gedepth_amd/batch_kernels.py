"""Wrappers of the batched KITTI entry points (csrc/infer.hip, csrc/eval.hip; include/gedepth_batch.h): ``infer_front_batch``, ``tta_merge_batch`` and
``depth_metric_sums_batch`` — one launch (the metric sums: two) for up to ``BATCH_MAX`` frames, each frame with the bits of
``kernels.infer_front`` / ``kernels.tta_merge`` / ``kernels.depth_metric_sums``.  ``kernels`` re-exports them; they launch through
``kernels._launch`` and live in a module of their own for the reason eval_kernels.py gives.

``GeBatchFrame`` mirrors the C struct of the header: the frames' pointers and geometry go to the library as a host array of these, which
the entry point copies into the kernel's argument block during the call (no device-side table; the array is free again on return)."""
import ctypes

import torch

from . import hip

BATCH_MAX = 8                      # GE_BATCH_MAX of include/gedepth_batch.h
_WS = {}                           # (device, stream, Hc, Wc) -> the partial-sum workspace of ge_depth_metrics_batch, sized for BATCH_MAX images


class GeBatchFrame(ctypes.Structure):
    _fields_ = [('image', ctypes.c_void_p), ('aux', ctypes.c_void_p), ('H', ctypes.c_int), ('W', ctypes.c_int), ('top', ctypes.c_int),
                ('left', ctypes.c_int)]


def _count(n, what):
    if not 1 <= n <= BATCH_MAX:
        raise ValueError(f'{what}: a batch holds 1 .. {BATCH_MAX} frames, got {n}')


def _table(rows):
    """[(image pointer, aux pointer or None, H, W, top, left)] -> a ctypes array of GeBatchFrame."""
    return (GeBatchFrame * len(rows))(*[GeBatchFrame(image, aux, int(H), int(W), int(top), int(left)) for image, aux, H, W, top, left in rows])


def infer_front_batch(bgrs, pes, out, tops, lefts, mean, std, views=2, to_rgb=True, pe_max=200.0, depth_scale=200.0):
    """KITTI test front end of n = ``len(bgrs)`` frames into the first ``views * n`` images of ``out`` (views * F, 5, Hc, Wc) f32, F >= n,
    frame-major (view v of frame f is image ``views * f + v``); the other images are not touched.  Per frame as ``kernels.infer_front``:
    ``bgrs[f]`` (H, W, 3) uint8, ``pes[f]`` (H, W) f32, the window at (``tops[f]``, ``lefts[f]``); the frames may differ in size."""
    from .kernels import _front_args, _launch
    n = len(bgrs)
    _count(n, 'infer_front_batch')
    if not (len(pes) == len(tops) == len(lefts) == n):
        raise ValueError(f'infer_front_batch: {n} frames, {len(pes)} ground depths, {len(tops)} tops and {len(lefts)} lefts')
    if views not in (1, 2) or out.dim() != 4 or out.shape[1] != 5 or out.shape[0] < views * n:
        raise ValueError(f'out must be (>= views * n = {views * n}, 5, Hc, Wc) with views 1 or 2, got {tuple(out.shape)}')
    Hc, Wc = out.shape[2:]
    rows = []
    for bgr, pe, top, left in zip(bgrs, pes, tops, lefts):
        H, W, m, s = _front_args(bgr, pe, mean, std)
        rows.append((hip.ptr(bgr, torch.uint8, 'bgr'), hip.ptr(pe, torch.float32, 'pe'), H, W, top, left))
    nbytes = n * (7 * Hc * Wc + 20 * views * Hc * Wc)
    _launch(f'infer_front_batch[{n}]', nbytes, 'ge_infer_front_batch', ctypes.cast(_table(rows), ctypes.c_void_p), n,
            hip.ptr(out, torch.float32, 'out'), Hc, Wc, int(views), float(pe_max), ctypes.cast(m, ctypes.c_void_p),
            ctypes.cast(s, ctypes.c_void_p), float(depth_scale), int(bool(to_rgb)), hip.stream())
    return out


def tta_merge_batch(pred, out, n=None):
    """``pred`` (2 F, 1, H, W) f32, the two flip views of F frames, frame-major -> ``out`` (F, 1, H, W) f32, per frame
    (pred[2 f] + mirror(pred[2 f + 1])) / 2 as ``kernels.tta_merge``.  ``n`` <= F: only the first n frames are merged and written."""
    from .kernels import _launch
    if pred.dim() != 4 or pred.shape[1] != 1 or pred.shape[0] % 2:
        raise ValueError(f'pred must be (2 F, 1, H, W), got {tuple(pred.shape)}')
    F, (H, W) = pred.shape[0] // 2, pred.shape[2:]
    n = F if n is None else int(n)
    _count(n, 'tta_merge_batch')
    if n > F or tuple(out.shape) != (F, 1, H, W):
        raise ValueError(f'out must be {(F, 1, H, W)} and n <= {F}, got {tuple(out.shape)} and n = {n}')
    _launch(f'tta_merge_batch[{n}]', 12 * n * H * W, 'ge_tta_merge_batch', hip.ptr(pred, torch.float32, 'pred'), hip.ptr(out, torch.float32, 'out'),
            n, H, W, hip.stream())
    return out


def depth_metric_sums_batch(pred, gts, tops, lefts, rect, depth_scale, min_depth, max_depth, out):
    """The ten metric sums of n = ``len(gts)`` images into the first n rows of ``out`` (>= n, 10) f64, on the current stream, without
    synchronising; the other rows are not touched.  ``pred``: (F, Hc, Wc) or (F, 1, Hc, Wc) f32, F >= n; ``gts[f]``: (H, W) uint16, read in
    the window at (``tops[f]``, ``lefts[f]``); ``rect`` and the three depth parameters as in ``kernels.depth_metric_sums``, whose bits
    every row carries."""
    from .kernels import _launch
    n = len(gts)
    _count(n, 'depth_metric_sums_batch')
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 3 or pred.shape[0] < n or len(tops) != n or len(lefts) != n:
        raise ValueError(f'pred must be (F, Hc, Wc) or (F, 1, Hc, Wc) with F >= {n} images, one top and one left each, got {tuple(pred.shape)}')
    if out.dim() != 2 or out.shape[1] != 10 or out.shape[0] < n:
        raise ValueError(f'out must hold ten float64 sums for each of {n} images, got shape {tuple(out.shape)}')
    Hc, Wc = pred.shape[1:]
    p_pred, p_out = hip.ptr(pred, torch.float32, 'pred'), hip.ptr(out, torch.float64, 'out')
    rows = []
    for gt, top, left in zip(gts, tops, lefts):
        if gt.dim() != 2:
            raise ValueError(f'a ground truth must be (H, W), got {tuple(gt.shape)}')
        if gt.device != pred.device:
            raise RuntimeError(f'pred and a ground truth sit on {pred.device} and {gt.device}')
        rows.append((hip.ptr(gt, torch.uint16, 'gt_raw'), None, gt.shape[0], gt.shape[1], top, left))
    if out.device != pred.device:
        raise RuntimeError(f'pred and out sit on {pred.device} and {out.device}')
    key = (pred.device, hip.stream(), Hc, Wc)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(hip.lib().ge_depth_metrics_batch_workspace(BATCH_MAX, Hc, Wc) // 8, device=pred.device, dtype=torch.float64)
        _WS[key] = ws
    r0, r1, c0, c1 = (int(v) for v in rect)
    _launch(f'depth_metrics_batch[{n}]', n * (6 * Hc * Wc) + 8 * ws.numel(), 'ge_depth_metrics_batch', p_pred,
            ctypes.cast(_table(rows), ctypes.c_void_p), n, Hc, Wc, r0, r1, c0, c1, float(depth_scale), float(min_depth), float(max_depth),
            hip.ptr(ws), p_out, hip.stream())
    return out

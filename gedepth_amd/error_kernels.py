"""Wrappers of the error images and the split-level error planes (csrc/error.hip; include/gedepth_error.h): ``error_image`` /
``error_image_batch`` paint every LiDAR return of a KITTI frame with the band of its abs-rel error over the frame's own pixels (one launch),
``error_accumulate`` / ``error_accumulate_batch`` add the abs-rel error of every return into a per-pixel float64 sum and uint32 count (one
launch, no atomics: the planes equal a sequential float64 sum in frame order).  The header states the arithmetic.  ``kernels`` re-exports
them; they launch through ``kernels._launch`` and live in a module of their own for the reason eval_kernels.py gives.

numpy in -> numpy out (uploaded to the current device, the result copied back); CUDA tensors in -> CUDA tensors out on the current
stream, without synchronising.  Every argument error is raised in the caller's words before any device work."""
import ctypes

import numpy as np
import torch

from . import hip
from .batch_kernels import BATCH_MAX, _count, _table

MAX_RADIUS = 3                     # GE_ERROR_MAX_RADIUS of include/gedepth_error.h
BACKGROUNDS = (0, 1, 2)            # the frame as it is, every channel >> 1, black


def paint_args(tau=0.05, radius=1, background=1):
    """The checks of the entry points in the caller's words -> ``(tau, radius, background)`` as float, int, int."""
    try:
        t = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f'tau must be a number in (0, 1], got {tau!r}') from None
    if not 0.0 < t <= 1.0:                                                 # NaN fails both comparisons
        raise ValueError(f'tau must lie in (0, 1], got {tau}')
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f'radius must be an integer in 0 .. {MAX_RADIUS}, got {radius!r}')
    if isinstance(background, bool) or not isinstance(background, (int, np.integer)) or background not in BACKGROUNDS:
        raise ValueError(f'background must be 0 (the frame), 1 (the frame, halved) or 2 (black), got {background!r}')
    return t, int(radius), int(background)


def _rect(rect, Hc, Wc):
    r0, r1, c0, c1 = (int(v) for v in rect)
    if not (0 <= r0 <= Hc and 0 <= r1 <= Hc and 0 <= c0 <= Wc and 0 <= c1 <= Wc):
        raise ValueError(f'the rectangle {(r0, r1, c0, c1)} leaves the {(Hc, Wc)} crop')
    return r0, r1, c0, c1


def _is_host(*arrays):
    """All numpy (True) or all tensors (False); a mix is a TypeError."""
    kinds = {torch.is_tensor(a) for a in arrays if a is not None}
    if len(kinds) != 1:
        raise TypeError('pass numpy arrays throughout (numpy comes back) or CUDA tensors throughout (CUDA tensors come back)')
    return not kinds.pop()


def _up(a, dtype):
    if a is None:
        return None
    dev = torch.device('cuda', torch.cuda.current_device())
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dtype)).to(dev)


def _one_pred(pred):
    if pred.ndim == 3 and pred.shape[0] == 1:
        pred = pred[0]
    if pred.ndim != 2:
        raise ValueError(f'pred must be (Hc, Wc) or (1, Hc, Wc), got {tuple(pred.shape)}')
    return pred


def _batch_pred(pred, n, what):
    if pred.ndim == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.ndim != 3 or pred.shape[0] < n:
        raise ValueError(f'{what}: pred must be (F, Hc, Wc) or (F, 1, Hc, Wc) with F >= {n} images, got {tuple(pred.shape)}')
    return pred


def _frame_shapes(gt, image, Hc, Wc, top, left):
    if gt.ndim != 2:
        raise ValueError(f'a ground truth must be (H, W), got {tuple(gt.shape)}')
    H, W = gt.shape
    if image is not None and tuple(image.shape) != (H, W, 3):
        raise ValueError(f'the frame must be (H, W, 3) = {(H, W, 3)} like its ground truth, got {tuple(image.shape)}')
    if top < 0 or left < 0 or top + Hc > H or left + Wc > W:
        raise ValueError(f'the {(Hc, Wc)} window at {(int(top), int(left))} leaves the {(H, W)} frame')
    return H, W


def error_image(pred, gt_raw, image, top, left, rect, depth_scale, min_depth, max_depth, tau=0.05, radius=1, background=1, want_err=True,
                out=None):
    """One image -> ``(out, err)``: ``out`` (Hc, Wc, 3) uint8 BGR (written into the CUDA tensor ``out=`` when one is given), ``err``
    (Hc, Wc) float32 (None with ``want_err=False``).

    ``pred`` (Hc, Wc) or (1, Hc, Wc) f32, ``gt_raw`` (H, W) uint16 read in the window at (``top``, ``left``), ``rect`` and the three depth
    parameters as in ``kernels.depth_metric_sums``; ``image`` the frame's (H, W, 3) uint8 BGR pixels (None only with ``background=2``).
    A counted pixel's n = (|gt - pred| / gt) / tau falls into one of ten bands (thresholds 1/16 .. 16, a NaN counts as +inf) and is painted
    in ColorBrewer RdYlBu-10, blue for small errors; an output pixel shows the largest n within ``radius`` (0 .. 3) in both directions,
    and where there is none the frame's pixel: ``background`` 0 as it is, 1 halved, 2 black.  ``err``: |gt - pred| / gt at the counted
    pixels (NaN kept), -1 elsewhere."""
    from .kernels import _launch
    tau, radius, background = paint_args(tau, radius, background)
    if image is None and background != 2:
        raise ValueError('error_image: background 0 and 1 show the frame: pass image=, or background=2')
    host = _is_host(pred, gt_raw, image)
    pred = _one_pred(pred)
    Hc, Wc = pred.shape
    H, W = _frame_shapes(gt_raw, image, Hc, Wc, top, left)
    r0, r1, c0, c1 = _rect(rect, Hc, Wc)
    if host:
        pred, gt_raw, image = _up(pred, np.float32), _up(gt_raw, np.uint16), _up(image, np.uint8)
    p_pred, p_gt, p_img = hip.ptr(pred, torch.float32, 'pred'), hip.ptr(gt_raw, torch.uint16, 'gt_raw'), hip.ptr(image, torch.uint8, 'image')
    if gt_raw.device != pred.device or (image is not None and image.device != pred.device):
        raise RuntimeError(f'pred, gt_raw and image sit on {pred.device}, {gt_raw.device} and {None if image is None else image.device}')
    if out is None:
        out = torch.empty(Hc, Wc, 3, device=pred.device, dtype=torch.uint8)
    elif host or tuple(out.shape) != (Hc, Wc, 3) or out.device != pred.device:
        raise ValueError(f'out must be a ({Hc}, {Wc}, 3) CUDA tensor beside pred (numpy inputs get a fresh numpy result), got '
                         f'{tuple(out.shape)}')
    err = torch.empty(Hc, Wc, device=pred.device, dtype=torch.float32) if want_err else None
    _launch(f'error_image[{radius}]', Hc * Wc * (6 + 3 + 3 + (4 if want_err else 0)), 'ge_error_image', p_pred, p_gt, p_img, H, W, int(top), int(left),
            Hc, Wc, r0, r1, c0, c1, float(depth_scale), float(min_depth), float(max_depth), tau, radius, background,
            hip.ptr(out, torch.uint8, 'out'), hip.ptr(err), hip.stream())
    if host:
        return out.cpu().numpy(), (None if err is None else err.cpu().numpy())
    return out, err


def _batch_rows(pred, gts, images, tops, lefts, what):
    """The frame table of a batch and its argument errors -> ``(rows, n)``; ``images`` None: no aux."""
    n = len(gts)
    if len(tops) != n or len(lefts) != n or (images is not None and len(images) != n):
        raise ValueError(f'{what}: {n} ground truths need one top, one left and one frame each')
    Hc, Wc = pred.shape[1:]
    rows = []
    for f, (gt, top, left) in enumerate(zip(gts, tops, lefts)):
        image = None if images is None else images[f]
        H, W = _frame_shapes(gt, image, Hc, Wc, top, left)
        if gt.device != pred.device or (image is not None and image.device != pred.device):
            raise RuntimeError(f'pred and a ground truth or frame sit on {pred.device} and {gt.device}')
        rows.append((hip.ptr(gt, torch.uint16, 'gt_raw'), hip.ptr(image, torch.uint8, 'image'), H, W, top, left))
    return rows


def error_image_batch(pred, gts, images, tops, lefts, rect, depth_scale, min_depth, max_depth, tau=0.05, radius=1, background=1, want_err=True,
                      out=None, err=None):
    """``error_image`` of n = ``len(gts)`` images in the same single launch -> ``(out, err)``: (n, Hc, Wc, 3) uint8 and (n, Hc, Wc) float32,
    block f with the bytes ``error_image`` gives image f.  ``pred`` (F, Hc, Wc) or (F, 1, Hc, Wc) f32 with F >= n and Wc % 4 == 0;
    ``gts[f]`` (H, W) uint16, ``images[f]`` its (H, W, 3) uint8 frame (an entry, or ``images`` itself, may be None only with
    ``background=2``); the frames may differ in size.  ``out`` / ``err``: CUDA tensors of >= n blocks to write the first n of; the other
    blocks are not touched."""
    from .kernels import _launch
    tau, radius, background = paint_args(tau, radius, background)
    n = len(gts)
    _count(n, 'error_image_batch')
    if images is not None and len(images) != n:
        raise ValueError(f'error_image_batch: {n} ground truths and {len(images)} frames')
    if background != 2 and (images is None or any(i is None for i in images)):
        raise ValueError('error_image_batch: background 0 and 1 show the frames: every image needs its frame, or background=2')
    host = _is_host(pred, *gts, *(images or ()))
    pred = _batch_pred(pred, n, 'error_image_batch')
    Hc, Wc = pred.shape[1:]
    r0, r1, c0, c1 = _rect(rect, Hc, Wc)
    if host:
        if out is not None or err is not None:
            raise TypeError('error_image_batch: out= / err= are CUDA tensors; numpy inputs get fresh numpy results')
        for f in range(n):
            _frame_shapes(gts[f], None if images is None else images[f], Hc, Wc, tops[f], lefts[f])
        pred, gts = _up(pred, np.float32), [_up(g, np.uint16) for g in gts]
        images = None if images is None else [_up(i, np.uint8) for i in images]
    rows = _batch_rows(pred, gts, images, tops, lefts, 'error_image_batch')
    p_pred = hip.ptr(pred, torch.float32, 'pred')
    if out is None:
        out = torch.empty(n, Hc, Wc, 3, device=pred.device, dtype=torch.uint8)
    elif out.dim() != 4 or tuple(out.shape[1:]) != (Hc, Wc, 3) or out.shape[0] < n:
        raise ValueError(f'out must be (>= {n}, {Hc}, {Wc}, 3), got {tuple(out.shape)}')
    if err is None:
        err = torch.empty(n, Hc, Wc, device=pred.device, dtype=torch.float32) if want_err else None
    elif err.dim() != 3 or tuple(err.shape[1:]) != (Hc, Wc) or err.shape[0] < n:
        raise ValueError(f'err must be (>= {n}, {Hc}, {Wc}), got {tuple(err.shape)}')
    p_out, p_err = hip.ptr(out, torch.uint8, 'out'), hip.ptr(err, torch.float32, 'err')
    if out.device != pred.device or (err is not None and err.device != pred.device):
        raise RuntimeError(f'pred, out and err sit on {pred.device}, {out.device} and {None if err is None else err.device}')
    _launch(f'error_image_batch[{n},{radius}]', n * Hc * Wc * (6 + 3 + 3 + (4 if err is not None else 0)), 'ge_error_image_batch', p_pred,
            ctypes.cast(_table(rows), ctypes.c_void_p), n, Hc, Wc, r0, r1, c0, c1, float(depth_scale), float(min_depth), float(max_depth), tau,
            radius, background, p_out, p_err, hip.stream())
    if host:
        return out.cpu().numpy(), (None if err is None else err.cpu().numpy())
    return out, err


def _planes(sum, count, Hc, Wc, host):
    """The accumulators' argument errors -> the device planes (uploaded copies of numpy planes)."""
    if tuple(sum.shape) != (Hc, Wc) or tuple(count.shape) != (Hc, Wc):
        raise ValueError(f'sum and count must be {(Hc, Wc)} planes, got {tuple(sum.shape)} and {tuple(count.shape)}')
    if host:
        if sum.dtype != np.float64 or count.dtype != np.uint32:
            raise TypeError(f'sum must be float64 and count uint32, got {sum.dtype} and {count.dtype}')
        return _up(sum, np.float64), _up(count, np.uint32)
    return sum, count


def _planes_back(host, d_sum, d_count, sum, count):
    if host:
        sum[...] = d_sum.cpu().numpy()
        count[...] = d_count.cpu().numpy()
    return sum, count


def error_accumulate(pred, gt_raw, top, left, rect, depth_scale, min_depth, max_depth, sum, count):
    """One image into the planes, in place -> ``(sum, count)``: at every counted pixel with a FINITE e = |gt - pred| / gt,
    ``sum += float64(e)`` and ``count += 1``; a NaN or infinite e enters neither.  ``sum`` (Hc, Wc) float64, ``count`` (Hc, Wc) uint32; the
    other arguments as in ``error_image``."""
    from .kernels import _launch
    host = _is_host(pred, gt_raw, sum, count)
    pred = _one_pred(pred)
    Hc, Wc = pred.shape
    H, W = _frame_shapes(gt_raw, None, Hc, Wc, top, left)
    r0, r1, c0, c1 = _rect(rect, Hc, Wc)
    d_sum, d_count = _planes(sum, count, Hc, Wc, host)
    if host:
        pred, gt_raw = _up(pred, np.float32), _up(gt_raw, np.uint16)
    p_pred, p_gt = hip.ptr(pred, torch.float32, 'pred'), hip.ptr(gt_raw, torch.uint16, 'gt_raw')
    p_sum, p_count = hip.ptr(d_sum, torch.float64, 'sum'), hip.ptr(d_count, torch.uint32, 'count')
    if not (pred.device == gt_raw.device == d_sum.device == d_count.device):
        raise RuntimeError(f'pred, gt_raw, sum and count sit on {pred.device}, {gt_raw.device}, {d_sum.device} and {d_count.device}')
    _launch('error_accumulate', Hc * Wc * 6, 'ge_error_accumulate', p_pred, p_gt, H, W, int(top), int(left), Hc, Wc, r0, r1, c0, c1,
            float(depth_scale), float(min_depth), float(max_depth), p_sum, p_count, hip.stream())
    return _planes_back(host, d_sum, d_count, sum, count)


def error_accumulate_batch(pred, gts, tops, lefts, rect, depth_scale, min_depth, max_depth, sum, count):
    """n = ``len(gts)`` images into the planes in one launch, image 0 first: the bits of n ``error_accumulate`` calls in index order.
    ``pred`` (F, Hc, Wc) or (F, 1, Hc, Wc) f32 with F >= n and Wc % 4 == 0."""
    from .kernels import _launch
    n = len(gts)
    _count(n, 'error_accumulate_batch')
    host = _is_host(pred, *gts, sum, count)
    pred = _batch_pred(pred, n, 'error_accumulate_batch')
    Hc, Wc = pred.shape[1:]
    r0, r1, c0, c1 = _rect(rect, Hc, Wc)
    if len(tops) != n or len(lefts) != n:
        raise ValueError(f'error_accumulate_batch: {n} ground truths need one top and one left each')
    for f in range(n):
        _frame_shapes(gts[f], None, Hc, Wc, tops[f], lefts[f])
    d_sum, d_count = _planes(sum, count, Hc, Wc, host)
    if host:
        pred, gts = _up(pred, np.float32), [_up(g, np.uint16) for g in gts]
    rows = _batch_rows(pred, gts, None, tops, lefts, 'error_accumulate_batch')
    p_pred = hip.ptr(pred, torch.float32, 'pred')
    p_sum, p_count = hip.ptr(d_sum, torch.float64, 'sum'), hip.ptr(d_count, torch.uint32, 'count')
    if not (pred.device == d_sum.device == d_count.device):
        raise RuntimeError(f'pred, sum and count sit on {pred.device}, {d_sum.device} and {d_count.device}')
    _launch(f'error_accumulate_batch[{n}]', n * Hc * Wc * 6, 'ge_error_accumulate_batch', p_pred, ctypes.cast(_table(rows), ctypes.c_void_p), n,
            Hc, Wc, r0, r1, c0, c1, float(depth_scale), float(min_depth), float(max_depth), p_sum, p_count, hip.stream())
    return _planes_back(host, d_sum, d_count, sum, count)

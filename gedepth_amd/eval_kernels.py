"""Wrappers of the entry points the HIP library declares outside include/gedepth_hip.h: the KITTI metric sums (csrc/eval.hip,
include/gedepth_eval.h) and the DDAD test protocol (include/gedepth_ddad.h: ``ge_depth_metrics_resized`` of csrc/eval.hip,
``ge_infer_front_ddad`` of csrc/infer.hip).  ``kernels.depth_metric_sums``, ``kernels.depth_metric_sums_resized`` and
``kernels.infer_front_ddad`` are these functions: they launch through ``kernels._launch`` like every other wrapper, and live in a module of
their own because kernels.py holds the entry points of include/gedepth_hip.h (tests/test_kernels_memguard_gpu.py reads their names out of
that file)."""
import ctypes

import torch

from . import hip

_WS = {}                           # (device, stream, Hc, Wc[, 'resized']) -> the partial-sum workspace of ge_depth_metrics[_resized]


def depth_metric_sums(pred, gt_raw, top, left, rect, depth_scale, min_depth, max_depth, out):
    """The ten metric sums of one image into ``out`` (10,) f64 (a row of an (N, 10) buffer), on the current stream, without synchronising.

    ``pred``: (Hc, Wc) or (1, Hc, Wc) f32 CUDA prediction.  ``gt_raw``: (H, W) uint16 CUDA tensor, the undivided ground-truth PNG, read in
    the (Hc, Wc) window at (``top``, ``left``) as ``float32(raw) / depth_scale``.  ``rect`` = (r0, r1, c0, c1): rows / columns of the crop that
    count (``KITTIDataset.eval_rect``), together with ``min_depth < gt < max_depth``.  Sums: n, the three threshold counts, sum |d| / gt,
    sum d^2 / gt, sum d^2, sum l, sum l^2, sum |log10 gt - log10 pred| (``depth.core.metrics_from_sums`` turns them into the metric tuple)."""
    from .kernels import _launch
    if pred.dim() == 3 and pred.shape[0] == 1:
        pred = pred[0]
    if pred.dim() != 2 or gt_raw.dim() != 2:
        raise ValueError(f'pred must be (Hc, Wc) or (1, Hc, Wc) and gt_raw (H, W), got {tuple(pred.shape)} and {tuple(gt_raw.shape)}')
    if tuple(out.shape) != (10,):
        raise ValueError(f'out must hold ten float64 sums, got shape {tuple(out.shape)}')
    Hc, Wc = pred.shape
    H, W = gt_raw.shape
    p_pred, p_gt, p_out = hip.ptr(pred, torch.float32, 'pred'), hip.ptr(gt_raw, torch.uint16, 'gt_raw'), hip.ptr(out, torch.float64, 'out')
    if not (pred.device == gt_raw.device == out.device):
        raise RuntimeError(f'pred, gt_raw and out sit on {pred.device}, {gt_raw.device} and {out.device}')
    key = (pred.device, hip.stream(), Hc, Wc)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(hip.lib().ge_depth_metrics_workspace(Hc, Wc) // 8, device=pred.device, dtype=torch.float64)
        _WS[key] = ws
    r0, r1, c0, c1 = (int(v) for v in rect)
    _launch('depth_metrics', 4 * Hc * Wc + 2 * Hc * Wc + 8 * ws.numel(), 'ge_depth_metrics', p_pred, p_gt, H, W, int(top), int(left), Hc, Wc,
            r0, r1, c0, c1, float(depth_scale), float(min_depth), float(max_depth), hip.ptr(ws), p_out, hip.stream())
    return out


def depth_metric_sums_resized(pred, gt, min_depth, max_depth, out):
    """The ten metric sums of one image under the DDAD protocol into ``out`` (10,) f64, on the current stream, without synchronising.

    ``pred``: (h, w) or (1, h, w) f32 CUDA prediction.  ``gt``: (H, W) f32 CUDA ground truth in metres.  The kernel resamples ``pred`` at the
    ground-truth pixels (bilinear, align_corners=True, float32: include/gedepth_ddad.h states the arithmetic) where
    ``min_depth < gt < max_depth`` and reduces in the same pass; the resized map is never written.  Sums as in ``depth_metric_sums``."""
    from .kernels import _launch
    if pred.dim() == 3 and pred.shape[0] == 1:
        pred = pred[0]
    if pred.dim() != 2 or gt.dim() != 2:
        raise ValueError(f'pred must be (h, w) or (1, h, w) and gt (H, W), got {tuple(pred.shape)} and {tuple(gt.shape)}')
    if tuple(out.shape) != (10,):
        raise ValueError(f'out must hold ten float64 sums, got shape {tuple(out.shape)}')
    h, w = pred.shape
    H, W = gt.shape
    p_pred, p_gt, p_out = hip.ptr(pred, torch.float32, 'pred'), hip.ptr(gt, torch.float32, 'gt'), hip.ptr(out, torch.float64, 'out')
    if not (pred.device == gt.device == out.device):
        raise RuntimeError(f'pred, gt and out sit on {pred.device}, {gt.device} and {out.device}')
    key = (pred.device, hip.stream(), H, W, 'resized')
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(hip.lib().ge_depth_metrics_resized_workspace(H, W) // 8, device=pred.device, dtype=torch.float64)
        _WS[key] = ws
    _launch('depth_metrics_resized', 4 * H * W + 4 * h * w + 8 * ws.numel(), 'ge_depth_metrics_resized', p_pred, h, w, p_gt, H, W,
            float(min_depth), float(max_depth), hip.ptr(ws), p_out, hip.stream())
    return out


def infer_front_ddad(bgr, pe, out, mean, std, to_rgb=True, pe_max=250.0, depth_scale=250.0):
    """DDAD test front end into ``out`` (1, 5, Hd, Wd) f32: the uint8 HWC BGR frame ``bgr`` (H, W, 3) area-averaged to (Hd, Wd) and
    normalised, and its camera's raw ground depth ``pe`` (H, W) f32 resized nearest-neighbour into channels 3 (clamped to [0, pe_max],
    / depth_scale) and 4 (raw), like LoadDDADImageFromFile -> DDADResize -> Normalize of the host test pipeline.  ``mean`` / ``std``: three
    floats each (widened to float64 as Normalize does with its float32 arrays)."""
    from .kernels import _front_args, _launch
    H, W, m, s = _front_args(bgr, pe, mean, std)
    if out.dim() != 4 or tuple(out.shape[:2]) != (1, 5):
        raise ValueError(f'out must be (1, 5, Hd, Wd), got {tuple(out.shape)}')
    Hd, Wd = out.shape[2:]
    _launch('infer_front_ddad', 3 * H * W + 8 * Hd * Wd + 20 * Hd * Wd, 'ge_infer_front_ddad', hip.ptr(bgr, torch.uint8, 'bgr'),
            hip.ptr(pe, torch.float32, 'pe'), hip.ptr(out, torch.float32, 'out'), H, W, Hd, Wd, float(pe_max),
            ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), float(depth_scale), int(bool(to_rgb)), hip.stream())
    return out

"""Wrapper of the evaluation entry point of the HIP library (csrc/eval.hip, include/gedepth_eval.h).  ``kernels.depth_metric_sums`` is this
function: it launches through ``kernels._launch`` like every other wrapper, and lives in a module of its own because kernels.py holds the
entry points of include/gedepth_hip.h (tests/test_kernels_memguard_gpu.py reads their names out of that file)."""
import torch

from . import hip

_WS = {}                           # (device, stream, Hc, Wc) -> the partial-sum workspace of ge_depth_metrics


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

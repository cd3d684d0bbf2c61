"""numpy float32 restatement of ``ge_depth_metrics_resized``'s resampling (include/gedepth_ddad.h) for the DDAD device-evaluation tests
(imported like ``eval_ref``): bilinear, align_corners=True, every intermediate an ``np.float32``, rows then columns.

It is NOT ``F.interpolate`` on the CPU: ATen evaluates the same weights and taps in another order, and the two agree in 60-73 % of the
pixels; tests/test_ddad_device_cpu.py measures the gap (largest relative difference 3.4e-7 on 384 x 640 -> 1216 x 1936, values 1 .. 150)."""
import numpy as np

GEOMETRIES = (((5, 7), (13, 18)), ((12, 20), (37, 61)), ((12, 20), (36, 64)), ((48, 80), (200, 532)), ((8, 12), (8, 12)), ((4, 4), (1, 1)),
              ((6, 8), (1, 16)), ((6, 8), (16, 1)))                       # (pred, ground truth) sizes of the kernel tests
HOST_BAND = 1e-6        # three times the measured gap: about eight float32 ulps for seven rounded operations evaluated in two orders


def _axis(n_in, n_out):
    """(i0, i1, w0, w1) of every destination index: scale = f32(n_in - 1) / f32(n_out - 1) (0 for one output), src = scale * f32(dst)."""
    f = np.float32
    scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    src = scale * np.arange(n_out, dtype=np.float32)
    assert src.dtype == np.float32
    i0 = src.astype(np.int32)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = src - i0.astype(np.float32)
    w0 = f(1) - w1
    return i0, i1, w0, w1


def resize_f32(pred, H, W):
    """The (H, W) float32 map the kernel forms pixel by pixel: wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11)."""
    pred = np.asarray(pred, np.float32)
    h, w = pred.shape
    y0, y1, wy0, wy1 = _axis(h, H)
    x0, x1, wx0, wx1 = _axis(w, W)
    wy0, wy1, wx0, wx1 = wy0[:, None], wy1[:, None], wx0[None, :], wx1[None, :]
    with np.errstate(all='ignore'):
        top = wx0 * pred[y0][:, x0] + wx1 * pred[y0][:, x1]
        bot = wx0 * pred[y1][:, x0] + wx1 * pred[y1][:, x1]
        out = wy0 * top + wy1 * bot
    assert out.dtype == np.float32
    return out


def resize_host(pred, H, W):
    """What ``DDADDataset.pre_eval`` forms: ATen's CPU ``F.interpolate``."""
    import torch
    import torch.nn.functional as F
    return F.interpolate(torch.from_numpy(np.asarray(pred, np.float32))[None, None], size=(H, W), mode='bilinear', align_corners=True)[0, 0].numpy()


def mask_of(gt, min_depth=1e-3, max_depth=200):
    gt = np.asarray(gt, np.float32)
    return np.logical_and(gt > np.float32(min_depth), gt < np.float32(max_depth))


def near_threshold(gt, pred, p, band):
    """How many of the pixels have a host ratio within ``band`` (relative) of 1.25 ** p."""
    with np.errstate(all='ignore'):
        ratio = np.maximum(gt / pred, pred / gt).astype(np.float64)
    t = 1.25 ** p
    return int((np.abs(ratio - t) <= band * t).sum())

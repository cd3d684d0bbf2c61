"""Wrapper of the ground-map entry point (csrc/ground.hip, include/gedepth_ground.h).  ``kernels.ground_maps`` is this function: it launches
through ``kernels._launch`` like every other wrapper, and lives in a module of its own for the reason eval_kernels.py gives (kernels.py holds
the entry points of include/gedepth_hip.h)."""
import torch

from . import hip

PLANES = ('attention', 'ground_term', 'ground_depth', 'slope_deg')       # the planes of ``maps``, in order


def ground_maps(logits_lr, y_lr, img, height=None, depth_scale=200.0, gain=200.0, flip=True, out=None, valid=None):
    """The ground embedding's maps of one frame, merged over its V (1 or 2) views, on the current stream and without synchronising ->
    ``(maps, valid)``: ``maps`` (4, H, W) f32 with the planes ``PLANES`` and ``valid`` (H, W) uint8, the number of views whose ground
    depth is valid (include/gedepth_ground.h has the arithmetic).

    ``logits_lr``: the (V, 11, h, w) slope logits of the dynamic-PE neck, or None for the vanilla model; ``y_lr``: the (V, 1, h, w) ground
    attention of the PE-mask neck; both are cast to contiguous float32 as the model's own ground embedding casts them.  ``img``: the
    (V, 5, H, W) f32 network input; the adaptive model reads its channel 4 (raw ground depth), the vanilla one its channel 3.  ``height``:
    None (1.65 m) or a device tensor with V camera heights.  ``flip``: with two views, view 1 is the horizontally mirrored frame.
    ``out`` / ``valid``: contiguous buffers to write into."""
    from .kernels import _launch
    if not (img.is_cuda and y_lr.is_cuda and (logits_lr is None or logits_lr.is_cuda)):
        raise RuntimeError('ground_maps: gedepth_amd ops run on MI355X only; got a CPU tensor')
    if img.dim() != 4 or img.shape[1] != 5 or img.dtype != torch.float32 or not img.is_contiguous():
        raise TypeError(f'img must be a contiguous (V, 5, H, W) float32 tensor, got {tuple(img.shape)} {img.dtype}')
    V, _, H, W = img.shape
    if V not in (1, 2):
        raise ValueError(f'ground_maps merges one or two views, got {V}')
    y_lr = y_lr.to(torch.float32).contiguous()
    if y_lr.dim() != 4 or y_lr.shape[:2] != (V, 1):
        raise ValueError(f'y_lr must be ({V}, 1, h, w), got {tuple(y_lr.shape)}')
    h, w = y_lr.shape[2:]
    if logits_lr is not None:
        logits_lr = logits_lr.to(torch.float32).contiguous()
        if tuple(logits_lr.shape) != (V, 11, h, w):
            raise ValueError(f'logits_lr must be {(V, 11, h, w)}, got {tuple(logits_lr.shape)}')
    if height is not None:
        height = height.to(torch.float32).contiguous()
        if height.numel() != V:
            raise ValueError(f'height must hold one value per view ({V}), got {height.numel()}')
    if out is None:
        out = torch.empty(4, H, W, device=img.device, dtype=torch.float32)
    if valid is None:
        valid = torch.empty(H, W, device=img.device, dtype=torch.uint8)
    if tuple(out.shape) != (4, H, W) or tuple(valid.shape) != (H, W):
        raise ValueError(f'out / valid must be {(4, H, W)} / {(H, W)}, got {tuple(out.shape)} / {tuple(valid.shape)}')
    pe = img[:, 4 if logits_lr is not None else 3]
    nbytes = 17 * H * W + 4 * V * H * W + 4 * V * h * w * (12 if logits_lr is not None else 1)
    _launch(f'ground_maps[{V}x{H}x{W}]', nbytes, 'ge_ground_maps', hip.ptr(logits_lr, torch.float32, 'logits_lr'),
            hip.ptr(y_lr, torch.float32, 'y_lr'), pe.data_ptr(), img.stride(0), hip.ptr(height, torch.float32, 'height'), float(depth_scale),
            float(gain), int(bool(flip)), hip.ptr(out, torch.float32, 'out'), hip.ptr(valid, torch.uint8, 'valid'), V, h, w, H, W, hip.stream())
    return out, valid

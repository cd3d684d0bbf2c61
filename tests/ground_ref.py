"""Plain torch restatement of ``ge_ground_maps`` (include/gedepth_ground.h) for any float dtype, imported like ``f64ref``.

The per-view quantities follow the reference's encoder_decoder.py:79-102 as ``oracle.dynamic_pe`` restates them (plus the vanilla line
:122); then view 1 is mirrored back and the views are merged.  At float64 it is the reference of tests/test_ground_maps_gpu.py, at float32
on the CPU its yardstick: how far float32 arithmetic alone lands from float64 on the same inputs."""
import torch
import torch.nn.functional as F

PLANES = ('attention', 'ground_term', 'ground_depth', 'slope_deg')


def per_view(logits_lr, y_lr, img, height=None, depth_scale=200.0, gain=200.0, dtype=torch.float64):
    """Each view at its own pixels -> dict of (V, H, W) tensors ``y``, ``t``, ``off``, ``deg`` (``dtype``) and ``ok`` (bool).
    ``logits_lr`` None: the vanilla model, which reads channel 3 of ``img``; else channel 4."""
    H, W = img.shape[2:]
    y = F.interpolate(y_lr.to(dtype), size=(H, W), mode='bilinear')[:, 0]
    if logits_lr is None:
        pe = img[:, 3].to(dtype)
        return dict(y=y, t=pe * y * gain, off=pe * gain, deg=torch.zeros_like(y), ok=pe > 0)
    pe = img[:, 4].to(dtype)
    logits = F.interpolate(logits_lr.to(dtype), size=(H, W), mode='bilinear')
    k = F.softmax(logits, dim=1)
    deg = torch.sum(k * torch.linspace(-5, 5, 11).view(1, 11, 1, 1).to(dtype), dim=1)
    k = torch.tan(torch.deg2rad(deg))
    h = 1.65 if height is None else torch.as_tensor(height).to(dtype).view(-1, 1, 1)
    a = -h / (pe + 1e-8)
    off = -h / ((a - k) + 1e-8)
    m = off.clone()
    m[m < 0] = 0
    m[m > depth_scale] = 0
    m[m > 0] = 1
    return dict(y=y, t=(off * m) * y, off=off, deg=deg, ok=m == 1)


def merge(views, flip=True):
    """``per_view``'s dict -> ``(maps (4, H, W), valid (H, W) uint8)``: view 1 mirrored back when ``flip``, then the table of the header."""
    V = views['y'].shape[0]
    a = {k: v[0] for k, v in views.items()}
    if V == 1:
        gd = torch.where(a['ok'], a['off'], torch.zeros_like(a['off']))
        return torch.stack((a['y'], a['t'], gd, a['deg'])), a['ok'].to(torch.uint8)
    b = {k: (v[1].flip(-1) if flip else v[1]) for k, v in views.items()}
    zero = torch.zeros_like(a['off'])
    gd = torch.where(a['ok'] & b['ok'], (a['off'] + b['off']) * 0.5,
                     torch.where(a['ok'], a['off'], torch.where(b['ok'], b['off'], zero)))
    maps = torch.stack(((a['y'] + b['y']) * 0.5, (a['t'] + b['t']) * 0.5, gd, (a['deg'] + b['deg']) * 0.5))
    return maps, a['ok'].to(torch.uint8) + b['ok'].to(torch.uint8)


def ground_maps(logits_lr, y_lr, img, height=None, depth_scale=200.0, gain=200.0, flip=True, dtype=torch.float64):
    return merge(per_view(logits_lr, y_lr, img, height, depth_scale, gain, dtype), flip)


def ambiguous(logits_lr, y_lr, img, height=None, flip=True):
    """(H, W) bool: output pixels where a view's validity is numerically undecided — its float64 offset within 2e-2 of 200, within 1e-6 of
    0, or not finite (the set of test_kernels_gpu.py::test_ground_embed_adaptive), in either view."""
    off = per_view(logits_lr, y_lr, img, height)['off']
    amb = ((off - 200.0).abs() < 2e-2) | (off.abs() < 1e-6) | ~torch.isfinite(off)
    if amb.shape[0] == 1:
        return amb[0]
    return amb[0] | (amb[1].flip(-1) if flip else amb[1])

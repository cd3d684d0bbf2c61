"""Wrapper of the prior sweep's front end (csrc/infer.hip; include/gedepth_sweep.h): ``infer_front_sweep`` writes one KITTI frame into
V = ``len(variants)`` slots of a batched engine's input that differ only in their two ground channels — one launch, the frame read once.
The header states the perturbation rule.  ``kernels`` re-exports it; it launches through ``kernels._launch`` and lives in a module of
its own for the reason eval_kernels.py gives.

``GePriorVariant`` mirrors the C struct of the header: the variants go to the library as a host array of these, which the entry point
copies into the kernel's argument block during the call (no device-side table; the array is free again on return)."""
import ctypes
import math

import torch

from . import hip

SWEEP_MAX = 8                      # GE_SWEEP_MAX of include/gedepth_sweep.h (= GE_BATCH_MAX)


class GePriorVariant(ctypes.Structure):
    _fields_ = [('c', ctypes.c_float), ('s', ctypes.c_float), ('drop', ctypes.c_int)]


def variant_table(variants):
    """[(c, s, drop)] -> a ctypes array of GePriorVariant; the entry point's own checks in the caller's words."""
    rows = [(float(c), float(s), int(bool(drop))) for c, s, drop in variants]
    if not 1 <= len(rows) <= SWEEP_MAX:
        raise ValueError(f'infer_front_sweep: a sweep holds 1 .. {SWEEP_MAX} variants, got {len(rows)}')
    for c, s, _ in rows:
        if not math.isfinite(c) or not math.isfinite(s) or not s > 0.0:
            raise ValueError(f'infer_front_sweep: a variant needs a finite c and a finite s > 0, got c = {c}, s = {s}')
    return (GePriorVariant * len(rows))(*[GePriorVariant(c, s, drop) for c, s, drop in rows])


def infer_front_sweep(bgr, pe, variants, out, top, left, mean, std, views=2, to_rgb=True, pe_max=200.0, depth_scale=200.0):
    """KITTI test front end of ONE frame into the first ``views * V`` images of ``out`` (views * F, 5, Hc, Wc) f32, F >= V =
    ``len(variants)``: view w of variant v is image ``views * v + w``, with the bits ``kernels.infer_front`` writes for the frame when it is
    given the plane the rule of include/gedepth_sweep.h makes of ``pe`` under ``variants[v]`` = ``(c, s, drop)``; the other images are not
    touched.  ``bgr`` (H, W, 3) uint8, ``pe`` (H, W) f32, the window at (``top``, ``left``)."""
    from .kernels import _front_args, _launch
    table = variant_table(variants)
    n = len(table)
    if views not in (1, 2) or out.dim() != 4 or out.shape[1] != 5 or out.shape[0] < views * n:
        raise ValueError(f'out must be (>= views * V = {views * n}, 5, Hc, Wc) with views 1 or 2, got {tuple(out.shape)}')
    Hc, Wc = out.shape[2:]
    H, W, m, s = _front_args(bgr, pe, mean, std)
    p_bgr, p_pe, p_out = hip.ptr(bgr, torch.uint8, 'bgr'), hip.ptr(pe, torch.float32, 'pe'), hip.ptr(out, torch.float32, 'out')
    _launch(f'infer_front_sweep[{n}]', 7 * Hc * Wc + n * 20 * views * Hc * Wc, 'ge_infer_front_sweep', p_bgr, p_pe, H, W, int(top), int(left),
            ctypes.cast(table, ctypes.c_void_p), n, p_out, Hc, Wc, int(views), float(pe_max), ctypes.cast(m, ctypes.c_void_p),
            ctypes.cast(s, ctypes.c_void_p), float(depth_scale), int(bool(to_rgb)), hip.stream())
    return out

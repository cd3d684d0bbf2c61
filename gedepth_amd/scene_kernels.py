"""Wrapper of the scene-cloud entry point (csrc/scene.hip, include/gedepth_scene.h).  ``kernels.scene_points`` is this function: it launches
through ``kernels._launch`` like every other wrapper, and lives in a module of its own for the reason eval_kernels.py gives.

``GeSceneLayer`` mirrors the C struct of the header: the layers go to the library as a host array of these, which the entry point copies
into the kernel's argument block during the call (no device-side table; the array is free again on return).  ``SceneLayer`` is the
descriptor a caller writes."""
import ctypes

import torch

from . import hip
from .cloud_kernels import cloud_capacity

SCENE_MAX_LAYERS = 4               # GE_SCENE_MAX_LAYERS of include/gedepth_scene.h
SCENE_F32, SCENE_U16 = 0, 1        # GE_SCENE_F32, GE_SCENE_U16
_KINDS = {'f32': (SCENE_F32, torch.float32), 'u16': (SCENE_U16, torch.uint16)}


class GeSceneLayer(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('kind', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int), ('top', ctypes.c_int),
                ('left', ctypes.c_int), ('scale', ctypes.c_float), ('dmin', ctypes.c_float), ('dmax', ctypes.c_float),
                ('from_frame', ctypes.c_int), ('red', ctypes.c_ubyte), ('green', ctypes.c_ubyte), ('blue', ctypes.c_ubyte),
                ('reserved', ctypes.c_ubyte)]


class SceneLayer:
    """One layer of ``scene_points``: ``data`` an (H_l, W_l) CUDA tensor, float32 for ``kind='f32'``, uint16 for ``kind='u16'`` (then
    z = raw / ``scale`` in float32); candidate (r, c) reads element (``top`` + r, ``left`` + c); kept iff ``min_depth <= z <= max_depth``;
    ``colour``: an (R, G, B) triple, or None for the frame's colour (white without a frame)."""

    def __init__(self, data, kind='f32', min_depth=1e-3, max_depth=80.0, colour=None, top=0, left=0, scale=1.0):
        self.data, self.kind, self.min_depth, self.max_depth = data, kind, float(min_depth), float(max_depth)
        self.colour, self.top, self.left, self.scale = colour, int(top), int(left), float(scale)


def _table(rows):
    """[(pointer, kind code, H, W, top, left, scale, dmin, dmax, colour or None)] -> a ctypes array of GeSceneLayer."""
    out = (GeSceneLayer * len(rows))()
    for e, (data, kind, H, W, top, left, scale, dmin, dmax, colour) in zip(out, rows):
        r, g, b = colour if colour is not None else (0, 0, 0)
        e.data, e.kind, e.H, e.W, e.top, e.left = data, kind, int(H), int(W), int(top), int(left)
        e.scale, e.dmin, e.dmax, e.from_frame, e.red, e.green, e.blue, e.reserved = scale, dmin, dmax, int(colour is None), r, g, b, 0
    return out


def scene_points(layers, fx, fy, cx, cy, H, W, bgr=None, top=0, left=0, row0=0, step=1, alpha=255):
    """The points of ``layers`` (1 .. 4 ``SceneLayer``) over one (H, W) candidate grid -> ``(records, counts)`` on the current stream, without
    synchronising.  Candidates, the keep rule and the 16-byte record are ``depth_points``'s, per layer with its own range, window and colour.
    ``records``: (L * capacity, 16) uint8, ``capacity = ceil((H - row0) / step) * ceil(W / step)``: all kept points of layer 0 in row-major
    candidate order, then all of layer 1, and so on, with no holes; rows from ``counts[L]`` on are not written.  ``counts``: (L + 1,) int32,
    the layers' kept counts and their total.  ``fx, fy, cx, cy``: intrinsics in MAP coordinates.  ``bgr``: (Hs, Ws, 3) uint8 CUDA frame
    whose pixel (top + r, left + c) colours candidate (r, c) of a layer without a colour of its own; None: white."""
    from .kernels import _launch
    layers = list(layers)
    L = len(layers)
    if not 1 <= L <= SCENE_MAX_LAYERS:
        raise ValueError(f'scene_points: a scene holds 1 .. {SCENE_MAX_LAYERS} layers, got {L}')
    H, W, row0, step = int(H), int(W), int(row0), int(step)
    if H <= 0 or W <= 0:
        raise ValueError(f'scene_points: the map size must be positive, got {(H, W)}')
    rows, device = [], None
    for k, ly in enumerate(layers):
        if ly.kind not in _KINDS:
            raise ValueError(f'layer {k}: kind must be \'f32\' or \'u16\', got {ly.kind!r}')
        code, dtype = _KINDS[ly.kind]
        d = ly.data
        if not torch.is_tensor(d) or d.dtype != dtype:
            raise TypeError(f'layer {k}: a {ly.kind} layer takes a {dtype} tensor, got {d.dtype if torch.is_tensor(d) else type(d).__name__}')
        if d.dim() != 2:
            raise ValueError(f'layer {k}: data must be (H, W), got {tuple(d.shape)}')
        if device is None:
            device = d.device
        elif d.device != device:
            raise RuntimeError(f'layer 0 and layer {k} sit on {device} and {d.device}')
        Hl, Wl = d.shape
        if ly.top < 0 or ly.left < 0 or ly.top + H > Hl or ly.left + W > Wl:
            raise ValueError(f'layer {k}: the {(H, W)} window at {(ly.top, ly.left)} leaves the {(Hl, Wl)} array')
        if ly.colour is not None and (len(ly.colour) != 3 or not all(0 <= int(v) <= 255 for v in ly.colour)):
            raise ValueError(f'layer {k}: colour must be three values in 0 .. 255 or None, got {ly.colour!r}')
        colour = None if ly.colour is None else tuple(int(v) for v in ly.colour)
        rows.append((d, dtype, code, Hl, Wl, ly.top, ly.left, ly.scale, ly.min_depth, ly.max_depth, colour))
    Hs = Ws = 0
    if bgr is not None:
        if bgr.dtype != torch.uint8 or bgr.dim() != 3 or bgr.shape[2] != 3:
            raise TypeError(f'bgr must be a (Hs, Ws, 3) uint8 tensor, got {tuple(bgr.shape)} {bgr.dtype}')
        if bgr.device != device:
            raise RuntimeError(f'the layers and bgr sit on {device} and {bgr.device}')
        Hs, Ws = bgr.shape[:2]
        if top < 0 or left < 0 or top + H > Hs or left + W > Ws:
            raise ValueError(f'the {(H, W)} window at {(top, left)} leaves the {(Hs, Ws)} frame')
    rows = [(hip.ptr(d, dtype, f'layer {k}'), *row) for k, (d, dtype, *row) in enumerate(rows)]      # the argument errors above come first
    p_bgr = hip.ptr(bgr, torch.uint8, 'bgr')
    nbytes = hip.lib().ge_scene_points_workspace(H, W, row0, step, L)
    if nbytes == 0:
        raise ValueError(f'scene_points: row0 = {row0} must lie in [0, {H}) and step = {step} must be >= 1 (map {(H, W)})')
    capacity = cloud_capacity(H, W, row0, step)
    records = torch.empty(L * capacity, 16, device=device, dtype=torch.uint8)
    counts = torch.empty(L + 1, device=device, dtype=torch.int32)
    ws = torch.empty(nbytes // 4, device=device, dtype=torch.int32)
    _launch(f'scene_points[{L}]', L * (2 * 4 * capacity + 19 * capacity) + 2 * nbytes, 'ge_scene_points', ctypes.cast(_table(rows), ctypes.c_void_p),
            L, H, W, p_bgr, Hs, Ws, int(top), int(left), float(fx), float(fy), float(cx), float(cy), row0, step, int(alpha), hip.ptr(records),
            hip.ptr(counts), hip.ptr(ws), hip.stream())
    return records, counts

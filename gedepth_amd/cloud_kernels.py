"""Wrapper of the point-cloud entry point (csrc/scene.hip, include/gedepth_cloud.h).  ``kernels.depth_points`` is this function: it launches
through ``kernels._launch`` like every other wrapper, and lives in a module of its own for the reason eval_kernels.py gives (kernels.py holds
the entry points of include/gedepth_hip.h)."""
import torch

from . import hip


def cloud_capacity(H, W, row0=0, step=1):
    """The number of candidates: ``ceil((H - row0) / step) * ceil(W / step)``."""
    return -(-(H - row0) // step) * -(-W // step)


def depth_points(depth, fx, fy, cx, cy, bgr=None, top=0, left=0, min_depth=1e-3, max_depth=80.0, row0=0, step=1, alpha=255):
    """Back-project ``depth`` ((H, W) or (1, H, W) f32 CUDA tensor) into ``(records, count)`` on the current stream, without synchronising.

    Candidates are the map pixels (r, c) with r = row0, row0 + step, ... and c = 0, step, ..., in row-major order; one is kept iff
    ``min_depth <= z <= max_depth`` (NaN fails).  ``records``: (capacity, 16) uint8, ``capacity = ceil((H - row0) / step) * ceil(W / step)``;
    row k is the k-th kept point: x = ((float)c - cx) / fx * z, y = ((float)r - cy) / fy * z, z as three little-endian float32 (numpy's
    float32 arithmetic, bit for bit), then the bytes R, G, B, alpha.  Rows from ``count`` on are not written.  ``count``: (1,) int32, the
    number of kept points.  ``fx, fy, cx, cy``: intrinsics in MAP coordinates.  ``bgr``: (Hs, Ws, 3) uint8 CUDA frame whose pixel
    (top + r, left + c) colours map pixel (r, c); None: white."""
    from .kernels import _launch
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2:
        raise ValueError(f'depth must be (H, W) or (1, H, W), got {tuple(depth.shape)}')
    if depth.is_cuda and not depth.is_contiguous():
        depth = depth.contiguous()
    H, W = depth.shape
    p_depth = hip.ptr(depth, torch.float32, 'depth')
    Hs = Ws = 0
    if bgr is not None:
        if bgr.dtype != torch.uint8 or bgr.dim() != 3 or bgr.shape[2] != 3:
            raise TypeError(f'bgr must be a (Hs, Ws, 3) uint8 tensor, got {tuple(bgr.shape)} {bgr.dtype}')
        if bgr.device != depth.device:
            raise RuntimeError(f'depth and bgr sit on {depth.device} and {bgr.device}')
        Hs, Ws = bgr.shape[:2]
    p_bgr = hip.ptr(bgr, torch.uint8, 'bgr')
    row0, step = int(row0), int(step)
    nbytes = hip.lib().ge_depth_points_workspace(H, W, row0, step)
    if nbytes == 0:
        raise ValueError(f'depth_points: row0 = {row0} must lie in [0, {H}) and step = {step} must be >= 1 (map {(H, W)})')
    capacity = cloud_capacity(H, W, row0, step)
    records = torch.empty(capacity, 16, device=depth.device, dtype=torch.uint8)
    count = torch.empty(1, device=depth.device, dtype=torch.int32)
    ws = torch.empty(nbytes // 4, device=depth.device, dtype=torch.int32)
    _launch('depth_points', 2 * 4 * capacity + 19 * capacity + 2 * nbytes, 'ge_depth_points', p_depth, H, W, p_bgr, Hs, Ws, int(top), int(left),
            float(fx), float(fy), float(cx), float(cy), float(min_depth), float(max_depth), row0, step, int(alpha), hip.ptr(records),
            hip.ptr(count), hip.ptr(ws), hip.stream())
    return records, count

"""Point clouds from depth maps (tools/misc/visualize_point-cloud_kitti.py of the reference): ``depth_to_points`` back-projects the pixels
whose depth is in range through the camera intrinsics and colours them from the frame; ``write_ply`` stores them as a binary
little-endian PLY file; ``kitti_intrinsics`` finds a KITTI frame's intrinsics.  ``write_scene_ply`` stores a scene cloud — several layers
in one record buffer (``kernels.scene_points``, gedepth_amd/csrc/scene.hip; ``DepthInferencer.scene_points``: the prediction, the ground
prior, the LiDAR ground truth and the slope-adjusted ground plane, role of the reference's visualize_point-cloud_kitti_gt_pe_pred.py) — as
the same file with one ``comment layer <name> <count>`` line per layer; ``scene_records_to_points`` brings its tensors to the host.

The per-pixel work is two gfx950 launches (``ge_depth_points``, gedepth_amd/csrc/scene.hip): an ordered stream compaction that leaves the
kept points in row-major order as 16-byte records — the file's payload byte for byte.  Where the reference formats about 428 000 points
one by one with ``"%.4f"`` into an ASCII file under an indented (malformed) header, the file here is the standard binary form with the
same properties: ``x y z`` (float), ``red green blue alpha`` (uchar).

A DDAD map works through ``depth_to_points`` as well, with the intrinsics scaled to the map and, for colour, a frame the caller has resized
to it; the DDAD inference engine itself has no uint8 frame at the map's size (``DepthInferencer.points``)."""
import os
import os.path as osp

import numpy as np
import torch

from ... import kernels

__all__ = ['POINT_DTYPE', 'depth_to_points', 'write_ply', 'kitti_intrinsics', 'write_scene_ply', 'scene_records_to_points']

POINT_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('alpha', 'u1')])

_PLY_HEADER = ('ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n'
               'property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n')


def _fxfycxcy(K):
    """(fx, fy, cx, cy) of a 3x3 or 3x4 matrix (P_rect's left block is K)."""
    K = np.asarray(K, dtype=np.float64)
    if K.shape not in ((3, 3), (3, 4)):
        raise ValueError(f'K must be a 3x3 or 3x4 matrix, got shape {K.shape}')
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def records_to_points(records, count):
    """``(records, count)`` device tensors of ``depth_to_points`` -> a ``POINT_DTYPE`` array of ``count`` records (one copy; synchronises)."""
    n = int(count.item())
    return records[:n].cpu().numpy().reshape(-1).view(POINT_DTYPE)


def depth_to_points(depth, K, img=None, top=0, left=0, min_depth=1e-3, max_depth=80.0, row0=0, step=1, alpha=255):
    """The coloured points of ``depth`` ((H, W) or (1, H, W) float32; a numpy array or a CUDA tensor).

    ``K``: 3x3 or 3x4 intrinsics in MAP coordinates (for a crop of a frame: ``cx - left``, ``cy - top``).  ``img``: (Hs, Ws, 3) uint8 BGR
    frame (numpy array or CUDA tensor) whose pixel (top + r, left + c) colours map pixel (r, c); None: white points.  The pixels (r, c) with
    r = row0, row0 + step, ... and c = 0, step, ... are taken in row-major order (``row0`` is the reference's "drop the top 100 rows") and
    kept where ``min_depth <= z <= max_depth``; a kept pixel becomes x = (c - cx) / fx * z, y = (r - cy) / fy * z, z in float32 and
    red, green, blue, ``alpha``.

    A numpy ``depth`` returns a ``POINT_DTYPE`` array of exactly the kept points.  A CUDA ``depth`` returns ``(records, count)``: a
    (capacity, 16) uint8 tensor whose first ``count`` rows are the records and a (1,) int32 tensor, without synchronising
    (``records_to_points`` / ``write_ply`` take them).  A CPU tensor raises, as in ``colorize``."""
    fx, fy, cx, cy = _fxfycxcy(K)
    if torch.is_tensor(depth):
        if not depth.is_cuda:
            raise RuntimeError('depth_to_points: gedepth_amd ops run on MI355X only; got a CPU tensor (pass a numpy array or a CUDA tensor)')
        dev, host = depth.device, False
        d = depth if depth.dtype == torch.float32 else depth.float()
    else:
        dev, host = torch.device('cuda', torch.cuda.current_device()), True
        d = torch.from_numpy(np.ascontiguousarray(np.asarray(depth), dtype=np.float32)).to(dev)
    bgr = None
    if img is not None:
        if torch.is_tensor(img):
            if not img.is_cuda:
                raise RuntimeError('depth_to_points: img must be a numpy array or a CUDA tensor, got a CPU tensor')
            bgr = img if img.is_contiguous() else img.contiguous()
        else:
            a = np.asarray(img)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise TypeError(f'img must be an (Hs, Ws, 3) uint8 BGR array, got {a.shape} {a.dtype}')
            bgr = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    records, count = kernels.depth_points(d, fx, fy, cx, cy, bgr, top, left, min_depth, max_depth, row0, step, alpha)
    return records_to_points(records, count) if host else (records, count)


def write_ply(path, points):
    """Write ``points`` — a ``POINT_DTYPE`` array, or the ``(records, count)`` tensors of ``depth_to_points`` (copied to the host once) — as a
    binary little-endian PLY file: the header, then the 16-byte records as they are.  Parent directories are created.  Host only."""
    if isinstance(points, (tuple, list)) and len(points) == 2 and torch.is_tensor(points[0]):
        points = records_to_points(*points)
    points = np.asarray(points)
    if points.dtype != POINT_DTYPE:
        raise TypeError(f'write_ply takes a POINT_DTYPE array or (records, count) tensors, got dtype {points.dtype}')
    points = np.ascontiguousarray(points.reshape(-1))
    os.makedirs(osp.dirname(osp.abspath(path)), exist_ok=True)
    with open(path, 'wb') as fh:
        fh.write(_PLY_HEADER.format(n=points.size).encode('ascii'))
        fh.write(points.tobytes())


def scene_records_to_points(records, counts, names=None):
    """``(records, counts)`` device tensors of ``kernels.scene_points`` -> ``(a POINT_DTYPE array of the counts[L] records, an ordered
    {layer name: count})`` (``counts`` and the records are copied to the host once each; synchronises).  ``names``: one per layer, default
    ``layer0``, ``layer1``, ..."""
    host = [int(v) for v in counts.cpu().tolist()]
    L = len(host) - 1
    names = [f'layer{k}' for k in range(L)] if names is None else list(names)
    if len(names) != L or len(set(names)) != L:
        raise ValueError(f'{len(names)} layer names {names} for the {L} layers of counts (one name each, no name twice)')
    if sum(host[:L]) != host[L] or min(host) < 0:
        raise ValueError(f'counts {host}: the last entry must be the sum of the others')
    return records[:host[L]].cpu().numpy().reshape(-1).view(POINT_DTYPE), dict(zip(names, host[:L]))


def write_scene_ply(path, points, counts):
    """Write a scene cloud as ``write_ply`` writes a cloud — the same binary little-endian PLY file, readable by the same tools — with one
    ``comment layer <name> <count>`` line per layer between the ``format`` line and ``element vertex``: the layers' records follow one another
    in that order.  ``points``: a ``POINT_DTYPE`` array with ``counts`` an ordered ``{layer name: count}`` that sums to its size, or the
    ``(records, counts)`` tensors of ``kernels.scene_points`` (copied to the host once) with ``counts`` the layers' names (None:
    ``scene_records_to_points``' default names).  Parent directories are created.  Host only."""
    if isinstance(points, (tuple, list)) and len(points) == 2 and torch.is_tensor(points[0]):
        points, counts = scene_records_to_points(*points, counts)
    points = np.asarray(points)
    if points.dtype != POINT_DTYPE:
        raise TypeError(f'write_scene_ply takes a POINT_DTYPE array or (records, counts) tensors, got dtype {points.dtype}')
    points = np.ascontiguousarray(points.reshape(-1))
    layers = [(str(k), int(v)) for k, v in dict(counts).items()]
    if any(not k or len(k.split()) != 1 for k, _ in layers):
        raise ValueError(f'layer names must be single words, got {[k for k, _ in layers]}')
    if any(v < 0 for _, v in layers) or sum(v for _, v in layers) != points.size:
        raise ValueError(f'the layer counts {dict(layers)} do not sum to the {points.size} points')
    head, tail = _PLY_HEADER.format(n=points.size).split('element vertex', 1)
    header = head + ''.join(f'comment layer {k} {v}\n' for k, v in layers) + 'element vertex' + tail
    os.makedirs(osp.dirname(osp.abspath(path)), exist_ok=True)
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(points.tobytes())


_NO_K = ('no intrinsics for this frame: pass K= (a 3x3 or 3x4 matrix), calib=(calib_cam_to_cam.txt, calib_velo_to_cam.txt) whose P_rect_02 '
         'is read, or an image path inside the test tree input/<date>/... of one of the KITTI recording days')


def kitti_intrinsics(path=None, calib=None, K=None, prefix=None):
    """Frame-coordinate ``(fx, fy, cx, cy)`` of a KITTI frame: from ``K`` (3x3 or 3x4), else from ``P_rect_02`` of
    ``calib=(calib_cam_to_cam.txt, calib_velo_to_cam.txt)``, else from the recording day's table when ``path`` lies inside the test tree
    ``prefix`` (``<prefix>/<date>/...``).  Otherwise a ``ValueError`` that names the three sources."""
    if K is not None:
        return _fxfycxcy(K)
    if calib is not None:
        from ..datasets.gpu_pipeline import read_kitti_calibration
        return _fxfycxcy(read_kitti_calibration(*calib)[0])
    if isinstance(path, str) and prefix is not None:
        from ..datasets.kitti import _P_RECT
        rel = osp.relpath(osp.abspath(path), osp.abspath(prefix))
        if not (rel.startswith('..') or osp.isabs(rel)):
            date = rel.split(osp.sep)[0]
            if date in _P_RECT:
                return _fxfycxcy(_P_RECT[date])
    raise ValueError(_NO_K)

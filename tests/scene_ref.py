"""Host restatement for the scene-cloud tests (imported like ``cloud_ref``): the records ``ge_scene_points`` (include/gedepth_scene.h) must
write, layer by layer through ``cloud_ref.points_f32`` and concatenated — no compaction, no kernel."""
import numpy as np

import cloud_ref as R

POINT_DTYPE = R.POINT_DTYPE


class Layer:
    """One layer on the host: ``data`` an (H_l, W_l) float32 array (``kind='f32'``) or uint16 array (``kind='u16'``, z = raw / scale in
    float32), its window offset, its range and its colour ((R, G, B), or None for the frame's)."""

    def __init__(self, data, kind='f32', dmin=1e-3, dmax=80.0, colour=None, top=0, left=0, scale=1.0):
        self.data, self.kind, self.dmin, self.dmax, self.colour, self.top, self.left, self.scale = data, kind, dmin, dmax, colour, top, left, scale

    def window(self, H, W):
        """The (H, W) float32 depths the candidates read."""
        crop = np.asarray(self.data)[self.top:self.top + H, self.left:self.left + W]
        assert crop.shape == (H, W), (crop.shape, H, W)
        if self.kind == 'u16':
            assert crop.dtype == np.uint16
            return crop.astype(np.float32) / np.float32(self.scale)
        assert crop.dtype == np.float32
        return crop


def points(layers, fx, fy, cx, cy, H, W, bgr=None, top=0, left=0, row0=0, step=1, alpha=255):
    """``(records, counts)``: a ``POINT_DTYPE`` array with the kept points of layer 0, then of layer 1, ..., and the L + 1 counts (the layers',
    then their total) as ``ge_scene_points`` writes them."""
    parts = []
    for ly in layers:
        frame = bgr if ly.colour is None else None
        p = R.points_f32(ly.window(H, W), fx, fy, cx, cy, frame, top if frame is not None else 0, left if frame is not None else 0,
                         ly.dmin, ly.dmax, row0, step, alpha)
        if ly.colour is not None:
            p['red'], p['green'], p['blue'] = ly.colour
        parts.append(p)
    counts = [p.size for p in parts]
    return np.concatenate(parts), np.array(counts + [sum(counts)], np.int32)


def read_scene_ply(path):
    """(ordered {layer: count} of the header's ``comment layer`` lines, POINT_DTYPE array) of a file ``write_scene_ply`` wrote;
    ``cloud_ref.read_ply`` checks everything else (it passes over comment lines)."""
    header, pts = R.read_ply(path)
    lines = header.decode('ascii').split('\n')
    fmt, vertex = lines.index('format binary_little_endian 1.0'), next(k for k, ln in enumerate(lines) if ln.startswith('element vertex '))
    comments = lines[fmt + 1:vertex]
    assert all(ln.startswith('comment layer ') and len(ln.split()) == 4 for ln in comments), comments
    assert not any(ln.startswith('comment') for ln in lines[:fmt] + lines[vertex:]), lines
    return {ln.split()[2]: int(ln.split()[3]) for ln in comments}, pts


# ------------------------------------------------------------------------------------------------ the inputs the CPU and the GPU tests share
H, W, HS, WS, TOP, LEFT = 37, 83, 45, 97, 3, 7                    # W odd; 3071 candidates: two spans of 1024 and a partial one
INTR = (71.25, 69.5, 40.75, 17.5)                                # fx, fy, cx, cy: exact in float32
GRIDS = ((0, 1), (5, 3))                                          # the (row0, step) the small case runs with
SPECIAL_ROWS = (8, 17)                                            # rows and columns (6 k) that are candidates of both grids
_f = np.float32
# name -> (kind, array shape, window offset, dmin, dmax, colour, scale, the range of the random fill): every array larger than the map,
# odd offsets, the uint16 array of odd width; uint16 bounds are exact multiples of 1 / 256
SMALL_SPEC = {
    'prediction': ('f32', (41, 90), (3, 5), _f(1e-3), _f(80.0), None, 1.0, 160.0),
    'ground': ('f32', (45, 97), (5, 7), _f(0.5), _f(60.0), (255, 0, 0), 1.0, 120.0),
    'gt': ('u16', (40, 89), (1, 3), _f(0.5), _f(80.0), (0, 255, 0), 256.0, 40960),
    'adjusted': ('f32', (39, 85), (1, 1), _f(2.0), _f(100.0), (0, 0, 255), 1.0, 200.0),
}
NAMES = tuple(SMALL_SPEC)
FRAME = np.random.default_rng(16).integers(0, 256, (HS, WS, 3), dtype=np.uint8)


def special_values(name):
    """The values every grid of the small case must meet in layer ``name``: the bounds, their neighbours and the values a range test can
    get wrong (as the layer's array holds them: raw for uint16)."""
    kind, _, _, dmin, dmax, _, scale, _ = SMALL_SPEC[name]
    if kind == 'u16':
        lo, hi = int(dmin * scale), int(dmax * scale)
        assert _f(lo) / _f(scale) == dmin and _f(hi) / _f(scale) == dmax
        return [np.uint16(v) for v in (0, 65535, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1)]
    return [_f(np.nan), _f(np.inf), _f(-np.inf), _f(0.0), _f(-3.5), dmin, dmax, np.nextafter(dmin, _f(0)), np.nextafter(dmin, _f(1e3)),
            np.nextafter(dmax, _f(0)), np.nextafter(dmax, _f(1e3))]


def small_layers(names=NAMES, masks=None):
    """The small case's layers as ``Layer``s.  ``masks``: {name: flat bool array over the 3071 map pixels}; a masked layer holds in-range
    depths where the mask is set and out-of-range ones (beyond dmax, below dmin, NaN for f32) elsewhere instead of the random fill."""
    out = []
    for k, name in enumerate(NAMES):
        if name not in names:
            continue
        kind, shape, (top, left), dmin, dmax, colour, scale, fill = SMALL_SPEC[name]
        rng = np.random.default_rng(20 + k)
        if kind == 'u16':
            data = rng.integers(0, fill, shape).astype(np.uint16)
        else:
            data = rng.uniform(0.0, fill, shape).astype(np.float32)
        win = data[top:top + H, left:left + W]
        if masks is not None and name in masks:
            m = np.asarray(masks[name], bool).reshape(H, W)
            pick = rng.random((H, W))
            if kind == 'u16':
                lo, hi = int(dmin * scale), int(dmax * scale)
                inside = rng.integers(lo, hi + 1, (H, W))
                outside = np.where(pick < 0.5, rng.integers(hi + 1, 65536, (H, W)), rng.integers(0, lo, (H, W)))
                win[...] = np.where(m, inside, outside).astype(np.uint16)
            else:
                inside = rng.uniform(float(dmin) * 1.01, float(dmax) * 0.99, (H, W))
                outside = np.where(pick < 0.4, rng.uniform(float(dmax) * 1.01, 3.0 * float(dmax), (H, W)),
                                   np.where(pick < 0.7, rng.uniform(-1.0, float(dmin) * 0.99, (H, W)), np.nan))
                win[...] = np.where(m, inside, outside).astype(np.float32)
        else:
            for j, v in enumerate(special_values(name)):
                for r in SPECIAL_ROWS:
                    win[r, 6 * j] = v
        out.append(Layer(data, kind, dmin, dmax, colour, top, left, scale))
    return out

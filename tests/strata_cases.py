"""The inputs of the stratified-sums tests (tests/test_strata_cpu.py checks what they promise from ``strata_ref`` alone, tests/test_strata_gpu.py
runs the kernel on them): the geometries and the ``_inputs`` ground truth of tests/test_eval_device_gpu.py (empty pixels, pixels at or beyond
80 m), a ground plane that follows about half of the returns, and sixteen boundary pixels written into fixed positions of the rectangle."""
import numpy as np

from test_eval_device_gpu import LIMITS, _full, _inputs

EDGES = (20.0, 40.0, 60.0)
TOL = 0.125                                  # a power of two: tol * g is exact, so |gt - g| == tol * g can be hit exactly
G16 = np.float32(16.0)
G16_UP, G16_DOWN = np.nextafter(G16, np.float32(np.inf)), np.nextafter(G16, np.float32(0))

# (raw, ground depth, what the pixel is there for); gt = raw / 256
BOUNDARY = (
    (5120, 50.0, 'gt == edge 20'), (10240, 50.0, 'gt == edge 40'), (15360, 50.0, 'gt == edge 60'),
    (5119, 50.0, 'one raw step below edge 20'), (10239, 50.0, 'one raw step below edge 40'), (15359, 50.0, 'one raw step below edge 60'),
    (3584, G16, '|gt - g| == tol * g, gt = 14 below g = 16'), (4608, G16, '|gt - g| == tol * g, gt = 18 above g = 16'),
    (3584, G16_UP, 'gt = 14, g one ulp above 16: off'), (3584, G16_DOWN, 'gt = 14, g one ulp below 16: on'),
    (4608, G16_UP, 'gt = 18, g one ulp above 16: on'), (4608, G16_DOWN, 'gt = 18, g one ulp below 16: off'),
    (2560, 0.0, 'g == 0'), (2560, -5.0, 'g < 0'), (2560, np.nan, 'g NaN'), (2560, np.inf, 'g +inf'),
)


def boundary_positions(rect):
    """Crop coordinates of the sixteen boundary pixels: two rows of eight from the rectangle's corner, one column in."""
    return [(rect[0] + k // 8, rect[2] + 1 + k % 8) for k in range(len(BOUNDARY))]


def _ground(geom, raw, seed):
    """(H, W) f32: about half of the pixels within 5 % of the ground truth there (on the ground for tol 0.125), a tenth without a plane
    (-5), the rest anywhere in 1 .. 80 m."""
    rng = np.random.default_rng(1000 + seed)
    gt = raw.astype(np.float32) / np.float32(LIMITS[0])
    u = rng.random(raw.shape)
    g = np.where(u < 0.5, gt * rng.uniform(0.95, 1.05, raw.shape), rng.uniform(1.0, 80.0, raw.shape))
    return np.where(u > 0.9, -5.0, g).astype(np.float32)


def _case(geom, seed, rect=None, edges=EDGES, ground=True, boundary=True, empty=()):
    raw, pred = _inputs(geom, seed)
    rect = _full(geom) if rect is None else rect
    g = _ground(geom, raw, seed) if ground else None
    top, left = geom[2:4]
    if geom[:2] == (1, 1):
        g[...] = 10.0                                                   # the one pixel (raw 2560: 10 m) lies on the ground
    elif boundary:
        for (r, c), (v, gv, _) in zip(boundary_positions(rect), BOUNDARY):
            raw[top + r, left + c] = v
            pred[r, c] = np.float32(v / 256.0 * 1.1)
            if g is not None:
                g[top + r, left + c] = gv
    S = (len(edges) + 1) * (2 if ground else 1)
    return dict(geom=geom, raw=raw, pred=pred, rect=rect, edges=tuple(edges), ground=g, tol=TOL, ground_offset=0, boundary=boundary,
                empty=set(empty), populated=set(range(S)) - set(empty), S=S)


def _cases():
    big = (40, 530, 2, 9, 37, 515)
    vec = (9, 28, 1, 4, 8, 24)
    out = {
        'odd-left-scalar': _case((11, 27, 3, 3, 8, 20), 0),
        'vector-edge-beyond-max': _case(vec, 1, edges=EDGES + (90.0,), empty=(8, 9)),          # 8-byte gt, 16-byte ground; no gt >= 90 counts
        'vector-ground-odd-offset': _case(vec, 2),                                              # the plane starts one element off: scalar loads
        'one-pixel': _case((1, 1, 0, 0, 1, 1), 3, empty=(0, 2, 3, 4, 5, 6, 7)),
        'multi-block-tails': _case(big, 4),
        'garg-rect': _case(big, 11, rect=(int(0.40810811 * 37), int(0.99189189 * 37), int(0.03594771 * 515), int(0.96405229 * 515))),
        'empty-rect': _case(big, 12, rect=(5, 5, 0, 515), boundary=False, empty=range(8)),
        'bins-only': _case(vec, 5, ground=False),
        'one-stratum': _case(big, 6, edges=(), ground=False),
    }
    out['vector-ground-odd-offset']['ground_offset'] = 1
    return out


CASES = _cases()

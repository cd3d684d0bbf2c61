"""Host restatements for the point-cloud tests (imported like ``eval_ref``): the record rule of include/gedepth_cloud.h in numpy float32,
the reference's back-projection in float64, and a small parser of binary little-endian PLY files."""
import numpy as np

POINT_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('alpha', 'u1')])

HEADER = ('ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n'
          'property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n')


def capacity(H, W, row0=0, step=1):
    return len(range(row0, H, step)) * len(range(0, W, step))


def points_f32(depth, fx, fy, cx, cy, bgr=None, top=0, left=0, dmin=1e-3, dmax=80.0, row0=0, step=1, alpha=255):
    """The records ``ge_depth_points`` must write, as a ``POINT_DTYPE`` array: candidates (r, c), r = row0, row0 + step, ... and
    c = 0, step, ..., row-major; kept iff dmin <= z <= dmax in float32 (NaN fails); x = ((float)c - cx) / fx * z, y = ((float)r - cy) / fy * z
    with one float32 rounding per operation; R, G, B from the BGR frame's pixel (top + r, left + c), white without a frame."""
    f = np.float32
    depth = np.asarray(depth, dtype=f)
    if depth.ndim == 3:
        depth = depth[0]
    H, W = depth.shape
    fx, fy, cx, cy, dmin, dmax = f(fx), f(fy), f(cx), f(cy), f(dmin), f(dmax)
    rows, cols = np.arange(row0, H, step), np.arange(0, W, step)
    z = depth[np.ix_(rows, cols)]
    with np.errstate(invalid='ignore'):
        keep = (dmin <= z) & (z <= dmax)
    r = np.broadcast_to(rows[:, None], z.shape)[keep]
    c = np.broadcast_to(cols[None, :], z.shape)[keep]
    zk = z[keep]
    out = np.zeros(zk.size, POINT_DTYPE)
    out['x'] = (c.astype(f) - cx) / fx * zk                    # float32 arrays and float32 scalars: every operation rounds to float32
    out['y'] = (r.astype(f) - cy) / fy * zk
    out['z'] = zk
    assert out['x'].dtype == f
    if bgr is None:
        out['red'] = out['green'] = out['blue'] = 255
    else:
        px = np.asarray(bgr)[top + r, left + c]
        out['red'], out['green'], out['blue'] = px[:, 2], px[:, 1], px[:, 0]
    out['alpha'] = alpha
    return out


def points_f64_reference(depth, K, row0=0, step=1):
    """(x, y, z) in float64 of EVERY candidate, by the reference's formula (tools/misc/visualize_point-cloud_kitti.py:176-188):
    ``inv(K)[:3, :3] @ [u, v, 1] * depth`` with u the column and v the row of the pixel."""
    depth = np.asarray(depth, dtype=np.float64)
    H, W = depth.shape
    K4 = np.eye(4)
    K4[:3, :3] = np.asarray(K, dtype=np.float64)[:3, :3]
    inv_K = np.linalg.inv(K4)[:3, :3]                         # the reference: np.array(np.matrix(intrinsics).I)
    rows, cols = np.arange(row0, H, step), np.arange(0, W, step)
    u, v = np.meshgrid(cols, rows, indexing='xy')
    pix = np.stack([u.reshape(-1), v.reshape(-1), np.ones(u.size)], 0).astype(np.float64)
    cam = (inv_K @ pix) * depth[np.ix_(rows, cols)].reshape(-1)[None, :]
    return cam[0], cam[1], cam[2]


def read_ply(path):
    """(header bytes, POINT_DTYPE array) of a binary little-endian PLY file with exactly the seven properties of ``HEADER``."""
    with open(path, 'rb') as fh:
        blob = fh.read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    header = blob[:end]
    lines = header.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0', lines[:2]
    vertex = [ln for ln in lines if ln.startswith('element vertex ')]
    assert len(vertex) == 1, lines
    n = int(vertex[0].split()[2])
    props = [tuple(ln.split()[1:]) for ln in lines if ln.startswith('property ')]
    assert props == [('float', 'x'), ('float', 'y'), ('float', 'z'), ('uchar', 'red'), ('uchar', 'green'), ('uchar', 'blue'),
                     ('uchar', 'alpha')], props
    payload = blob[end:]
    assert len(payload) == 16 * n, (len(payload), n)
    return header, np.frombuffer(payload, dtype=POINT_DTYPE).copy()

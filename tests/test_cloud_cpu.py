"""Point clouds, the parts that need no GPU: the fourth header and its binding, argument validation of ``ge_depth_points``, the float32
record rule against the reference's float64 formula, ``write_ply``, ``kitti_intrinsics`` and the refusals."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import cloud_ref as R
from gedepth_amd import hip
from toy_kitti import make_toy_kitti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
BAD_ARG, UNSUPPORTED = 10001, 10002
P_RECT_26 = [[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01], [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01], [0.0, 0.0, 1.0, 2.745884e-03]]


def _declared(name):
    header = open(os.path.join(ROOT, 'include', name)).read()
    return set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))


def test_cloud_header_parses_and_library_exports_it():
    declared = _declared('gedepth_cloud.h')
    assert declared == set(hip.CLOUD_SIGNATURES) == {'ge_depth_points', 'ge_depth_points_workspace'}
    for other in (hip.SIGNATURES, hip.EVAL_SIGNATURES, hip.DDAD_SIGNATURES):
        assert not set(hip.CLOUD_SIGNATURES) & set(other)
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.CLOUD_SIGNATURES['ge_depth_points'] == (i, [vp, i, i, vp, i, i, i, i] + [f] * 6 + [i] * 3 + [vp] * 4)
    assert hip.CLOUD_SIGNATURES['ge_depth_points_workspace'] == (c.c_size_t, [i] * 4)
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    for name, (res, args) in hip.CLOUD_SIGNATURES.items():            # lib() has bound the fourth table too
        fn = getattr(hip.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_training_header_is_unchanged_by_the_cloud_entry_points():
    assert _declared('gedepth_hip.h') == set(hip.SIGNATURES) and len(hip.SIGNATURES) == 102
    assert hip.lib().ge_abi_version() == 7
    assert set(hip.EVAL_SIGNATURES) == {'ge_depth_metrics', 'ge_depth_metrics_workspace'}
    assert set(hip.DDAD_SIGNATURES) == {'ge_infer_front_ddad', 'ge_depth_metrics_resized', 'ge_depth_metrics_resized_workspace'}


def test_argument_validation_without_a_gpu():
    """Every check comes before a launch, so fake non-null pointers are never followed."""
    lib = hip.lib()
    p = 4096                                                          # any 16-byte aligned non-null address

    def run(depth=p, H=37, W=83, bgr=p, Hs=45, Ws=97, top=3, left=7, fx=700.0, fy=700.0, cx=40.0, cy=20.0, dmin=1e-3, dmax=80.0, row0=0,
            step=1, alpha=255, records=p, count=p, workspace=p):
        return lib.ge_depth_points(depth, H, W, bgr, Hs, Ws, top, left, fx, fy, cx, cy, dmin, dmax, row0, step, alpha, records, count,
                                   workspace, None)
    for null in ('depth', 'records', 'count', 'workspace'):
        assert run(**{null: None}) == BAD_ARG, null
    for size in ('H', 'W', 'Hs', 'Ws'):
        assert run(**{size: 0}) == BAD_ARG and run(**{size: -4}) == BAD_ARG, size
    assert run(row0=-1) == BAD_ARG and run(row0=37) == BAD_ARG and run(row0=2 ** 31 - 1) == BAD_ARG
    assert run(step=0) == BAD_ARG and run(step=-3) == BAD_ARG
    assert run(alpha=-1) == BAD_ARG and run(alpha=256) == BAD_ARG
    assert run(fx=0.0) == BAD_ARG and run(fy=0.0) == BAD_ARG and run(fx=-0.0) == BAD_ARG
    assert run(dmin=80.5) == BAD_ARG
    assert run(top=9) == BAD_ARG and run(left=15) == BAD_ARG          # 9 + 37 > 45, 15 + 83 > 97: the window leaves the frame
    assert run(top=-1) == BAD_ARG and run(left=-1) == BAD_ARG
    assert run(Hs=2 ** 31 - 1, top=2 ** 31 - 8) == BAD_ARG            # no overflow in top + H
    assert run(Ws=2 ** 31 - 1, left=2 ** 31 - 8) == BAD_ARG
    for k in (4, 8, 12):
        assert run(records=p + k) == UNSUPPORTED, k                   # records: 16-byte aligned
    for k in (1, 2, 3):
        assert run(depth=p + k) == UNSUPPORTED, k                     # depth: 4-byte aligned
    assert run(H=65536, W=32768, bgr=None) == UNSUPPORTED             # H * W = 2^31
    assert run(H=65536, W=32768, bgr=None, row0=65535, step=7) == UNSUPPORTED
    assert run(records=p + 4, alpha=256) == BAD_ARG                   # argument errors are found first


def test_workspace_query():
    ws = hip.lib().ge_depth_points_workspace
    for bad in ((0, 5, 0, 1), (5, -1, 0, 1), (5, 5, 5, 1), (5, 5, -1, 1), (5, 5, 0, 0), (65536, 32768, 0, 1)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, 0, 1) == 4
    sizes = [ws(h, 1216, 0, 1) for h in (1, 8, 64, 352)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4 and all(s % 4 == 0 for s in sizes)        # grows with the candidate count
    assert ws(352, 1216, 0, 1) > ws(352, 1216, 100, 1) > ws(352, 1216, 100, 2) > ws(352, 1216, 100, 3) > 0
    assert ws(352, 1216, 0, 1) > 256 * 4                               # more entries than a folding block has threads
    assert ws(46340, 46340, 0, 1) >= ws(352, 1216, 0, 1)               # the grid is capped by growing the span: still one int per block


def test_float32_rule_vs_the_reference_formula_in_float64():
    """x and y of include/gedepth_cloud.h against ``inv(K)[:3, :3] @ [u, v, 1] * depth`` in float64, on float32-rounded KITTI intrinsics at
    352 x 1216 (crop-shifted as the engine shifts them), z in [1e-3, 80].  Sub, div and mul round once each, so the relative error is at
    most (1 + 2^-24)^3 - 1 = 1.8e-7 < 2^-22; an exact zero (c == cx) stays zero."""
    rng = np.random.default_rng(0)
    H, W = 352, 1216
    depth = np.exp(rng.uniform(np.log(1e-3), np.log(80.0), (H, W))).astype(np.float32)
    depth[0, 0], depth[-1, -1] = np.float32(1e-3), np.float32(80.0)
    worst = 0.0
    for cx_shift, cy_shift in ((13, 23), (0.0, 0.0)):
        fx, fy = np.float32(P_RECT_26[0][0]), np.float32(P_RECT_26[1][1])
        cx, cy = np.float32(P_RECT_26[0][2] - cx_shift), np.float32(P_RECT_26[1][2] - cy_shift)
        if cx_shift == 0.0:
            cx, cy = np.float32(600.0), np.float32(170.0)              # integral: column 600 and row 170 give exact zeros
        got = R.points_f32(depth, fx, fy, cx, cy)
        assert got.size == H * W                                       # every pixel is in range
        K = [[float(fx), 0.0, float(cx)], [0.0, float(fy), float(cy)], [0.0, 0.0, 1.0]]
        x64, y64, z64 = R.points_f64_reference(depth, K)
        assert np.array_equal(got['z'].astype(np.float64), z64)
        for name, ref in (('x', x64), ('y', y64)):
            g = got[name].astype(np.float64)
            zero = ref == 0
            assert np.array_equal(g[zero], ref[zero]), name
            assert (~zero).sum() > 0.99 * ref.size
            rel = np.abs(g[~zero] - ref[~zero]) / np.abs(ref[~zero])
            worst = max(worst, float(rel.max()))
            print(f'[{name} cx={float(cx)} cy={float(cy)}] largest relative error {rel.max():.3e}, exact zeros {int(zero.sum())}')
            assert rel.max() <= 2.0 ** -22, (name, rel.max())
            if cx_shift == 0.0:
                assert zero.sum() == (H if name == 'x' else W)
    assert worst > 0


def test_reference_restatement_keeps_order_and_predicate():
    """``points_f32`` itself: row-major order, the closed interval, NaN / inf dropped, the colour swap, row0 / step."""
    depth = np.array([[1.0, np.nan, 80.0, 80.00001], [np.inf, 1e-3, 0.0, -1.0], [5.0, 6.0, -np.inf, 7.0]], np.float32)
    bgr = np.arange(5 * 6 * 3, dtype=np.uint8).reshape(5, 6, 3)
    got = R.points_f32(depth, 2.0, 4.0, 1.0, 1.0, bgr, top=1, left=2, alpha=9)
    assert got['z'].tolist() == [1.0, 80.0, np.float32(1e-3), 5.0, 6.0, 7.0]
    assert got['x'].tolist() == [-0.5, 40.0, 0.0, -2.5, 0.0, 7.0] and got['y'][:3].tolist() == [-0.25, -20.0, 0.0]
    assert (got['blue'][0], got['green'][0], got['red'][0], got['alpha'][0]) == tuple(bgr[1, 2]) + (9,)
    assert tuple(bgr[3, 5]) == (got['blue'][-1], got['green'][-1], got['red'][-1])
    sub = R.points_f32(depth, 2.0, 4.0, 1.0, 1.0, row0=1, step=2)
    assert sub['z'].tolist() == [] and R.capacity(3, 4, 1, 2) == 2
    assert R.points_f32(depth, 2.0, 4.0, 1.0, 1.0, row0=0, step=2)['z'].tolist() == [1.0, 80.0, 5.0]
    assert (R.points_f32(depth, 2.0, 4.0, 1.0, 1.0)['red'] == 255).all()


def _points(n, seed=0):
    rng = np.random.default_rng(seed)
    pts = np.zeros(n, R.POINT_DTYPE)
    for k in 'xyz':
        pts[k] = rng.normal(0, 30, n).astype(np.float32)
    for j, k in enumerate(('red', 'green', 'blue', 'alpha')):
        pts[k] = (np.arange(n) * (2 * j + 1) + 17 * j) % 256           # odd strides: every byte value in every colour field
    return pts


@pytest.mark.parametrize('n', [0, 1, 1000])
def test_write_ply_round_trip(tmp_path, n):
    from gedepth_amd.depth.utils import POINT_DTYPE, write_ply
    assert POINT_DTYPE == R.POINT_DTYPE and POINT_DTYPE.itemsize == 16
    pts = _points(n, seed=n)
    if n == 1000:
        for k in ('red', 'green', 'blue', 'alpha'):
            assert set(pts[k].tolist()) == set(range(256)), k
    path = tmp_path / 'a' / 'b' / f'cloud{n}.ply'                      # parent directories are created
    write_ply(str(path), pts)
    header, back = R.read_ply(path)
    assert header == R.HEADER.format(n=n).encode('ascii')
    assert os.path.getsize(path) == len(header) + 16 * n
    assert back.dtype == R.POINT_DTYPE and back.tobytes() == pts.tobytes()
    assert open(path, 'rb').read()[len(header):] == pts.tobytes()
    with pytest.raises(TypeError, match='POINT_DTYPE'):
        write_ply(str(tmp_path / 'x.ply'), np.zeros((n, 4), np.float32))


def _calib_files(tmp_path, P):
    cam = ['line: 0'] * 34
    cam[8] = 'R_rect_00: ' + ' '.join(f'{v:.6e}' for v in np.eye(3).reshape(-1))
    cam[25] = 'P_rect_02: ' + ' '.join(f'{v:.6e}' for v in np.asarray(P).reshape(-1))
    velo = ['calib_time: x', 'R: ' + ' '.join(f'{v:.6e}' for v in np.eye(3).reshape(-1)), 'T: 0.0 0.0 0.0']
    paths = tmp_path / 'calib_cam_to_cam.txt', tmp_path / 'calib_velo_to_cam.txt'
    paths[0].write_text('\n'.join(cam) + '\n')
    paths[1].write_text('\n'.join(velo) + '\n')
    return str(paths[0]), str(paths[1])


def test_kitti_intrinsics_sources(tmp_path):
    from gedepth_amd.depth.utils import kitti_intrinsics
    root = str(tmp_path / 'kitti')
    make_toy_kitti(root, frames=1)
    prefix = os.path.join(root, 'input')
    img = os.path.join(prefix, '2011_09_26', '2011_09_26_drive_0001_sync', 'image_02', 'data', '0000000005.png')
    table = (P_RECT_26[0][0], P_RECT_26[1][1], P_RECT_26[0][2], P_RECT_26[1][2])
    assert kitti_intrinsics(img, prefix=prefix) == table                              # the recording day's table
    other = [[700.0, 0.0, 601.5, 1.0], [0.0, 701.0, 180.25, 2.0], [0.0, 0.0, 1.0, 3.0]]
    calib = _calib_files(tmp_path, other)
    assert kitti_intrinsics(img, calib=calib, prefix=prefix) == (700.0, 701.0, 601.5, 180.25)      # P_rect_02 comes before the table
    K = np.array([[500.0, 0.0, 320.0], [0.0, 510.0, 240.0], [0.0, 0.0, 1.0]])
    assert kitti_intrinsics(img, calib=calib, K=K, prefix=prefix) == (500.0, 510.0, 320.0, 240.0)  # an explicit K comes first
    assert kitti_intrinsics(K=np.array(other)) == (700.0, 701.0, 601.5, 180.25)                    # 3x4
    for kw in (dict(), dict(path=img), dict(path=str(tmp_path / 'frame.png'), prefix=prefix),
               dict(path=os.path.join(prefix, '2012_01_01', 'x.png'), prefix=prefix)):
        with pytest.raises(ValueError, match=r'K=.*calib=.*test tree'):
            kitti_intrinsics(**kw)
    with pytest.raises(ValueError, match='3x3 or 3x4'):
        kitti_intrinsics(K=np.eye(4))


def test_ddad_is_not_implemented_and_says_why():
    from gedepth_amd.depth.apis import inference_point_cloud
    from gedepth_amd.depth.apis.inference import DepthInferencer
    from gedepth_amd.mmrt.config import Config
    model = types.SimpleNamespace(cfg=Config.fromfile(os.path.join(CFG, 'depthformer_v_ddad.py')))
    with pytest.raises(NotImplementedError, match=r'DDADResize.*depth_to_points'):
        inference_point_cloud(model, np.zeros((1216, 1936, 3), np.uint8), K=np.eye(3))
    eng = DepthInferencer.__new__(DepthInferencer)
    eng.ddad = True
    with pytest.raises(NotImplementedError, match=r'DDADResize.*depth_to_points'):
        eng.points(np.zeros((1216, 1936, 3), np.uint8), K=np.eye(3))


def test_cpu_inputs_and_missing_sources_raise_before_device_work():
    import torch
    from gedepth_amd import kernels
    from gedepth_amd.depth.apis import inference_point_cloud
    from gedepth_amd.depth.utils import depth_to_points
    from gedepth_amd.mmrt.config import Config
    with pytest.raises(RuntimeError, match='MI355X only'):
        depth_to_points(torch.zeros(8, 20), np.eye(3))
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.depth_points(torch.zeros(8, 20), 1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match='3x3 or 3x4'):
        depth_to_points(np.zeros((8, 20), np.float32), np.eye(2))
    model = types.SimpleNamespace(cfg=Config.fromfile(os.path.join(CFG, 'depthformer_swint_v.py')))
    frame = np.zeros((375, 1242, 3), np.uint8)
    with pytest.raises(ValueError, match='pe_165.npy'):                                   # no ground depth
        inference_point_cloud(model, frame, K=np.eye(3))
    with pytest.raises(ValueError, match=r'K=.*calib=.*test tree'):                       # ground depth given, no intrinsics
        inference_point_cloud(model, frame, pe=np.zeros((375, 1242), np.float32))
    with pytest.raises(ValueError, match='one path per frame'):
        inference_point_cloud(model, [frame, frame], K=np.eye(3), out_file='one.ply')


def test_cli_ply_dir_flag(monkeypatch):
    import importlib.util
    monkeypatch.setenv('LOCAL_RANK', '0')
    spec = importlib.util.spec_from_file_location('ge_tools_test_ply', os.path.join(ROOT, 'tools', 'test.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args(['cfg.py', '--ply-dir', 'clouds', '--show-dir', 'pictures'])
    assert args.ply_dir == 'clouds' and args.show_dir == 'pictures' and tool.parse_args(['cfg.py']).ply_dir is None
    with pytest.raises(ValueError, match='--device-eval') as with_ply:
        tool.parse_args(['cfg.py', '--device-eval', '--eval', 'x', '--synthetic', '0', '--ply-dir', 'd'])
    with pytest.raises(ValueError, match='--device-eval') as with_show:
        tool.parse_args(['cfg.py', '--device-eval', '--eval', 'x', '--synthetic', '0', '--show-dir', 'd'])
    assert str(with_ply.value) == str(with_show.value)                                    # the same error

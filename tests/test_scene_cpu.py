"""The scene clouds, the parts that need no GPU: the third table of headers and its binding, the ``GeSceneLayer`` mirror, argument validation
of ``ge_scene_points`` (every check comes before a launch), the wrapper's and the engine route's argument errors on a CPU model,
``write_scene_ply``, ``tools/test.py --scene-dir``, and what the GPU tests' small case relies on, from the restatement alone."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import cloud_ref as R
import scene_ref as S
from gedepth_amd import hip
from gedepth_amd import scene_kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
BAD_ARG, UNSUPPORTED = 10001, 10002
P = 4096                                                             # a fake non-null, 16-byte aligned pointer that is never followed


def _vp(a):
    return ctypes.cast(a, ctypes.c_void_p)


def test_third_header_is_parsed_and_bound():
    assert hip.SCENE_HEADERS == {'SCENE_SIGNATURES': 'gedepth_scene.h'}
    tables = {**hip.HEADERS, **hip.EXTRA_HEADERS, **hip.SCENE_HEADERS}
    assert len(tables) == len(hip.HEADERS) + len(hip.EXTRA_HEADERS) + 1
    header = open(os.path.join(ROOT, 'include', 'gedepth_scene.h')).read()
    declared = set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))
    assert declared == set(hip.SCENE_SIGNATURES) == {'ge_scene_points', 'ge_scene_points_workspace', 'ge_scene_layer_size'}
    names = [set(getattr(hip, t)) for t in tables]
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            assert not names[a] & names[b], (list(tables)[a], list(tables)[b])
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.SCENE_SIGNATURES['ge_scene_points'] == (i, [vp, i, i, i, vp, i, i, i, i, f, f, f, f, i, i, i, vp, vp, vp, vp])
    assert hip.SCENE_SIGNATURES['ge_scene_points_workspace'] == (c.c_size_t, [i, i, i, i, i])
    assert hip.SCENE_SIGNATURES['ge_scene_layer_size'] == (c.c_size_t, [])
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    for name, (res, args) in hip.SCENE_SIGNATURES.items():
        fn = getattr(hip.lib(), name)                                  # lib() has bound the third table too
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_layer_struct_mirror_and_kernels_reexport():
    from gedepth_amd import kernels
    lib = hip.lib()
    assert ctypes.sizeof(K.GeSceneLayer) == lib.ge_scene_layer_size() == 48           # 4 of them: the 192-byte by-value table
    assert [n for n, _ in K.GeSceneLayer._fields_] == ['data', 'kind', 'H', 'W', 'top', 'left', 'scale', 'dmin', 'dmax', 'from_frame', 'red',
                                                        'green', 'blue', 'reserved']
    t = K._table([(P, 0, 37, 83, 0, 0, 1.0, 1e-3, 80.0, None), (P + 2, 1, 40, 89, 1, 3, 256.0, 0.5, 80.0, (0, 255, 7))])
    assert (t[0].data, t[0].kind, t[0].from_frame, t[0].red, t[0].green, t[0].blue) == (P, 0, 1, 0, 0, 0)
    assert (t[1].data, t[1].kind, t[1].H, t[1].W, t[1].top, t[1].left, t[1].scale, t[1].dmin, t[1].dmax, t[1].from_frame, t[1].red, t[1].green,
            t[1].blue) == (P + 2, 1, 40, 89, 1, 3, 256.0, 0.5, 80.0, 0, 0, 255, 7)
    assert kernels.scene_points is K.scene_points and kernels.SceneLayer is K.SceneLayer and K.SCENE_MAX_LAYERS == 4
    # the workspace: one int per (layer, span of ge_depth_points); 0 for refused arguments
    one = lib.ge_depth_points_workspace(352, 1216, 0, 1)
    assert [lib.ge_scene_points_workspace(352, 1216, 0, 1, L) for L in (0, 1, 2, 4, 5, -1)] == [0, one, 2 * one, 4 * one, 0, 0]
    assert lib.ge_scene_points_workspace(1024, 1100, 0, 1, 2) == 2 * 4 * 880          # the span has grown: 880 blocks per layer
    assert lib.ge_scene_points_workspace(37, 83, 0, 1, 4) == 4 * 3 * 4 and lib.ge_scene_points_workspace(37, 83, 5, 3, 4) == 4 * 1 * 4
    for bad in ((0, 83, 0, 1), (37, 0, 0, 1), (37, 83, -1, 1), (37, 83, 37, 1), (37, 83, 0, 0), (46341, 46341, 0, 1)):
        assert lib.ge_scene_points_workspace(*bad, 2) == 0, bad
    assert lib.ge_scene_points_workspace(32768, 32768, 0, 1, 1) > 0 and lib.ge_scene_points_workspace(32768, 32768, 0, 1, 2) == 0     # the total is an int


def _layers(n=2, **kw):
    row = dict(data=P, kind=0, H=11, W=30, top=3, left=3, scale=1.0, dmin=1e-3, dmax=80.0, colour=None)
    row.update(kw)
    return K._table([tuple(row.values())] * n)


def test_scene_points_argument_validation_without_a_gpu():
    lib = hip.lib()

    def run(layers='default', L=2, H=8, W=24, bgr=None, Hs=0, Ws=0, top=0, left=0, fx=2.0, fy=2.0, row0=0, step=1, alpha=255, records=P,
            counts=P, ws=P):
        layers = _vp(_layers(max(L, 1) if 1 <= L <= 4 else 4)) if layers == 'default' else layers
        return lib.ge_scene_points(layers, L, H, W, bgr, Hs, Ws, top, left, fx, fy, 1.0, 1.0, row0, step, alpha, records, counts, ws, None)
    assert run(layers=None) == BAD_ARG and run(records=None) == BAD_ARG and run(counts=None) == BAD_ARG and run(ws=None) == BAD_ARG
    assert run(layers=_vp(_layers(data=None))) == BAD_ARG
    for L in (0, -1, 5):
        assert run(L=L) == BAD_ARG, L
    assert run(H=0) == BAD_ARG and run(W=-4) == BAD_ARG
    assert run(layers=_vp(_layers(H=0))) == BAD_ARG and run(layers=_vp(_layers(W=-1))) == BAD_ARG
    assert run(row0=-1) == BAD_ARG and run(row0=8) == BAD_ARG and run(step=0) == BAD_ARG
    assert run(alpha=-1) == BAD_ARG and run(alpha=256) == BAD_ARG
    assert run(fx=0.0) == BAD_ARG and run(fy=0.0) == BAD_ARG
    assert run(layers=_vp(_layers(dmin=2.0, dmax=1.0))) == BAD_ARG
    assert run(layers=_vp(_layers(kind=2))) == BAD_ARG and run(layers=_vp(_layers(kind=-1))) == BAD_ARG
    assert run(layers=_vp(_layers(kind=1, scale=0.0))) == BAD_ARG
    assert run(layers=_vp(_layers(top=4))) == BAD_ARG                  # 4 + 8 > 11: the window leaves its array
    assert run(layers=_vp(_layers(left=7))) == BAD_ARG                 # 7 + 24 > 30
    assert run(layers=_vp(_layers(top=-1))) == BAD_ARG and run(layers=_vp(_layers(left=-1))) == BAD_ARG
    assert run(bgr=P, Hs=8, Ws=24, top=1) == BAD_ARG and run(bgr=P, Hs=9, Ws=24, left=1) == BAD_ARG and run(bgr=P, Hs=0, Ws=24) == BAD_ARG
    assert run(bgr=P, Hs=9, Ws=25, top=-1) == BAD_ARG
    # the second layer alone is wrong
    good, bad = (P, 0, 11, 30, 3, 3, 1.0, 1e-3, 80.0, None), (P, 0, 9, 27, 2, 3, 1.0, 1e-3, 80.0, None)
    assert run(layers=_vp(K._table([good, bad]))) == BAD_ARG
    assert run(records=P + 8) == UNSUPPORTED
    assert run(layers=_vp(_layers(data=P + 2))) == UNSUPPORTED and run(layers=_vp(_layers(data=P + 1, kind=1))) == UNSUPPORTED
    assert run(layers=_vp(K._table([good, (P + 2, 0, 11, 30, 3, 3, 1.0, 1e-3, 80.0, None)]))) == UNSUPPORTED
    big = K._table([(P, 0, 46341, 46341, 0, 0, 1.0, 1e-3, 80.0, None)])
    assert run(layers=_vp(big), L=1, H=46341, W=46341) == UNSUPPORTED  # H * W beyond int


def test_wrapper_argument_errors_come_before_the_library():
    L = K.SceneLayer
    f32, u16 = torch.zeros(11, 30), torch.zeros(11, 30, dtype=torch.uint16)
    with pytest.raises(ValueError, match='1 .. 4 layers, got 0'):
        K.scene_points([], 1, 1, 0, 0, 8, 24)
    with pytest.raises(ValueError, match='1 .. 4 layers, got 5'):
        K.scene_points([L(f32)] * 5, 1, 1, 0, 0, 8, 24)
    with pytest.raises(TypeError, match='a u16 layer takes a torch.uint16 tensor'):
        K.scene_points([L(f32, 'u16')], 1, 1, 0, 0, 8, 24)
    with pytest.raises(TypeError, match='a f32 layer takes a torch.float32 tensor'):
        K.scene_points([L(f32), L(u16)], 1, 1, 0, 0, 8, 24)
    with pytest.raises(ValueError, match='kind must be'):
        K.scene_points([L(f32, 'f16')], 1, 1, 0, 0, 8, 24)
    with pytest.raises(ValueError, match=r'layer 1: the \(8, 24\) window at \(4, 0\) leaves the \(11, 30\) array'):
        K.scene_points([L(f32), L(u16, 'u16', top=4)], 1, 1, 0, 0, 8, 24)
    with pytest.raises(ValueError, match='colour must be'):
        K.scene_points([L(f32, colour=(1, 2, 256))], 1, 1, 0, 0, 8, 24)
    with pytest.raises(RuntimeError, match='layer 0 and layer 1 sit on'):
        K.scene_points([L(f32), L(torch.zeros(11, 30, device='meta'))], 1, 1, 0, 0, 8, 24)
    with pytest.raises(RuntimeError, match='MI355X only'):             # CPU tensors are not run
        K.scene_points([L(f32)], 1, 1, 0, 0, 8, 24)


def _cpu_model(cfg_name):
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    cfg = Config.fromfile(os.path.join(CFG, cfg_name))
    cfg.model.pretrained = None
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.cfg = cfg
    return model.eval()


def test_scene_cloud_argument_errors_before_device_work(tmp_path):
    """A CPU model: any device work would raise something else (``torch.cuda.Stream``), so each error below comes before it."""
    from PIL import Image
    from gedepth_amd.depth.apis import inference_scene_cloud
    from gedepth_amd.depth.apis.batch_inference import BatchDepthInferencer
    from gedepth_amd.depth.apis.inference import SCENE_LAYERS, DepthInferencer, _scene_layer_names
    assert SCENE_LAYERS == ('prediction', 'ground', 'gt', 'adjusted')
    assert _scene_layer_names(None, None) == ['prediction', 'ground', 'adjusted'] and _scene_layer_names(None, 'x') == list(SCENE_LAYERS)
    assert _scene_layer_names(('adjusted', 'gt', 'prediction'), 'x') == ['prediction', 'gt', 'adjusted']      # the reference's order
    model = _cpu_model('depthformer_swint_v.py')
    frame = np.zeros((375, 1242, 3), np.uint8)
    pe = np.zeros((375, 1242), np.float32)
    gt = np.zeros((375, 1242), np.uint16)
    Kmat = np.array([[721.5, 0, 609.5], [0, 721.5, 172.8], [0, 0, 1]])
    with pytest.raises(ValueError, match="unknown scene layer.*'lidar'"):
        inference_scene_cloud(model, frame, gt, layers=('prediction', 'lidar'), pe=pe, K=Kmat)
    with pytest.raises(ValueError, match="'gt' layer needs gt="):
        inference_scene_cloud(model, frame, None, layers=('prediction', 'gt'), pe=pe, K=Kmat)
    with pytest.raises(ValueError, match=r'gt has shape \(370, 1224\), the frame is \(375, 1242\)'):
        inference_scene_cloud(model, frame, np.zeros((370, 1224), np.uint16), pe=pe, K=Kmat)
    with pytest.raises(TypeError, match='16-bit single-channel PNG or an .* uint16 array, got float32'):
        inference_scene_cloud(model, frame, gt.astype(np.float32), pe=pe, K=Kmat)
    png = str(tmp_path / 'gt8.png')
    Image.fromarray(np.zeros((375, 1242), np.uint8)).save(png)
    with pytest.raises(TypeError, match='got mode L'):
        inference_scene_cloud(model, frame, png, pe=pe, K=Kmat)
    with pytest.raises(ValueError, match='no intrinsics'):
        inference_scene_cloud(model, frame, gt, pe=pe)
    with pytest.raises(ValueError, match='no ground depth'):
        inference_scene_cloud(model, frame, gt, K=Kmat)
    with pytest.raises(ValueError, match='smaller than the KB crop'):
        inference_scene_cloud(model, np.zeros((300, 1242, 3), np.uint8), None, pe=np.zeros((300, 1242), np.float32), K=Kmat)
    with pytest.raises(ValueError, match='1 ground truths for 2 frames'):
        inference_scene_cloud(model, [frame, frame], [gt], pe=pe, K=Kmat)
    ddad = _cpu_model('depthformer_v_ddad.py')
    with pytest.raises(NotImplementedError, match='point clouds on a DDAD engine'):
        inference_scene_cloud(ddad, frame, gt, pe=pe, K=Kmat)
    # the engines' own refusals need no device either: a DDAD engine, as ``points``; the batched engine, as for ``points``
    eng = object.__new__(DepthInferencer)
    eng.ddad = True
    with pytest.raises(NotImplementedError) as scene:
        eng.scene_points(frame, gt)
    with pytest.raises(NotImplementedError) as cloud:
        eng.points(frame)
    assert str(scene.value) == str(cloud.value)
    with pytest.raises(NotImplementedError, match=r'runs batch\(imgs\)'):
        object.__new__(BatchDepthInferencer).scene_points(frame, gt)
    assert BatchDepthInferencer.scene_points is BatchDepthInferencer.points


def test_write_scene_ply_round_trip(tmp_path):
    from gedepth_amd.depth.utils import POINT_DTYPE, scene_records_to_points, write_ply, write_scene_ply
    pts, counts = S.points(S.small_layers(), *S.INTR, S.H, S.W, S.FRAME, S.TOP, S.LEFT)
    assert POINT_DTYPE == S.POINT_DTYPE and pts.size == counts[-1] > 0
    named = dict(zip(S.NAMES, (int(c) for c in counts[:-1])))
    out = tmp_path / 'a' / 'b' / 'scene.ply'
    write_scene_ply(str(out), pts, named)
    layers, back = S.read_scene_ply(out)
    assert layers == named and list(layers) == list(S.NAMES) and back.tobytes() == pts.tobytes()
    # the same file as write_ply's but for the comment lines, which sit between the format line and element vertex
    write_ply(str(tmp_path / 'plain.ply'), pts)
    blob, plain = out.read_bytes(), (tmp_path / 'plain.ply').read_bytes()
    comments = ''.join(f'comment layer {k} {v}\n' for k, v in named.items()).encode('ascii')
    head = b'ply\nformat binary_little_endian 1.0\n'
    assert plain.startswith(head) and blob == head + comments + plain[len(head):]
    # tensors: the names in ``counts``' place; CPU tensors serve (the function is host only)
    records = torch.from_numpy(np.concatenate([pts, np.zeros(5, POINT_DTYPE)]).view(np.uint8).reshape(-1, 16))
    arr, got = scene_records_to_points(records, torch.from_numpy(counts), S.NAMES)
    assert arr.tobytes() == pts.tobytes() and got == named and list(got) == list(S.NAMES)
    assert list(scene_records_to_points(records, torch.from_numpy(counts))[1]) == ['layer0', 'layer1', 'layer2', 'layer3']
    write_scene_ply(str(tmp_path / 't.ply'), (records, torch.from_numpy(counts)), S.NAMES)
    assert (tmp_path / 't.ply').read_bytes() == blob
    empty = {k: 0 for k in S.NAMES}
    write_scene_ply(str(tmp_path / 'e.ply'), pts[:0], empty)
    assert S.read_scene_ply(tmp_path / 'e.ply')[0] == empty and R.read_ply(tmp_path / 'e.ply')[1].size == 0
    with pytest.raises(ValueError, match='do not sum'):
        write_scene_ply(str(tmp_path / 'x.ply'), pts, dict(named, gt=named['gt'] + 1))
    with pytest.raises(ValueError, match='single words'):
        write_scene_ply(str(tmp_path / 'x.ply'), pts, {'two words': pts.size})
    with pytest.raises(TypeError, match='POINT_DTYPE'):
        write_scene_ply(str(tmp_path / 'x.ply'), np.zeros(3, np.float32), {'a': 3})
    with pytest.raises(ValueError, match='layer names'):
        scene_records_to_points(records, torch.from_numpy(counts), ('a', 'b'))
    with pytest.raises(ValueError, match='sum of the others'):
        scene_records_to_points(records, torch.tensor([1, 2, 4], dtype=torch.int32))
    assert not (tmp_path / 'x.ply').exists()


def _cli(name):
    spec = importlib.util.spec_from_file_location(f'tools_{name}_cli_scene', os.path.join(ROOT, 'tools', f'{name}.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_scene_dir_and_its_exclusions():
    cli = _cli('test')
    cfg = os.path.join(CFG, 'depthformer_swint_v.py')
    args = cli.parse_args([cfg, 'model.pth', '--scene-dir', 'clouds'])
    assert args.scene_dir == 'clouds' and cli.parse_args([cfg]).scene_dir is None
    for extra in (['--eval', 'x'], ['--out', 'r.pkl'], ['--format-only'], ['--show'], ['--show-dir', 'd'], ['--ply-dir', 'd'], ['--ground-dir', 'd'],
                  ['--device-eval'], ['--device-eval', '--eval', 'x', '--synthetic', '0']):
        with pytest.raises(ValueError, match=f'--scene-dir cannot be combined with .*{extra[0]}'):
            cli.parse_args([cfg, '--scene-dir', 'clouds'] + extra)
    from gedepth_amd.depth.apis.test import multi_gpu_test, single_gpu_test
    for kw in (dict(pre_eval=True), dict(format_only=True), dict(show=True), dict(out_dir='d'), dict(ply_dir='d'), dict(ground_dir='d'),
               dict(pre_eval=True, device_eval=True)):
        with pytest.raises(NotImplementedError, match='scene_dir with'):
            single_gpu_test(torch.nn.Identity(), None, scene_dir='clouds', **kw)
    with pytest.raises(NotImplementedError, match='scene_dir with'):
        multi_gpu_test(torch.nn.Identity(), None, pre_eval=True, scene_dir='clouds')


def test_small_case_properties_on_the_host():
    """What the GPU tests' small case relies on, from the restatement alone: every layer keeps between 30 % and 70 % of its candidates for
    each (row0, step), and every special value is among each grid's candidates of each layer."""
    layers = S.small_layers()
    assert [ly.kind for ly in layers] == ['f32', 'f32', 'u16', 'f32'] and R.capacity(S.H, S.W) == 3071
    for ly, name in zip(layers, S.NAMES):
        h, w = ly.data.shape
        assert h > S.H and w > S.W and ly.top % 2 == 1 and ly.left % 2 == 1, name                    # larger than the map, odd offsets
    assert layers[2].data.shape[1] % 2 == 1                                                          # the uint16 rows start at odd elements
    for row0, step in S.GRIDS:
        cap = R.capacity(S.H, S.W, row0, step)
        pts, counts = S.points(layers, *S.INTR, S.H, S.W, S.FRAME, S.TOP, S.LEFT, row0, step)
        assert counts[-1] == counts[:-1].sum() == pts.size
        for ly, name, kept in zip(layers, S.NAMES, counts):
            assert 0.3 * cap <= kept <= 0.7 * cap, (name, row0, step, kept, cap)
            cand = np.asarray(ly.data)[ly.top:ly.top + S.H, ly.left:ly.left + S.W][row0::step, ::step].reshape(-1)
            for v in S.special_values(name):
                assert (np.isnan(cand).any() if np.isnan(v) else (cand == v).any()), (name, row0, step, v)
    pts, counts = S.points(layers, *S.INTR, S.H, S.W, S.FRAME, S.TOP, S.LEFT)
    ends = np.cumsum(counts[:-1])
    for k, (ly, name) in enumerate(zip(layers, S.NAMES)):
        z = pts['z'][ends[k] - counts[k]:ends[k]]
        assert (z == ly.dmin).any() and (z == ly.dmax).any() and np.isfinite(z).all() and z.min() >= ly.dmin and z.max() <= ly.dmax, name
        part = pts[ends[k] - counts[k]:ends[k]]
        if ly.colour is not None:
            assert (part['red'] == ly.colour[0]).all() and (part['green'] == ly.colour[1]).all() and (part['blue'] == ly.colour[2]).all()
    # a single frame-coloured f32 layer with a zero window is cloud_ref's own cloud
    depth = np.ascontiguousarray(layers[0].window(S.H, S.W))
    one, c = S.points([S.Layer(depth)], *S.INTR, S.H, S.W, S.FRAME, S.TOP, S.LEFT, 5, 3, 77)
    assert one.tobytes() == R.points_f32(depth, *S.INTR, S.FRAME, S.TOP, S.LEFT, 1e-3, 80.0, 5, 3, 77).tobytes() and list(c) == [one.size] * 2

"""Scene clouds on the MI355X: ``ge_scene_points`` (csrc/scene.hip) bit for bit against the numpy float32 restatement (tests/scene_ref.py)
under red zones and both poison bytes (tests/memguard.py), ``DepthInferencer.scene_points`` / ``inference_scene_cloud`` on the toy KITTI
tree, and tools/test.py's ``--scene-dir`` end to end.

Every kernel case runs twice under each poison byte.  Checked each time: the red zones of every layer, the frame, ``records``, ``counts``
and the workspace; every workspace word written; the rows of ``records`` from ``counts[L]`` on still poison; the two runs, and the runs
under 0xFF and 0x7F, identical; ``counts`` and the first ``counts[L]`` rows equal to the restatement's."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import cloud_ref as R
import memguard
import scene_ref as S
from toy_kitti import make_toy_kitti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, 'configs', 'depthformer', 'depthformer_swint_v.py')
pytestmark = pytest.mark.gpu


def _device_layer(guard, ly, offset):
    """``ly`` (a ``scene_ref.Layer``) as a ``kernels.SceneLayer`` on framed device memory.  ``offset``: the array starts one element into
    its frame, so an f32 array is 4-byte but not 16-byte aligned and a uint16 array 2-byte but not 4-byte aligned."""
    from gedepth_amd.kernels import SceneLayer
    data = np.ascontiguousarray(ly.data)
    if offset:
        flat = guard.framed(torch.from_numpy(np.concatenate([np.zeros(1, data.dtype), data.reshape(-1)])).cuda())
        dev = flat[1:].view(data.shape)
        assert dev.data_ptr() % 16 == data.itemsize
    else:
        dev = guard.framed(torch.from_numpy(data).cuda())
    return SceneLayer(dev, ly.kind, float(ly.dmin), float(ly.dmax), ly.colour, ly.top, ly.left, float(ly.scale))


def _run(monkeypatch, layers, h=S.H, w=S.W, bgr=None, top=0, left=0, row0=0, step=1, alpha=255, intr=S.INTR, offset=True):
    """kernels.scene_points twice under each poison byte, with the checks of the module docstring.  Returns (counts, the first counts[L]
    rows as a POINT_DTYPE array, the restatement's records, the restatement's counts)."""
    from gedepth_amd import hip, kernels, scene_kernels
    ref, ref_counts = S.points(layers, *intr, h, w, bgr, top, left, row0, step, alpha)
    L, cap = len(layers), R.capacity(h, w, row0, step)
    seen = []
    for poison in memguard.POISONS:
        guard = memguard.Guard(poison)
        guard.install(monkeypatch, [scene_kernels], binding=hip)
        dev = [_device_layer(guard, ly, offset) for ly in layers]
        d_bgr = None if bgr is None else guard.framed(torch.from_numpy(bgr).cuda())
        outs = [kernels.scene_points(dev, *intr, h, w, d_bgr, top, left, row0, step, alpha) for _ in range(2)]
        torch.cuda.synchronize()
        monkeypatch.undo()
        frames = guard.check()                                    # red zones of the layers, the frame and, per launch, records / counts / workspace
        assert guard.launched == ['ge_scene_points'] * 2 and guard.direct.count('ge_scene_points_workspace') == 2
        own = [f for f in frames if os.path.basename(f.site[0]) == 'scene_kernels.py']
        assert [tuple(f.shape) for f in own] == [(L * cap, 16), (L + 1,), (hip.lib().ge_scene_points_workspace(h, w, row0, step, L) // 4,)] * 2
        for f in own[2::3]:
            assert not bool(f.poisoned().any()), 'a workspace word was never written'
        for records, counts in outs:
            assert records.shape == (L * cap, 16) and records.dtype == torch.uint8 and counts.shape == (L + 1,) and counts.dtype == torch.int32
            c = counts.cpu().numpy()
            n = int(c[L])
            assert 0 <= n <= L * cap and c[:L].sum() == n and (c[:L] >= 0).all() and (c[:L] <= cap).all()
            rows = records.cpu().numpy()
            assert (rows[n:] == poison).all(), 'bytes of records beyond 16 * total were written'
            seen.append((c.tobytes(), rows[:n].tobytes()))
    assert all(s == seen[0] for s in seen), 'two runs, or the runs under the two poison bytes, differ'
    return np.frombuffer(seen[0][0], np.int32), np.frombuffer(seen[0][1], dtype=R.POINT_DTYPE), ref, ref_counts


def _assert_equal(counts, got, ref, ref_counts, what=''):
    assert counts.tolist() == ref_counts.tolist(), (what, counts, ref_counts)
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero(got != ref)[0]
        raise AssertionError(f'{what}: {bad.size} of {ref.size} records differ; first at {bad[0]}: {got[bad[0]]} != {ref[bad[0]]}')


@pytest.mark.parametrize('grid', S.GRIDS)
def test_small_four_layers_bit_exact_under_guards(monkeypatch, grid):
    """37 x 83, four layers, each array larger than the map with odd window offsets, the uint16 array of odd width, every array one
    element into its allocation (tests/test_scene_cpu.py checks the inputs' properties on the host)."""
    row0, step = grid
    layers = S.small_layers()
    counts, got, ref, ref_counts = _run(monkeypatch, layers, bgr=S.FRAME, top=S.TOP, left=S.LEFT, row0=row0, step=step, alpha=200 + step)
    _assert_equal(counts, got, ref, ref_counts, f'row0={row0} step={step}')
    cap = R.capacity(S.H, S.W, row0, step)
    assert all(0 < c < cap for c in counts[:4]) and (got['alpha'] == 200 + step).all()
    ends = np.cumsum(counts[:4])
    for k, ly in enumerate(layers[1:], 1):                          # the constant colours, layer by layer
        part = got[ends[k] - counts[k]:ends[k]]
        assert (part['red'] == ly.colour[0]).all() and (part['green'] == ly.colour[1]).all() and (part['blue'] == ly.colour[2]).all()


@pytest.mark.parametrize('names', [('prediction',), ('ground',), ('gt',), ('adjusted',), ('prediction', 'gt'), ('ground', 'adjusted')])
def test_subsets_of_the_layers(monkeypatch, names):
    layers = S.small_layers(names)
    assert len(layers) == len(names)
    counts, got, ref, ref_counts = _run(monkeypatch, layers, bgr=S.FRAME, top=S.TOP, left=S.LEFT)
    _assert_equal(counts, got, ref, ref_counts, '+'.join(names))
    assert counts[-1] > 0


@pytest.mark.parametrize('colour', ['bgr', 'white'])
def test_a_lone_frame_coloured_layer_is_depth_points(monkeypatch, colour):
    """A single f32 layer with the frame's colour and a zero window: the bytes and the count of ``kernels.depth_points`` on the same inputs
    (the same kernels, entered through ``ge_depth_points``, which stores no total; the numpy restatement is the independent reference)."""
    from gedepth_amd import kernels
    depth = np.ascontiguousarray(S.small_layers(('prediction',))[0].window(S.H, S.W))
    bgr = S.FRAME if colour == 'bgr' else None
    top, left = (S.TOP, S.LEFT) if bgr is not None else (0, 0)
    for row0, step in S.GRIDS:
        counts, got, ref, ref_counts = _run(monkeypatch, [S.Layer(depth)], bgr=bgr, top=top, left=left, row0=row0, step=step, alpha=99)
        _assert_equal(counts, got, ref, ref_counts, colour)
        d_bgr = None if bgr is None else torch.from_numpy(bgr).cuda()
        records, count = kernels.depth_points(torch.from_numpy(depth).cuda(), *S.INTR, d_bgr, top, left, 1e-3, 80.0, row0, step, 99)
        n = int(count.item())
        assert n == counts[0] == counts[1] > 0 and records[:n].cpu().numpy().tobytes() == got.tobytes()


IDX = np.arange(S.H * S.W)
MASKS = {
    'nothing': np.zeros(S.H * S.W, bool),
    'everything': np.ones(S.H * S.W, bool),
    'first': IDX == 0,
    'last': IDX == S.H * S.W - 1,
    'lane63': IDX % 64 == 63,
}
ARRANGEMENTS = {
    'empty-between': ('everything', 'nothing', 'lane63', 'first'),           # an empty layer between two non-empty ones
    'boundary-in-a-wave': ('lane63', 'everything', 'last', 'lane63'),        # 47 points, then a layer whose first wave starts at record 47
    'single-points': ('last', 'first', 'nothing', 'everything'),
    'all-empty': ('nothing', 'nothing', 'nothing', 'nothing'),
}


@pytest.mark.parametrize('name', list(ARRANGEMENTS))
def test_structured_layers(monkeypatch, name):
    masks = {n: MASKS[m] for n, m in zip(S.NAMES, ARRANGEMENTS[name])}
    counts, got, ref, ref_counts = _run(monkeypatch, S.small_layers(masks=masks), bgr=S.FRAME, top=S.TOP, left=S.LEFT)
    _assert_equal(counts, got, ref, ref_counts, name)
    assert counts[:4].tolist() == [int(MASKS[m].sum()) for m in ARRANGEMENTS[name]]
    if name == 'all-empty':
        assert counts.tolist() == [0] * 5 and got.size == 0        # and _run has found every byte of records still poison
    if name == 'boundary-in-a-wave':
        assert counts[0] % 64 != 0 and counts[1] == 3071


def _big_layers(h, w, seed, n):
    """``n`` layers over an (h, w) map at KITTI's scale: f32 with NaNs, uint16 over 256, arrays a little larger than the map."""
    rng = np.random.default_rng(seed)
    spec = [('f32', (0, 0), (0, 0), None, 1e-3, 80.0), ('u16', (23, 13), (23, 26), (0, 255, 0), 1e-3, 80.0),
            ('f32', (23, 13), (23, 26), (255, 0, 0), 1e-3, 80.0), ('f32', (1, 3), (2, 5), (0, 0, 255), 0.5, 60.0)][:n]
    out = []
    for kind, (top, left), (dh, dw), colour, dmin, dmax in spec:
        shape = (h + dh, w + dw)
        if kind == 'u16':
            data = np.where(rng.random(shape) < 0.5, rng.integers(0, 30000, shape), 0).astype(np.uint16)
        else:
            data = rng.uniform(0.0, 120.0, shape).astype(np.float32)
            data[rng.random(shape) < 0.01] = np.nan
        out.append(S.Layer(data, kind, np.float32(dmin), np.float32(dmax), colour, top, left, 256.0))
    return out


def _big_case(monkeypatch, h, w, seed, n):
    layers = _big_layers(h, w, seed, n)
    frame = np.random.default_rng(seed + 100).integers(0, 256, (h + 23, w + 26, 3), dtype=np.uint8)
    intr = (721.5377, 721.5377, 609.5593 - 13, 172.854 - 23)
    counts, got, ref, ref_counts = _run(monkeypatch, layers, h, w, frame, 23, 13, intr=intr, offset=False)
    assert counts.tolist() == ref_counts.tolist() and all(0.2 * h * w < c < 0.8 * h * w for c in counts[:n])
    assert got[0] == ref[0] and got[-1] == ref[-1]
    assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(ref.tobytes()).hexdigest()


def test_kitti_sized_scene(monkeypatch):
    """352 x 1216 with four layers: 4 x 418 spans, so a block folds more workspace entries than it has threads."""
    from gedepth_amd import hip
    assert hip.lib().ge_scene_points_workspace(352, 1216, 0, 1, 4) // 4 == 4 * 418 > 256
    _big_case(monkeypatch, 352, 1216, 8, 4)


def test_span_grows_past_the_grid_cap(monkeypatch):
    """1024 x 1100 with two layers: more than 1024 spans of 1024 per layer, so the span grows (5 candidates per thread, 880 blocks)."""
    from gedepth_amd import hip
    assert hip.lib().ge_scene_points_workspace(1024, 1100, 0, 1, 2) == 2 * 4 * 880
    _big_case(monkeypatch, 1024, 1100, 9, 2)


# ------------------------------------------------------------------------------------------------ the engine, on the toy tree
@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import test_inference_gpu as TI
    root = str(tmp_path_factory.mktemp('kitti_scene'))
    split = make_toy_kitti(root, seed=4, frames=1)
    model = TI._model('depthformer_swint_v.py', root, split)
    drive = '2011_09_26_drive_0001_sync'
    img = os.path.join(root, 'input', '2011_09_26', drive, 'image_02', 'data', '0000000005.png')
    gt = os.path.join(root, 'gt_depth', drive, 'proj_depth', 'groundtruth', 'image_02', '0000000005.png')
    return model, img, gt


def _engine_ref(eng, names, **kw):
    """The restatement on the buffers the last ``scene_points`` call left on the device: ``static_out``, the raw ground depth, the
    uploaded ground truth, the ``ground_depth`` plane and the uploaded frame, with the crop-shifted intrinsics of the day."""
    from gedepth_amd.depth.datasets.kitti import _P_RECT
    from gedepth_amd.ground_kernels import PLANES
    dev, top, left = eng.last_frame
    frame = dev.cpu().numpy()
    assert (top, left) == (frame.shape[0] - 352, int((frame.shape[1] - 1216) / 2))
    head, P = eng.model.decode_head, _P_RECT['2011_09_26']
    lo, hi = np.float32(kw.pop('min_depth', head.min_depth)), np.float32(kw.pop('max_depth', head.max_depth))
    made = {'prediction': lambda: S.Layer(eng.static_out[0].cpu().numpy(), 'f32', lo, hi),
            'ground': lambda: S.Layer(eng.last_ground_depth.cpu().numpy(), 'f32', lo, hi, (255, 0, 0), top, left),
            'gt': lambda: S.Layer(eng.last_gt.cpu().numpy(), 'u16', lo, hi, (0, 255, 0), top, left, 256.0),
            'adjusted': lambda: S.Layer(eng.static_ground[PLANES.index('ground_depth')].cpu().numpy(), 'f32', lo, hi, (0, 0, 255))}
    return S.points([made[n]() for n in names], P[0][0], P[1][1], P[0][2] - left, P[1][2] - top, 352, 1216, frame, top, left, **kw)


def test_engine_scene_points_bit_exact_and_no_new_capture(toy):
    from PIL import Image
    from gedepth_amd import kernels
    from gedepth_amd.depth.apis.inference import SCENE_LAYERS, DepthInferencer
    model, img, gt = toy
    eng = DepthInferencer(model)
    raw_gt = np.asarray(Image.open(gt))
    for call in range(3):                                          # two eager calls, then ground_maps' capture: each compared within its own run
        records, counts = eng.scene_points(img, gt=gt)
        assert records.is_cuda and records.shape == (4 * 352 * 1216, 16) and counts.shape == (5,) and len(eng.last_frame) == 3
        ref, ref_counts = _engine_ref(eng, SCENE_LAYERS)
        c = counts.cpu().numpy()
        assert c.tolist() == ref_counts.tolist() and all(k > 1000 for k in c), (call, c, ref_counts)
        assert records[:c[4]].cpu().numpy().tobytes() == ref.tobytes(), call
        assert eng.captures == (1 if call == 2 else 0)
        assert np.array_equal(eng.last_gt.cpu().numpy(), raw_gt) and tuple(eng.last_ground_depth.shape) == raw_gt.shape
    assert list(eng.graphs) == [eng._key(True)]                    # ground_maps' capture and key, nothing else
    assert eng.ground_maps(img, to_host=False)['depth'] is eng.static_out and eng.captures == 1 and list(eng.graphs) == [eng._key(True)]
    # without 'adjusted' the frame runs as __call__: its key, still in its warm-up, so eager and without a capture
    records, counts = eng.scene_points(img, layers=('prediction',))
    assert counts.shape == (2,) and records.shape == (352 * 1216, 16)
    n = int(counts[1])
    dev, top, left = eng.last_frame
    fx, fy, cx, cy = _intrinsics()
    head = model.decode_head
    want, count = kernels.depth_points(eng.static_out, fx, fy, cx - left, cy - top, dev, top, left, head.min_depth, head.max_depth)
    assert n == int(counts[0]) == int(count) > 1000 and torch.equal(records[:n], want[:n])
    assert eng.captures == 1 and list(eng.graphs) == [eng._key(True)] and eng.calls[eng._key()] == 1
    # the caller's order does not matter; the array form of gt; the cloud arguments
    records, counts = eng.scene_points(img, gt=raw_gt, layers=('gt', 'prediction', 'ground'), row0=100, step=4, alpha=7, max_depth=40.0)
    ref, ref_counts = _engine_ref(eng, ('prediction', 'ground', 'gt'), row0=100, step=4, alpha=7, max_depth=40.0)
    c = counts.cpu().numpy()
    assert records.shape == (3 * 63 * 304, 16) and c.tolist() == ref_counts.tolist() and records[:c[3]].cpu().numpy().tobytes() == ref.tobytes()
    assert eng.captures == 1 and eng.calls[eng._key()] == 2
    with pytest.raises(ValueError, match='gt has shape'):
        eng.scene_points(img, gt=raw_gt[:-1])
    with pytest.raises(TypeError, match='unknown argument'):
        eng.scene_points(img, gt=raw_gt, stride=2)


def _intrinsics():
    from gedepth_amd.depth.datasets.kitti import _P_RECT
    P = _P_RECT['2011_09_26']
    return P[0][0], P[1][1], P[0][2], P[1][2]


def test_inference_scene_cloud_writes_what_it_returns(toy, tmp_path):
    from gedepth_amd.depth.apis import inference_scene_cloud
    from gedepth_amd.depth.apis.inference import SCENE_LAYERS
    from gedepth_amd.depth.utils import POINT_DTYPE
    model, img, gt = toy
    out = tmp_path / 'clouds' / 'frame.ply'
    clouds = inference_scene_cloud(model, img, gt, out_file=str(out))
    assert len(clouds) == 1
    pts, counts = clouds[0]
    assert pts.dtype == POINT_DTYPE and list(counts) == list(SCENE_LAYERS) and sum(counts.values()) == pts.size > 4000
    layers, back = S.read_scene_ply(out)
    assert layers == counts and list(layers) == list(SCENE_LAYERS) and back.tobytes() == pts.tobytes()
    eng = model._ge_inferencers[False]
    ref, ref_counts = _engine_ref(eng, SCENE_LAYERS)               # the static buffers are still this call's
    assert pts.tobytes() == ref.tobytes() and list(counts.values()) == ref_counts[:4].tolist()
    two = inference_scene_cloud(model, [img, img], [gt, None], out_file=[str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')], step=8)
    assert [list(c) for _, c in two] == [list(SCENE_LAYERS), ['prediction', 'ground', 'adjusted']]
    for f, (p, c) in zip(('a.ply', 'b.ply'), two):
        layers, back = S.read_scene_ply(tmp_path / f)
        assert layers == c and back.tobytes() == p.tobytes()


# ------------------------------------------------------------------------------------------------ tools/test.py --scene-dir
def test_cli_scene_dir(tmp_path):
    import test_visualize_gpu as TV
    from gedepth_amd.depth.apis.inference import SCENE_LAYERS
    from gedepth_amd.depth.datasets import build_dataset
    from gedepth_amd.mmrt.checkpoint import save_checkpoint
    root = str(tmp_path / 'kitti')
    split = make_toy_kitti(root, frames=1)
    cfg, model = TV._vanilla_model()
    ckpt = str(tmp_path / 'model.pth')
    save_checkpoint(model, ckpt)
    cfg.data.test.data_root, cfg.data.test.split = root, split
    ds = build_dataset(cfg.data.test, dict(test_mode=True))
    names = [info['filename'] for info in ds.img_infos]
    assert len(names) == 2
    scene = tmp_path / 'scene'
    TV._run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), CONFIG, ckpt, '--scene-dir', str(scene),
             '--options', f'data.test.data_root={root}', f'data.test.split={split}', 'data.workers_per_gpu=0'])
    found = sorted(os.path.relpath(os.path.join(d, f), scene) for d, _, fs in os.walk(scene) for f in fs)
    assert found == sorted(n[:-4] + '.ply' for n in names)
    for i, n in enumerate(names):
        layers, pts = S.read_scene_ply(scene / (n[:-4] + '.ply'))
        assert list(layers) == list(SCENE_LAYERS) and sum(layers.values()) == pts.size and all(v > 1000 for v in layers.values()), (n, layers)
        ends = np.cumsum(list(layers.values()))
        gt = pts[ends[1]:ends[2]]                                  # the ground truth's points: green, and the PNG's depths in the KB window
        assert (gt['red'] == 0).all() and (gt['green'] == 255).all() and (gt['blue'] == 0).all()
        raw = ds.gt_raw(i)
        top, left = raw.shape[0] - 352, int((raw.shape[1] - 1216) / 2)
        z = raw[top:top + 352, left:left + 1216].astype(np.float32) / np.float32(256.0)
        head = model.decode_head
        assert gt['z'].tobytes() == z[(z >= np.float32(head.min_depth)) & (z <= np.float32(head.max_depth))].tobytes(), n

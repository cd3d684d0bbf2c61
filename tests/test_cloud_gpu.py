"""Point clouds on the MI355X: ``ge_depth_points`` (csrc/scene.hip: the scene cloud of one frame-coloured f32 layer, with no
total stored behind its one-int count) bit for bit against the numpy float32 restatement (tests/cloud_ref.py)
under red zones and both poison bytes (tests/memguard.py), ``DepthInferencer.points`` / ``inference_point_cloud`` on the toy KITTI tree,
and tools/test.py's ``--ply-dir`` end to end.

Every kernel case runs twice under each poison byte.  Checked each time: the red zones of the map, the frame, ``records``, ``count`` and the
workspace; every workspace word written; the rows of ``records`` from ``count`` on still poison; the two runs, and the runs under 0xFF and
0x7F, identical; ``count`` and the first ``count`` rows equal to the restatement's."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import cloud_ref as R
import memguard
from toy_kitti import make_toy_kitti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, 'configs', 'depthformer', 'depthformer_swint_v.py')
pytestmark = pytest.mark.gpu

H, W, HS, WS, TOP, LEFT = 37, 83, 45, 97, 3, 7                    # W odd; 3071 candidates: two spans of 1024 and a partial one
DMIN, DMAX = np.float32(1e-3), np.float32(80.0)
INTR = (71.25, 69.5, 40.75, 17.5)                                # fx, fy, cx, cy: exact in float32
_f = np.float32
SPECIAL = [_f(np.nan), _f(np.inf), _f(-np.inf), _f(0.0), _f(-3.5), DMIN, DMAX, np.nextafter(DMIN, _f(0)), np.nextafter(DMIN, _f(1)),
           np.nextafter(DMAX, _f(0)), np.nextafter(DMAX, _f(100))]
SPECIAL_ROWS = (6, 11, 12, 17)                                    # 6, 12: candidates of row0 = 0, steps 1 - 3; 11, 17: of row0 = 5


def _small_map():
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.0, 160.0, (H, W)).astype(np.float32)    # about half beyond 80
    for k, v in enumerate(SPECIAL):
        for r in SPECIAL_ROWS:
            depth[r, 6 * k] = v
    return depth


SMALL = _small_map()
FRAME = np.random.default_rng(6).integers(0, 256, (HS, WS, 3), dtype=np.uint8)


def _masked(mask):
    """The small map with in-range depths where ``mask`` (a flat bool array over the 3071 pixels) and out-of-range ones elsewhere."""
    rng = np.random.default_rng(7)
    inside = rng.uniform(1.0, 79.0, H * W).astype(np.float32)
    outside = np.where(rng.random(H * W) < 0.5, rng.uniform(80.5, 200.0, H * W), np.nan).astype(np.float32)
    return np.where(mask, inside, outside).reshape(H, W)


def _run(monkeypatch, depth, bgr=None, top=0, left=0, row0=0, step=1, alpha=255, intr=INTR, dmin=DMIN, dmax=DMAX, offset=False):
    """kernels.depth_points twice under each poison byte, with the checks of the module docstring.  ``offset``: the map starts 4 bytes into
    its frame, so it is 4-byte but not 16-byte aligned.  Returns (count, the first ``count`` rows as a POINT_DTYPE array, the restatement)."""
    from gedepth_amd import cloud_kernels, hip, kernels
    ref = R.points_f32(depth, *intr, bgr, top, left, dmin, dmax, row0, step, alpha)
    h, w = depth.shape
    cap = R.capacity(h, w, row0, step)
    seen = []
    for poison in memguard.POISONS:
        guard = memguard.Guard(poison)
        guard.install(monkeypatch, [cloud_kernels], binding=hip)
        if offset:
            flat = guard.framed(torch.from_numpy(np.concatenate([np.zeros(1, np.float32), depth.reshape(-1)])).cuda())
            d_depth = flat[1:].view(h, w)
            assert d_depth.data_ptr() % 16 == 4
        else:
            d_depth = guard.framed(torch.from_numpy(depth).cuda())
        d_bgr = None if bgr is None else guard.framed(torch.from_numpy(bgr).cuda())
        outs = [kernels.depth_points(d_depth, *intr, d_bgr, top, left, float(dmin), float(dmax), row0, step, alpha) for _ in range(2)]
        torch.cuda.synchronize()
        monkeypatch.undo()
        frames = guard.check()                                    # red zones of the map, the frame and, per launch, records / count / workspace
        assert guard.launched == ['ge_depth_points'] * 2 and guard.direct.count('ge_depth_points_workspace') == 2
        own = [f for f in frames if os.path.basename(f.site[0]) == 'cloud_kernels.py']
        assert [tuple(f.shape) for f in own] == [(cap, 16), (1,), (hip.lib().ge_depth_points_workspace(h, w, row0, step) // 4,)] * 2
        for f in own[2::3]:
            assert not bool(f.poisoned().any()), 'a workspace word was never written'
        for records, count in outs:
            assert records.shape == (cap, 16) and records.dtype == torch.uint8 and count.shape == (1,) and count.dtype == torch.int32
            n = int(count.item())
            assert 0 <= n <= cap
            rows = records.cpu().numpy()
            assert (rows[n:] == poison).all(), 'bytes of records beyond 16 * count were written'
            seen.append((n, rows[:n].tobytes()))
    assert all(s == seen[0] for s in seen), 'two runs, or the runs under the two poison bytes, differ'
    n, blob = seen[0]
    return n, np.frombuffer(blob, dtype=R.POINT_DTYPE), ref


def _assert_equal(n, got, ref, what=''):
    assert n == ref.size, (what, n, ref.size)
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero(got != ref)[0]
        raise AssertionError(f'{what}: {bad.size} of {n} records differ; first at {bad[0]}: {got[bad[0]]} != {ref[bad[0]]}')


def test_small_map_properties_on_the_host():
    """What the small case relies on, from the restatement alone: between 30 % and 70 % kept for every (row0, step), and every special value
    among the candidates of each."""
    assert SMALL.shape == (37, 83) and R.capacity(H, W) == 3071
    for row0 in (0, 5):
        for step in (1, 2, 3):
            kept = R.points_f32(SMALL, *INTR, None, 0, 0, DMIN, DMAX, row0, step).size
            cap = R.capacity(H, W, row0, step)
            assert 0.3 * cap <= kept <= 0.7 * cap, (row0, step, kept, cap)
            cand = SMALL[row0::step, ::step].reshape(-1)
            for v in SPECIAL:
                assert (np.isnan(cand).any() if np.isnan(v) else (cand == v).any()), (row0, step, v)
    z = R.points_f32(SMALL, *INTR, None, 0, 0, DMIN, DMAX)['z']
    assert (z == DMIN).any() and (z == DMAX).any() and np.isfinite(z).all()
    assert not (z == SPECIAL[7]).any() and not (z == SPECIAL[10]).any() and (z == SPECIAL[8]).any() and (z == SPECIAL[9]).any()


@pytest.mark.parametrize('colour', ['bgr', 'white'])
@pytest.mark.parametrize('step', [1, 2, 3])
@pytest.mark.parametrize('row0', [0, 5])
def test_small_map_bit_exact_under_guards(monkeypatch, row0, step, colour):
    bgr = FRAME if colour == 'bgr' else None
    n, got, ref = _run(monkeypatch, SMALL, bgr, TOP if bgr is not None else 0, LEFT if bgr is not None else 0, row0, step, alpha=200 + step,
                       offset=True)
    _assert_equal(n, got, ref, f'row0={row0} step={step} {colour}')
    assert 0 < n < R.capacity(H, W, row0, step)
    if bgr is None:
        assert (got['red'] == 255).all() and (got['green'] == 255).all() and (got['blue'] == 255).all()
    assert (got['alpha'] == 200 + step).all()


IDX = np.arange(H * W)
MASKS = {
    'nothing': np.zeros(H * W, bool),
    'everything': np.ones(H * W, bool),
    'first-candidate': IDX == 0,
    'last-candidate': IDX == H * W - 1,
    'lane-63-of-every-wave': IDX % 64 == 63,
    'every-other-wave': (IDX // 64) % 2 == 0,
}


@pytest.mark.parametrize('name', list(MASKS))
def test_structured_masks(monkeypatch, name):
    n, got, ref = _run(monkeypatch, _masked(MASKS[name]), FRAME, TOP, LEFT, offset=True)
    _assert_equal(n, got, ref, name)
    assert n == int(MASKS[name].sum())
    if name == 'nothing':
        assert n == 0                                              # and _run has found every byte of records still poison
    if name == 'everything':
        assert n == R.capacity(H, W) == 3071


def _big_case(monkeypatch, h, w, seed):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.0, 120.0, (h, w)).astype(np.float32)
    depth[rng.random((h, w)) < 0.01] = np.nan
    frame = rng.integers(0, 256, (h + 23, w + 26, 3), dtype=np.uint8)
    intr = (721.5377, 721.5377, 609.5593 - 13, 172.854 - 23)
    n, got, ref = _run(monkeypatch, depth, frame, 23, 13, intr=intr)
    assert n == ref.size and 0.5 * h * w < n < 0.8 * h * w
    assert got[0] == ref[0] and got[-1] == ref[-1]
    assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(ref.tobytes()).hexdigest()


def test_kitti_sized_map(monkeypatch):
    """352 x 1216: 418 spans of 1024 candidates, more workspace entries than the 256 threads of the block that folds them."""
    from gedepth_amd import hip
    assert hip.lib().ge_depth_points_workspace(352, 1216, 0, 1) // 4 > 256
    _big_case(monkeypatch, 352, 1216, 8)


def test_span_grows_past_the_grid_cap(monkeypatch):
    """1024 x 1100 = 1 126 400 candidates: more than 1024 spans of 1024, so the span grows (5 candidates per thread) and the grid stays
    at 880 blocks: the one other path of the launch code."""
    from gedepth_amd import hip
    assert hip.lib().ge_depth_points_workspace(1024, 1100, 0, 1) == 4 * 880
    _big_case(monkeypatch, 1024, 1100, 9)


def test_depth_to_points_numpy_and_device():
    from gedepth_amd.depth.utils import POINT_DTYPE, depth_to_points
    K = [[INTR[0], 0.0, INTR[2]], [0.0, INTR[1], INTR[3]], [0.0, 0.0, 1.0]]
    ref = R.points_f32(SMALL, *INTR, FRAME, TOP, LEFT, DMIN, DMAX, 5, 2, 77)
    host = depth_to_points(SMALL[None], np.array(K), FRAME, TOP, LEFT, 1e-3, 80.0, row0=5, step=2, alpha=77)       # numpy in, numpy out
    assert isinstance(host, np.ndarray) and host.dtype == POINT_DTYPE and host.tobytes() == ref.tobytes()
    records, count = depth_to_points(torch.from_numpy(SMALL).cuda(), [row + [0.0] for row in K],
                                     torch.from_numpy(FRAME).cuda(), TOP, LEFT, row0=5, step=2, alpha=77)
    assert records.is_cuda and count.is_cuda and int(count) == ref.size
    assert records[:ref.size].cpu().numpy().tobytes() == ref.tobytes()
    with pytest.raises(RuntimeError, match='bad argument'):
        depth_to_points(SMALL, K, FRAME, TOP + 6, LEFT)                                  # the window leaves the frame
    with pytest.raises(ValueError, match='row0'):
        depth_to_points(SMALL, K, row0=37)


# ------------------------------------------------------------------------------------------------ the engine, on the toy tree
@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import test_inference_gpu as TI
    root = str(tmp_path_factory.mktemp('kitti_cloud'))
    split = make_toy_kitti(root, seed=4, frames=1)
    model = TI._model('depthformer_swint_v.py', root, split)
    img = os.path.join(root, 'input', '2011_09_26', '2011_09_26_drive_0001_sync', 'image_02', 'data', '0000000005.png')
    return model, img


def _engine_ref(eng, img):
    """The restatement on ``static_out`` as the last call left it: the frame's KB-crop window, the crop-shifted intrinsics of the day."""
    from gedepth_amd.depth.apis.inference import _decode
    from gedepth_amd.depth.datasets.kitti import _P_RECT
    frame = _decode(img)
    top, left = frame.shape[0] - 352, int((frame.shape[1] - 1216) / 2)
    P = _P_RECT['2011_09_26']
    head = eng.model.decode_head
    depth = eng.static_out.cpu().numpy()
    return R.points_f32(depth, P[0][0], P[1][1], P[0][2] - left, P[1][2] - top, frame, top, left, head.min_depth, head.max_depth)


def test_engine_points_bit_exact_and_same_graph(toy):
    from gedepth_amd.depth.apis.inference import DepthInferencer
    model, img = toy
    eng = DepthInferencer(model)
    for call in range(3):                                          # two eager calls, then the capture: each compared within its own run
        records, count = eng.points(img)
        assert records.is_cuda and records.shape == (352 * 1216, 16) and count.shape == (1,)
        ref = _engine_ref(eng, img)
        n = int(count.item())
        assert n == ref.size > 1000, (call, n, ref.size)
        assert records[:n].cpu().numpy().tobytes() == ref.tobytes(), call
        assert eng.captures == (1 if call == 2 else 0)
    assert list(eng.graphs) == [eng._key()]
    assert eng(img, to_host=False) is eng.static_out and eng.captures == 1 and list(eng.graphs) == [eng._key()]      # __call__ replays it
    sub, cnt = eng.points(img, row0=100, step=4, alpha=0, max_depth=40.0)
    assert sub.shape == (63 * 304, 16) and 0 <= int(cnt) <= 63 * 304 and eng.captures == 1


def test_inference_point_cloud_writes_what_it_returns(toy, tmp_path):
    from gedepth_amd.depth.apis import inference_point_cloud
    from gedepth_amd.depth.utils import POINT_DTYPE
    model, img = toy
    out = tmp_path / 'clouds' / 'frame.ply'
    clouds = inference_point_cloud(model, img, out_file=str(out))
    assert len(clouds) == 1 and clouds[0].dtype == POINT_DTYPE and clouds[0].size > 1000
    header, back = R.read_ply(out)
    assert header == R.HEADER.format(n=clouds[0].size).encode('ascii') and back.tobytes() == clouds[0].tobytes()
    eng = model._ge_inferencers[False]
    assert clouds[0].tobytes() == _engine_ref(eng, img).tobytes()                        # static_out is still this call's map
    two = inference_point_cloud(model, [img, img], out_file=[str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')], step=8)
    assert len(two) == 2 and all(R.read_ply(tmp_path / f)[1].tobytes() == c.tobytes() for f, c in zip(('a.ply', 'b.ply'), two))


# ------------------------------------------------------------------------------------------------ tools/test.py --ply-dir
def test_cli_ply_dir(tmp_path):
    """One run writes the clouds and, through --format-only --show-dir, the raw maps they were made from (two runs of the forward are not
    bit-reproducible, so the maps of another run would not do)."""
    import test_visualize_gpu as TV
    from gedepth_amd.depth.apis.inference import _decode
    from gedepth_amd.depth.datasets import build_dataset
    from gedepth_amd.depth.datasets.kitti import _P_RECT
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
    ply, raw = tmp_path / 'ply', tmp_path / 'raw'
    TV._run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), CONFIG, ckpt, '--ply-dir', str(ply), '--format-only', '--show-dir', str(raw),
             '--options', f'data.test.data_root={root}', f'data.test.split={split}', 'data.workers_per_gpu=0'])
    head, P = model.decode_head, _P_RECT['2011_09_26']
    found = sorted(os.path.relpath(os.path.join(d, f), ply) for d, _, fs in os.walk(ply) for f in fs)
    assert found == sorted(n[:-4] + '.ply' for n in names)
    for n in names:
        depth = np.load(raw / (n[:-4] + '.npy'))
        frame = _decode(os.path.join(ds.img_dir, n))
        top, left = frame.shape[0] - 352, int((frame.shape[1] - 1216) / 2)
        ref = R.points_f32(depth, P[0][0], P[1][1], P[0][2] - left, P[1][2] - top, frame, top, left, head.min_depth, head.max_depth)
        header, got = R.read_ply(ply / (n[:-4] + '.ply'))
        assert header == R.HEADER.format(n=ref.size).encode('ascii') and ref.size > 1000, n
        assert got.tobytes() == ref.tobytes(), n


def test_cli_ply_dir_with_device_eval_raises():
    import importlib.util
    spec = importlib.util.spec_from_file_location('ge_tools_test_ply_gpu', os.path.join(ROOT, 'tools', 'test.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(ValueError, match='--device-eval'):
        tool.parse_args([CONFIG, '--device-eval', '--eval', 'x', '--synthetic', '0', '--ply-dir', 'd'])
    from gedepth_amd.depth.apis.test import single_gpu_test

    class Loader:
        dataset = None
        batch_sampler = []
    with pytest.raises(NotImplementedError, match='ply_dir'):
        single_gpu_test(torch.nn.Identity(), Loader(), pre_eval=True, device_eval=True, ply_dir='d')

"""The ground maps on the MI355X: ``ge_ground_maps`` (csrc/ground.hip) under red zones and both poison bytes (tests/memguard.py) against the
training path's own kernels and the float64 restatement (tests/ground_ref.py); ``DepthInferencer.ground_maps`` on the toy KITTI and DDAD
trees, eager and replayed; ``inference_ground`` and tools/test.py's ``--ground-dir`` end to end.

Every kernel case runs twice under each poison byte.  Checked each time: every red zone; no element of ``maps`` or ``valid`` left holding
the poison pattern; exactly two launches of ``ge_ground_maps``; the two runs, and the runs under 0xFF and 0x7F, identical byte for byte."""
import contextlib
import functools
import gc
import os
import sys

import numpy as np
import pytest
import torch

import ground_ref as G
import memguard
from toy_kitti import make_toy_kitti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
pytestmark = pytest.mark.gpu

SHAPES = [(33, 47), (24, 40)]      # odd W: the scalar path with a mirrored read; W % 4 == 0: the vector path
HEIGHTS = (1.56, 1.53)
ENGINE_EPS = 2e-4                  # engine vs the host route, per pixel and relative: the bound of test_inference_gpu.py / test_eval_device_gpu.py
KEYS = ('depth', 'attention', 'ground_term', 'ground_depth', 'slope_deg', 'valid')


def _drop_engines(*models):
    """A model and the engines ``engine_for`` keeps in it refer to each other.  Break the cycle and collect now, while nothing runs, so that
    no engine (its stream, pinned buffer, events and static tensors) is left for the collector to free in the middle of a later test."""
    for m in models:
        m.__dict__.pop('_ge_inferencers', None)
    torch.cuda.synchronize()
    gc.collect()


# ------------------------------------------------------------------------------------------------ the kernel
@functools.lru_cache(maxsize=None)
def _inputs(hw):
    """``test_kernels_gpu._ground_inputs(2, H, W, seed=H)``: the two batch entries are the two views.  Shared, never modified."""
    from test_kernels_gpu import _ground_inputs
    return _ground_inputs(2, *hw, seed=hw[0])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _run(monkeypatch, img, logits, y, height=None, flip=True, offset=False):
    """kernels.ground_maps twice under each poison byte, with the checks of the module docstring -> (maps, valid) on the host.  ``offset``:
    ``maps`` starts 4 bytes into its frame, so it is 4-byte but not 16-byte aligned."""
    from gedepth_amd import ground_kernels, hip, kernels
    V, _, H, W = img.shape
    seen = []
    for poison in memguard.POISONS:
        guard = memguard.Guard(poison)
        guard.install(monkeypatch, [ground_kernels], binding=hip)
        d_img, d_y = guard.framed(img.cuda()), guard.framed(y.cuda())
        d_logits = None if logits is None else guard.framed(logits.cuda())
        d_height = None if height is None else guard.framed(height.cuda())
        outs = []
        for _ in range(2):
            out = None
            if offset:
                flat = guard.proxy.empty(4 * H * W + 1, device='cuda', dtype=torch.float32)
                out = flat[1:].view(4, H, W)
                assert out.data_ptr() % 16 == 4
            outs.append(kernels.ground_maps(d_logits, d_y, d_img, d_height, 200.0, 200.0, flip, out=out) + (flat[:1] if offset else None,))
        torch.cuda.synchronize()
        monkeypatch.undo()
        frames = guard.check()                                        # red zones of the inputs and, per launch, of maps and valid
        assert guard.launched == ['ge_ground_maps'] * 2
        own = [f for f in frames if os.path.basename(f.site[0]) == 'ground_kernels.py']
        assert [tuple(f.shape) for f in own] == ([(H, W)] if offset else [(4, H, W), (H, W)]) * 2
        for maps, valid, before in outs:
            assert maps.shape == (4, H, W) and maps.dtype == torch.float32 and valid.shape == (H, W) and valid.dtype == torch.uint8
            assert not bool(memguard.poisoned(maps, poison).any()), 'an element of maps was never written'
            assert not bool(memguard.poisoned(valid, poison).any()), 'an element of valid was never written'
            assert before is None or bool(memguard.poisoned(before, poison).all()), 'the element before an offset maps was written'
            seen.append((_bits(maps).cpu(), valid.cpu()))
    assert all(torch.equal(m, seen[0][0]) and torch.equal(v, seen[0][1]) for m, v in seen), \
        'two runs, or the runs under the two poison bytes, differ'
    return seen[0][0].view(torch.float32), seen[0][1]


def _same(got, ref, what):
    """``torch.equal``; where both hold NaN, the same bits."""
    assert torch.equal(got, ref) or torch.equal(_bits(got), _bits(ref)), \
        f'{what}: {int((_bits(got) != _bits(ref)).sum())} of {got.numel()} elements differ from the training kernels\' composition'


def _rel(x, ref):
    d = (x.double() - ref).abs()
    return torch.where(ref != 0, d / ref.abs(), d)


def _check_adaptive(maps, valid, img, logits, y, height, what):
    """The value checks of an adaptive case (module docstring of tests/ground_ref.py for the two restatements) -> the printed figures."""
    from gedepth_amd import kernels
    V = img.shape[0]
    d_height = None if height is None else height.cuda()
    pe, _, y_hr, val = kernels.ground_embed_adaptive(logits.cuda(), y.cuda(), img.cuda(), d_height, 200.0)
    pe, y_hr, val = pe[:, 0].cpu(), y_hr[:, 0].cpu(), val.cpu()
    if V == 2:
        _same(maps[0], (y_hr[0] + y_hr[1].flip(-1)) * 0.5, f'{what} attention')
        _same(maps[1], (pe[0] + pe[1].flip(-1)) * 0.5, f'{what} ground_term')
        assert torch.equal(valid, val[0] + val[1].flip(-1)), f'{what} valid'
    else:
        _same(maps[0], y_hr[0], f'{what} attention')
        _same(maps[1], pe[0], f'{what} ground_term')
        assert torch.equal(valid, val[0]), f'{what} valid'
    m64, v64 = G.ground_maps(logits, y, img, height, dtype=torch.float64)
    m32, v32 = G.ground_maps(logits, y, img, height, dtype=torch.float32)
    amb = G.ambiguous(logits, y, img, height)
    assert int(amb.sum()) <= max(4, amb.numel() // 50000), int(amb.sum())
    assert torch.equal(valid[~amb], v64[~amb]), f'{what}: valid differs from the float64 one outside the ambiguous set'
    # slope_deg: the float32 CPU restatement's largest absolute error against float64 is the yardstick; the kernel gets 4 x it (its expf /
    # tanf and its un-contracted interpolation round differently from ATen's)
    yard_deg = float((m32[3].double() - m64[3]).abs().max())
    kern_deg = float((maps[3].double() - m64[3]).abs().max())
    # ground_depth: the same scheme, relative, over the pixels whose valid agrees with the float64 one outside the ambiguous set
    yard_gd = float(_rel(m32[2], m64[2])[(v32 == v64) & ~amb].max())
    kern_gd = float(_rel(maps[2], m64[2])[(valid == v64) & ~amb].max())
    print(f'\n[{what}] slope_deg: yardstick {yard_deg:.2e} deg, kernel {kern_deg:.2e} deg; ground_depth: yardstick {yard_gd:.2e}, '
          f'kernel {kern_gd:.2e} (relative); ambiguous {int(amb.sum())}; valid 0/1/2: '
          f'{[round(float((valid == k).float().mean()), 3) for k in range(3)]}')
    assert kern_deg <= 4 * yard_deg, (what, kern_deg, yard_deg)
    assert kern_gd <= 4 * yard_gd, (what, kern_gd, yard_gd)
    assert float(maps[3].abs().max()) <= 5.0 and float(maps[3].abs().max()) > 0.1
    for k in range(V + 1):                                             # the inputs take every branch of the merge
        assert bool((valid == k).any()), f'{what}: no pixel with {k} valid views'
    return maps, valid


@pytest.mark.parametrize('use_height', [False, True], ids=['h165', 'heights'])
@pytest.mark.parametrize('hw', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_two_views_under_guards(monkeypatch, hw, use_height):
    """Bounds: 4 x the yardstick, the float32 CPU restatement's own largest error against float64 on the same inputs (``_check_adaptive``).
    Measured on an MI355X, yardstick / kernel — slope_deg, absolute, in degrees: (24, 40) 5.84e-7 / 5.19e-7, (33, 47) 4.95e-6 / 4.83e-6,
    the same with both height settings; ground_depth, relative: (24, 40) 8.66e-7 / 8.66e-7 at 1.65 m and 9.11e-7 / 9.11e-7 with the two
    heights, (33, 47) 4.32e-6 / 4.29e-6 and 5.55e-6 / 5.55e-6.  One view (test_one_view_under_guards): slope_deg (24, 40) 1.13e-6 /
    8.38e-7, (33, 47) 6.92e-6 / 7.04e-6; ground_depth 7.32e-7 / 7.32e-7 and 6.36e-6 / 5.56e-6.  The ambiguous set is empty in every case;
    49 % of the pixels have no valid view, 6 % one, 44 % both.  attention, ground_term and valid equal the training kernels'
    composition bit for bit."""
    img, logits, y = _inputs(hw)
    height = torch.tensor(HEIGHTS) if use_height else None
    maps, valid = _run(monkeypatch, img, logits, y, height)
    _check_adaptive(maps, valid, img, logits, y, height, f'{hw} V=2 {"heights" if use_height else "1.65"}')


@pytest.mark.parametrize('hw', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_one_view_under_guards(monkeypatch, hw):
    img, logits, y = _inputs(hw)
    img, logits, y = img[1:].contiguous(), logits[1:].contiguous(), y[1:].contiguous()      # view 1 alone: nothing is mirrored for V = 1
    height = torch.tensor(HEIGHTS[1:])
    maps, valid = _run(monkeypatch, img, logits, y, height)
    _check_adaptive(maps, valid, img, logits, y, height, f'{hw} V=1')
    assert int(valid.max()) == 1


def test_maps_4_bytes_into_their_frame_take_the_scalar_path_with_the_same_bits(monkeypatch):
    hw = (24, 40)
    img, logits, y = _inputs(hw)
    aligned = _run(monkeypatch, img, logits, y)
    shifted = _run(monkeypatch, img, logits, y, offset=True)
    assert torch.equal(_bits(aligned[0]), _bits(shifted[0])) and torch.equal(aligned[1], shifted[1])


@pytest.mark.parametrize('hw', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_vanilla_under_guards(monkeypatch, hw):
    """``logits_lr=None``: channel 3, bit-equal to ``ground_embed_vanilla``'s composition and to ``img[:, 3] * 200`` with the ``> 0`` rule."""
    from gedepth_amd import kernels
    img, _, y = _inputs(hw)
    img = img.clone()                                  # the plane's validity goes by rows, the same in both views: cut a strip out of each
    img[0, 3, :, :hw[1] // 4] = 0                      # output columns left of W / 4: view 1 alone
    img[1, 3, :, :hw[1] // 3] = 0                      # view 1 is mirrored: output columns from W - W / 3 on have view 0 alone
    maps, valid = _run(monkeypatch, img, None, y)
    pe, y_hr = kernels.ground_embed_vanilla(y.cuda(), img.cuda(), 200.0)
    pe, y_hr = pe[:, 0].cpu(), y_hr[:, 0].cpu()
    _same(maps[0], (y_hr[0] + y_hr[1].flip(-1)) * 0.5, 'vanilla attention')
    _same(maps[1], (pe[0] + pe[1].flip(-1)) * 0.5, 'vanilla ground_term')
    off, ok = img[:, 3] * 200.0, img[:, 3] > 0
    want, want_valid = G.merge(dict(y=y_hr, t=pe, off=off, deg=torch.zeros_like(off), ok=ok))
    _same(maps[2], want[2], 'vanilla ground_depth')
    assert torch.equal(valid, want_valid) and set(valid.unique().tolist()) == {0, 1, 2}
    assert torch.equal(maps[3], torch.zeros(hw))


def test_wrapper_argument_errors():
    from gedepth_amd import kernels
    img, logits, y = _inputs((24, 40))
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.ground_maps(logits, y, img)
    with pytest.raises(RuntimeError, match='MI355X only'):
        kernels.ground_maps(logits.cuda(), y.cuda(), img)
    with pytest.raises(ValueError, match='one or two views'):
        kernels.ground_maps(None, y.cuda().repeat(2, 1, 1, 1)[:3], img.cuda().repeat(2, 1, 1, 1)[:3].contiguous())
    with pytest.raises(ValueError, match='logits_lr must be'):
        kernels.ground_maps(logits.cuda()[:, :10], y.cuda(), img.cuda())
    bf = kernels.ground_maps(logits.cuda().bfloat16(), y.cuda().bfloat16(), img.cuda())            # the necks' dtype under bf16 autocast
    f32 = kernels.ground_maps(logits.cuda().bfloat16().float(), y.cuda().bfloat16().float(), img.cuda())
    assert torch.equal(_bits(bf[0]), _bits(f32[0])) and torch.equal(bf[1], f32[1])


# ------------------------------------------------------------------------------------------------ the engine, KITTI
def _exact_variants(model):
    for m in model.modules():
        if hasattr(m, 'kernel_variant'):
            m.kernel_variant = 1
    return model


def _kitti_model(cfg_name, root, split):
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    cfg = Config.fromfile(os.path.join(CFG, cfg_name))
    cfg.data.test.data_root, cfg.data.test.split = root, split
    cfg.model.pretrained = None
    torch.manual_seed(0)
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.init_weights()
    model.cfg = cfg
    return _exact_variants(model.cuda().eval())


@pytest.fixture(scope='module')
def kitti(tmp_path_factory):
    """Toy KITTI tree (one frame per drive), random-init depthformer_swint_a.py with the exact kernel variants, and the frames' paths."""
    from gedepth_amd.depth.datasets import build_dataset
    root = str(tmp_path_factory.mktemp('kitti_ground'))
    split = make_toy_kitti(root, frames=1)
    model = _kitti_model('depthformer_swint_a.py', root, split)
    ds = build_dataset(model.cfg.data.test, dict(test_mode=True))
    paths = [ds.engine_frame(i)['img'] for i in range(len(ds))]
    assert len(paths) == 2
    yield model, ds, paths, root, split
    _drop_engines(model)


@contextlib.contextmanager
def _neck_outputs(model):
    """Forward hooks on the two ground necks: the dict holds ``logits`` / ``y`` of the model's latest forward."""
    seen = {}
    hooks = [model.pe_mask_neck.register_forward_hook(lambda m, i, o: seen.__setitem__('y', o[0]))]
    if model.dynamic_pe_neck_FLAGS:
        hooks.append(model.dynamic_pe_neck.register_forward_hook(lambda m, i, o: seen.__setitem__('logits', o)))
    try:
        yield seen
    finally:
        for h in hooks:
            h.remove()


@contextlib.contextmanager
def _reproducible_convolutions():
    """As in test_ddad_device_gpu.py: with deterministic convolution algorithms the whole eval forward repeats its bits."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


def _assert_dict(out, H, W, slope=True, host=True):
    want = [k for k in KEYS if slope or k != 'slope_deg']
    assert sorted(out) == sorted(want), sorted(out)
    for k in want:
        v = out[k]
        assert isinstance(v, np.ndarray) if host else (torch.is_tensor(v) and v.is_cuda), k
        assert tuple(v.shape) == ((1, H, W) if k == 'depth' else (H, W)), (k, v.shape)
        assert str(v.dtype).split('.')[-1] == ('uint8' if k == 'valid' else 'float32'), (k, v.dtype)


def _assert_matches_kernel(out, ref_maps, ref_valid, eng, slope=True):
    from gedepth_amd.ground_kernels import PLANES
    for k, plane in zip(PLANES, ref_maps):
        if k == 'slope_deg' and not slope:
            continue
        assert torch.equal(_bits(out[k]), _bits(plane)), k
    assert torch.equal(out['valid'], ref_valid) and torch.equal(out['depth'], eng.static_out)


def test_kitti_engine_eager_equals_the_kernel_on_the_hooked_neck_outputs(kitti):
    from gedepth_amd import kernels
    from gedepth_amd.depth.apis import inference_depther
    from gedepth_amd.depth.apis.inference import DepthInferencer
    model, _, paths, _, _ = kitti
    eng = DepthInferencer(model)
    assert eng.static_ground is None and eng.static_ground_valid is None            # allocated on first use
    with _neck_outputs(model) as seen:
        out = eng.ground_maps(paths[0], graph=False, to_host=False)
    _assert_dict(out, 352, 1216, host=False)
    assert out['depth'] is eng.static_out and out['valid'] is eng.static_ground_valid and eng.static_ground.shape == (4, 352, 1216)
    assert model.keep_ground_lr is False and model.ground_lr is None                 # the flag is off again, nothing is retained
    assert seen['logits'].shape[:2] == (2, 11) and seen['y'].shape[:2] == (2, 1) and seen['logits'].shape[2:] == seen['y'].shape[2:]
    ref_maps, ref_valid = kernels.ground_maps(seen['logits'], seen['y'], eng.static_in, None, model.depth_scale, 200.0, True)
    _assert_matches_kernel(out, ref_maps, ref_valid, eng)
    depth = out['depth'].cpu().numpy()
    host = inference_depther(model, paths[0], graph=False)[0]
    rel = float((np.abs(depth - host) / np.maximum(np.abs(host), 1e-3)).max())
    print(f'\n[kitti ground engine] depth vs inference_depther: largest relative difference {rel:.2e}')
    assert rel <= ENGINE_EPS
    att, valid = out['attention'].cpu().numpy(), out['valid'].cpu().numpy()
    assert att.min() >= 0.0 and att.max() <= 1.0 and set(np.unique(valid)) <= {0, 1, 2} and (valid == 2).any()
    assert eng.captures == 0 and not eng.graphs
    _drop_engines(model)


def test_kitti_engine_replay_is_bit_identical_and_keyed_apart(kitti):
    from gedepth_amd.depth.apis.inference import DepthInferencer
    model, _, paths, _, _ = kitti
    with _reproducible_convolutions():
        eng = DepthInferencer(model)
        eager = [eng.ground_maps(p, graph=False) for p in paths]
        for _ in range(2):
            eng.ground_maps(paths[0])                                                 # two eager calls ...
        assert eng.captures == 0
        eng.ground_maps(paths[0])                                                     # ... then the capture
        assert eng.captures == 1
        replay = [eng.ground_maps(p) for p in paths]
        assert eng.captures == 1 and list(eng.graphs) == [eng._key(True)] and eng._key(True) != eng._key()
        plain = eng(paths[1])                                                         # its own key: eager, and its own map
        assert eng.captures == 1 and list(eng.graphs) == [eng._key(True)] and eng.calls[eng._key()] == 1
        records, count = eng.points(paths[0], ground=True)                            # either mode fills static_out and last_frame
        assert eng.captures == 1 and int(count.item()) > 1000
    for e, r in zip(eager, replay):
        _assert_dict(r, 352, 1216)
        for k in KEYS:
            assert e[k].tobytes() == r[k].tobytes(), f'{k}: the replay differs from the eager run'
    assert not np.array_equal(replay[0]['attention'], replay[1]['attention'])          # a stale static buffer would repeat a map
    assert plain.tobytes() == eager[1]['depth'].tobytes()


def test_kitti_vanilla_engine_has_no_slope(kitti):
    from gedepth_amd.depth.apis.inference import DepthInferencer
    _, _, paths, root, split = kitti
    model = _kitti_model('depthformer_swint_v.py', root, split)
    out = DepthInferencer(model).ground_maps(paths[0], graph=False)
    _assert_dict(out, 352, 1216, slope=False)
    att = out['attention']
    assert np.isfinite(att).all() and att.min() >= 0.0 and att.max() <= 1.0 and np.isfinite(out['ground_term']).all()
    assert set(np.unique(out['valid'])) <= {0, 1, 2} and (out['valid'] == 2).any() and (out['valid'] == 0).any()


# ------------------------------------------------------------------------------------------------ the engine, DDAD
@pytest.fixture(scope='module')
def ddad(tmp_path_factory):
    """The ``toy`` fixture of test_ddad_device_gpu.py: random-init depthformer_a_ddad.py at Swin-T width, the toy DDAD tree (96 x 160 frames),
    DDADResize to (48, 80); two frames each of CAMERA_01 and CAMERA_05."""
    from test_dataset_cpu import _make_toy_ddad
    from test_ddad_device_gpu import _test_pipeline
    from gedepth_amd.depth.datasets import build_dataset
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    root = str(tmp_path_factory.mktemp('ddad_ground'))
    split = _make_toy_ddad(root, frames=2, seed=5)
    cfg = Config.fromfile(os.path.join(CFG, 'depthformer_a_ddad.py'))
    swin_t, rev = [64, 96, 192, 384, 768], [768, 384, 192, 96, 64]
    cfg.model.pretrained = None
    cfg.model.backbone.update(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24])
    cfg.model.neck.update(in_channels=swin_t, out_channels=swin_t)
    cfg.model.pe_mask_neck.in_channels = rev
    cfg.model.dynamic_pe_neck.in_channels = rev
    cfg.model.decode_head.update(in_channels=swin_t, up_sample_channels=swin_t)
    cfg.data.test.pipeline = _test_pipeline(os.path.join(root, 'pe'), (48, 80))
    cfg.data.test.split = split
    torch.manual_seed(0)
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.init_weights()
    model.cfg = cfg
    model = _exact_variants(model.cuda().eval())
    ds = build_dataset(cfg.data.test, dict(test_mode=True))
    frames = [ds.engine_frame(i) for i in (0, 2)]
    assert [f['camera'] for f in frames] == ['CAMERA_01', 'CAMERA_05']
    yield model, frames
    _drop_engines(model)


def test_ddad_engine_one_view_with_the_cameras_height(ddad):
    from gedepth_amd import kernels
    from gedepth_amd.depth.apis.inference import DepthInferencer
    from gedepth_amd.depth.datasets.pipelines import loading
    model, frames = ddad
    eng = DepthInferencer(model)
    assert eng.static_in.shape[0] == 1
    for frame in frames:
        with _neck_outputs(model) as seen:
            out = eng.ground_maps(graph=False, to_host=False, **frame)
        _assert_dict(out, 48, 80, host=False)
        height = torch.tensor([loading._DDAD_CAMERA_HEIGHT[frame['camera']]], device='cuda', dtype=torch.float32)
        assert torch.equal(eng.static_height, height)
        ref_maps, ref_valid = kernels.ground_maps(seen['logits'], seen['y'], eng.static_in, height, model.depth_scale, 200.0, False)
        _assert_matches_kernel(out, ref_maps, ref_valid, eng)
        assert int(out['valid'].max()) <= 1


def test_ddad_graph_captured_on_one_camera_replays_for_the_other(ddad, monkeypatch):
    """The heights are set 1.0 m apart, as test_ddad_device_gpu.py::test_graph_replay_follows_the_camera_height sets them, so that a height
    baked into the graph would show in every map."""
    from gedepth_amd.depth.apis.inference import DepthInferencer
    from gedepth_amd.depth.datasets.pipelines import loading
    monkeypatch.setattr(loading, '_DDAD_CAMERA_HEIGHT', {'CAMERA_01': 1.2, 'CAMERA_05': 2.2, 'CAMERA_06': 1.53, 'CAMERA_09': 1.53})
    model, (f01, f05) = ddad
    with _reproducible_convolutions():
        eng = DepthInferencer(model)
        eager05 = eng.ground_maps(graph=False, **f05)
        eager05_as01 = eng.ground_maps(graph=False, **dict(f05, camera='CAMERA_01'))
        for _ in range(3):
            eng.ground_maps(**f01)                                                    # CAMERA_01's height is in the buffer at the capture
        assert eng.captures == 1
        replay05 = eng.ground_maps(**f05)
        replay05_as01 = eng.ground_maps(**dict(f05, camera='CAMERA_01'))
        assert eng.captures == 1
    _assert_dict(replay05, 48, 80)
    for k in KEYS:
        assert replay05[k].tobytes() == eager05[k].tobytes() and replay05_as01[k].tobytes() == eager05_as01[k].tobytes(), k
    assert not np.array_equal(replay05['ground_depth'], replay05_as01['ground_depth']), 'the camera height must reach a replayed graph'


# ------------------------------------------------------------------------------------------------ the API and the tool
def test_inference_ground_one_dict_per_frame(kitti):
    from gedepth_amd.depth.apis import inference_depther, inference_ground
    model, _, paths, _, _ = kitti
    outs = inference_ground(model, paths, graph=False)
    assert isinstance(outs, list) and len(outs) == 2
    for o in outs:
        _assert_dict(o, 352, 1216)
    assert outs[0]['depth'] is not outs[1]['depth'] and not np.array_equal(outs[0]['attention'], outs[1]['attention'])
    frame = np.zeros((375, 1242, 3), np.uint8)
    for api in (inference_ground, inference_depther):                                # the same argument errors, before any device work
        with pytest.raises(ValueError, match='no ground depth'):
            api(model, frame)
        with pytest.raises(ValueError, match='2 ground-depth maps for 1 frames'):
            api(model, frame, pe=[None, None])
    _drop_engines(model)


def test_ground_dir_in_the_same_pass_as_device_eval(kitti, tmp_path):
    """``single_gpu_test(device_eval=True, ground_dir=...)``: the metric tuples of the device evaluation and the pictures of every frame
    from one pass; with the host loop's ``pre_eval`` it refuses, naming ``device_eval``."""
    from gedepth_amd.depth.apis.test import replace_str, single_gpu_test
    from gedepth_amd.depth.datasets import build_dataloader
    model, ds, _, _, _ = kitti
    loader = lambda: build_dataloader(ds, 1, 0, dist=False, shuffle=False)
    with pytest.raises(NotImplementedError, match='device_eval=True'):
        single_gpu_test(model, loader(), pre_eval=True, ground_dir=str(tmp_path / 'no'))
    assert not (tmp_path / 'no').exists()
    _drop_engines(model)
    both = single_gpu_test(model, loader(), pre_eval=True, device_eval=True, ground_dir=str(tmp_path / 'maps'))
    eng = model._ge_inferencers[False]
    assert list(eng.calls) == [eng._key(True)] and eng._key() not in eng.calls        # one pass: every frame ran in ground mode
    _drop_engines(model)
    alone = single_gpu_test(model, loader(), pre_eval=True, device_eval=True)
    assert len(both) == len(alone) == 2 and all(isinstance(t, tuple) and len(t) == 9 for t in both)
    for a, b in zip(both, alone):                                                     # the same maps up to the convolutions' run-to-run noise
        assert np.allclose(a, b, rtol=1e-3, atol=2e-3, equal_nan=True), (a, b)
    stems = [os.path.splitext(replace_str(info['filename']))[0] for info in ds.img_infos]
    assert sorted(os.listdir(tmp_path / 'maps')) == sorted(f'{s}_{k}.png' for s in stems for k in ('attention', 'slope', 'ground'))
    assert single_gpu_test(model, loader(), ground_dir=str(tmp_path / 'raw'), format_only=True) == []
    # show_ground itself, on one host dict: each picture is colorize over the documented range, as show_result writes its picture
    from PIL import Image
    from gedepth_amd.depth.apis import inference_ground
    from gedepth_amd.depth.utils import colorize
    out = inference_ground(model, ds.engine_frame(0)['img'], graph=False)[0]
    model.show_ground(out, str(tmp_path / 'one' / 'frame.png'))
    head = model.decode_head
    for key, suffix, lo, hi in (('attention', 'attention', 0.0, 1.0), ('slope_deg', 'slope', -5.0, 5.0),
                                ('ground_depth', 'ground', head.min_depth, head.max_depth)):
        rgb = np.asarray(Image.open(tmp_path / 'one' / f'frame_{suffix}.png').convert('RGB'))
        assert np.array_equal(rgb, colorize(out[key], vmin=lo, vmax=hi)[..., ::-1]), key
    assert sorted(os.listdir(tmp_path / 'raw')) == sorted(s + '.npz' for s in stems)
    _drop_engines(model)


def test_cli_ground_dir(kitti, tmp_path):
    """tools/test.py --ground-dir in a fresh process: 3 pictures per frame at the map's size; with --format-only one .npz per frame whose
    maps are the API's.  The tool's process runs the convolution library's default algorithms, which do not repeat their bits from run to
    run (test_ddad_device_gpu.py::test_graph_replay_follows_the_camera_height measures 1.2e-6 .. 2.6e-6 relative per pixel on the depth),
    so "the API's" is held to ``ENGINE_EPS`` = 2e-4 absolute on the attention (a sigmoid, in [0, 1]), the bound every engine comparison
    in this suite uses; the largest difference is printed."""
    import test_visualize_gpu as TV
    from PIL import Image
    from gedepth_amd.depth.apis import inference_ground, init_depther
    from gedepth_amd.depth.apis.test import replace_str
    from gedepth_amd.mmrt.checkpoint import save_checkpoint
    model, ds, paths, root, split = kitti
    ckpt = str(tmp_path / 'model.pth')
    save_checkpoint(model, ckpt)
    names = [info['filename'] for info in ds.img_infos]
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'test.py'), os.path.join(CFG, 'depthformer_swint_a.py'), ckpt]
    opts = ['--options', f'data.test.data_root={root}', f'data.test.split={split}', 'data.workers_per_gpu=0']
    png, raw = tmp_path / 'png', tmp_path / 'raw'
    TV._run(cmd + ['--ground-dir', str(png)] + opts)
    stems = [os.path.splitext(replace_str(n))[0] for n in names]
    assert sorted(os.listdir(png)) == sorted(f'{s}_{k}.png' for s in stems for k in ('attention', 'slope', 'ground'))
    for f in os.listdir(png):
        assert Image.open(png / f).size == (1216, 352), f
    assert len({(png / f).read_bytes() for f in os.listdir(png)}) == 6                # six different pictures
    TV._run(cmd + ['--ground-dir', str(raw), '--format-only'] + opts)
    assert sorted(os.listdir(raw)) == sorted(s + '.npz' for s in stems)
    loaded = init_depther(model.cfg, ckpt)             # the tool's model: the checkpoint with the default kernel variants
    api = inference_ground(loaded, paths, graph=False)
    for s, want in zip(stems, api):
        with np.load(raw / (s + '.npz')) as z:
            got = {k: z[k] for k in z.files}
        _assert_dict(got, 352, 1216)
        diff = float(np.abs(got['attention'] - want['attention']).max())
        print(f'\n[--ground-dir {s}] attention vs inference_ground: largest difference {diff:.2e}, '
              f'bit-identical {np.array_equal(got["attention"], want["attention"])}')
        assert diff <= ENGINE_EPS
    _drop_engines(loaded, model)

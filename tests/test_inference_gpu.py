"""Single-frame inference on MI355X (gedepth_amd/depth/apis/inference.py, csrc/infer.hip): the front end against the reference-written
test-pipeline fixture and against the training pipeline's kernels, the merge against ATen, the engine against ``aug_test`` / the CPU
oracle, graph replay, the ground-depth sources, the other configurations and a checkpoint round trip."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from toy_kitti import make_toy_kitti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'kitti_pipeline.npz')
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
KITTI_SIZES = ((375, 1242), (370, 1224), (374, 1238), (376, 1241))
pytestmark = pytest.mark.gpu


def _rel(got, ref):
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)
    return rel.max(), rel.mean()


def _exact_variants(model):
    for m in model.modules():
        if hasattr(m, 'kernel_variant'):
            m.kernel_variant = 1
    return model


def _model(cfg_name, root, split, flip=True):
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    cfg = Config.fromfile(os.path.join(CFG, cfg_name))
    cfg.data.test.data_root, cfg.data.test.split = root, split
    aug = next(t for t in cfg.data.test.pipeline if t['type'] == 'MultiScaleFlipAug')
    aug['flip'] = flip
    cfg.model.pretrained = None
    torch.manual_seed(0)
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.init_weights()
    model.cfg = cfg
    return _exact_variants(model.cuda().eval())


def _host_route(model):
    """Today's route for the first test frame: the host test pipeline and ``model(return_loss=False)`` (aug_test / simple_test)."""
    from gedepth_amd.depth.apis.test import _to_device
    from gedepth_amd.depth.datasets import build_dataloader, build_dataset
    ds = build_dataset(model.cfg.data.test, dict(test_mode=True))
    batch = next(iter(build_dataloader(ds, 1, 0, dist=False, shuffle=False)))
    with torch.no_grad():
        got = model(return_loss=False, rescale=True, **_to_device(batch, 'cuda'))
    return os.path.join(ds.img_dir, ds.img_infos[0]['filename']), batch, got[0]


def _plane(H, W):
    v = np.arange(H, dtype=np.float64).reshape(H, 1)
    return (np.where(v > 173.0, 1.65 * 721.5377 / np.maximum(v - 172.854, 1e-6), -5.0) * np.ones((1, W))).astype(np.float32)


def _frame(seed, H=375, W=1242):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    meta = json.loads(str(np.load(FIXTURE)['meta']))
    root = str(tmp_path_factory.mktemp('kitti_infer'))
    split = make_toy_kitti(root, seed=meta['toy_seed'])
    return root, split


@pytest.fixture(scope='module')
def vanilla(toy):
    return _model('depthformer_swint_v.py', *toy)


def _front(bgr_np, pe_np, views=2):
    from gedepth_amd import kernels as K
    H, W = bgr_np.shape[:2]
    out = torch.empty(views, 5, 352, 1216, device='cuda')
    K.infer_front(torch.from_numpy(bgr_np).cuda(), torch.from_numpy(pe_np).cuda(), out, H - 352, int((W - 1216) / 2),
                  [float(np.float32(v)) for v in MEAN], [float(np.float32(v)) for v in STD])
    return out


def test_front_end_matches_reference_fixture(toy):
    """Both flip views of ge_infer_front against the reference's own test pipeline output (kitti_pipeline.npz), element for element."""
    from PIL import Image
    root, _ = toy
    g = np.load(FIXTURE)
    meta = json.loads(str(g['meta']))
    sy, sx = meta['strides']
    pe = np.load(os.path.join(root, 'input', '2011_09_26', 'pe', 'pe_165.npy')).astype(np.float32)
    for m in meta['test']:
        bgr = np.ascontiguousarray(np.asarray(Image.open(os.path.join(root, m['filename'])).convert('RGB'))[..., ::-1])
        img = _front(bgr, pe)[m['aug']].cpu().numpy()
        tag = f'test{m["index"]}_{m["aug"]}'
        assert np.array_equal(img[:, ::sy, ::sx], g[f'{tag}_img']), tag
        assert np.allclose(img.astype(np.float64).sum((1, 2)), g[f'{tag}_sum'], rtol=1e-12, atol=1e-9), tag


def _chain(bgr, pe, top, left, Hc, Wc, pe_max=200.0, depth_scale=200.0):
    """The training pipeline's chain for the (Hc, Wc) window at (top, left) of one frame (device tensors ``bgr`` uint8 HWC, ``pe`` f32):
    ge_aug_load -> ge_aug_color_normalize(color_on=0) -> ge_aug_window(flip) -> [view 0, view 1], each (5, Hc, Wc).  ``pe_max`` /
    ``depth_scale``: those of the front-end call under test."""
    from gedepth_amd import hip
    lib = hip.lib()
    mean = (ctypes.c_double * 3)(*[float(np.float32(v)) for v in MEAN])
    std = (ctypes.c_double * 3)(*[float(np.float32(v)) for v in STD])
    ones = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    H, W = bgr.shape[:2]
    raw = torch.empty(5, Hc, Wc, device='cuda')
    norm = torch.empty_like(raw)
    hip.check(lib.ge_aug_load(hip.ptr(bgr), hip.ptr(pe), hip.ptr(raw), H, W, top, left, Hc, Wc, pe_max, hip.stream()), 'load')
    hip.check(lib.ge_aug_color_normalize(hip.ptr(raw), hip.ptr(norm), Hc, Wc, 0, 1.0, 1.0, vp(ones), vp(mean), vp(std), depth_scale, 1,
                                         hip.stream()), 'normalize')
    views = []
    for flip in (0, 1):
        ref = torch.empty_like(raw)
        hip.check(lib.ge_aug_window(hip.ptr(norm), hip.ptr(ref), 5, Hc, Wc, Hc, Wc, 0, 0, flip, 0.0, hip.stream()), 'window')
        views.append(ref)
    return views


def test_front_end_equals_training_pipeline_chain():
    """ge_infer_front == ge_aug_load -> ge_aug_color_normalize(color_on=0) -> ge_aug_window(flip), bit for bit, on every KITTI size."""
    for i, (H, W) in enumerate(KITTI_SIZES):
        rng = np.random.default_rng(10 + i)
        bgr = torch.from_numpy(_frame(20 + i, H, W)).cuda()
        pe_np = _plane(H, W) * rng.uniform(0.5, 2.0, (H, W)).astype(np.float32)
        pe_np[rng.random((H, W)) < 0.01] = 250.0                      # above the 200 m filter
        pe = torch.from_numpy(pe_np).cuda()
        got = _front(bgr.cpu().numpy(), pe_np)
        for flip, ref in enumerate(_chain(bgr, pe, H - 352, int((W - 1216) / 2), 352, 1216)):
            assert torch.equal(got[flip], ref), ((H, W), flip)
        assert torch.equal(got[1], got[0].flip(-1))


def test_tta_merge_bit_exact():
    from gedepth_amd import kernels as K
    g = torch.Generator(device='cuda').manual_seed(5)
    p = torch.rand(2, 1, 352, 1216, device='cuda', generator=g) * 80.0
    assert torch.equal(K.tta_merge(p), (p[0] + p[1].flip(-1)) / 2)


def test_engine_vs_aug_test_and_oracle(vanilla):
    from gedepth_amd.depth.apis import inference_depther
    from oracle import gedepth_oracle as O
    model = vanilla
    path, batch, ref = _host_route(model)
    out = inference_depther(model, path, graph=False)
    assert isinstance(out, list) and len(out) == 1
    got = out[0]
    assert got.shape == (1, 352, 1216) and got.dtype == np.float32
    mx, mean = _rel(got, ref)
    print(f'\n[engine vs aug_test] max rel {mx:.2e} mean {mean:.2e}')
    assert mx <= 2e-4 and mean <= 1e-5, (mx, mean)
    P = {k: (v.detach().float() if v.is_floating_point() else v.detach()).cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        oref = O.aug_test([t.float() for t in batch['img']], batch['img_metas'], P, dict(O.SWIN_T, adaptive=False))[0].numpy()
    mx, mean = _rel(got, oref)
    print(f'[engine vs oracle.aug_test] max rel {mx:.2e} mean {mean:.2e}')
    assert mx <= 2e-4 and mean <= 1e-5, (mx, mean)


def test_graph_replay(vanilla):
    from gedepth_amd.depth.apis import inference_depther
    model = vanilla
    frames = [_frame(s) for s in (31, 32, 33)]
    pe = _plane(375, 1242)
    eager = [inference_depther(model, f, pe=pe, graph=False)[0] for f in frames]
    eng = model._ge_inferencers[False]
    eng.reset()
    for _ in range(3):
        inference_depther(model, _frame(30), pe=pe)                 # two eager calls, then the capture
    assert eng.captures == 1
    graphed = [inference_depther(model, f, pe=pe)[0] for f in frames]
    same = all(np.array_equal(a, b) for a, b in zip(graphed, eager))
    print(f'\n[graph replay] bit-identical to eager: {same}')
    for a, b in zip(graphed, eager):
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
    assert not np.array_equal(graphed[0], graphed[1])              # a stale static buffer would repeat a map
    a = inference_depther(model, _frame(34, 375, 1242), pe=pe)[0]
    b = inference_depther(model, _frame(35, 370, 1224), pe=_plane(370, 1224))[0]
    assert eng.captures == 1 and a.shape == b.shape == (1, 352, 1216) and np.isfinite(b).all()


def _write_calib(d):
    from gedepth_amd.depth.datasets.kitti import _P_RECT
    cam = [f'line{i}: 0' for i in range(26)]
    cam[8] = 'R_rect_00: 9.999239e-01 9.837760e-03 -7.445048e-03 -9.869795e-03 9.999421e-01 -4.278459e-03 7.402527e-03 4.351614e-03 9.999631e-01'
    cam[25] = 'P_rect_02: ' + ' '.join(repr(v) for row in _P_RECT['2011_09_26'] for v in row)
    velo = ['calib_time: 0',
            'R: 7.533745e-03 -9.999714e-01 -6.166020e-04 1.480249e-02 7.280733e-04 -9.998902e-01 9.998621e-01 7.523790e-03 1.480755e-02',
            'T: -4.069766e-03 -7.631618e-02 -2.717806e-01']
    paths = (os.path.join(d, 'calib_cam_to_cam.txt'), os.path.join(d, 'calib_velo_to_cam.txt'))
    for p, lines in zip(paths, (cam, velo)):
        with open(p, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return paths


def test_ground_depth_sources(vanilla, toy, tmp_path):
    from gedepth_amd import kernels as K
    from gedepth_amd.depth.apis import inference_depther
    from gedepth_amd.depth.datasets.gpu_pipeline import read_kitti_calibration
    model = vanilla
    calib = _write_calib(str(tmp_path))
    P2, R0, Tr = read_kitti_calibration(*calib)
    A = P2 @ R0 @ Tr
    Rinv = np.linalg.inv(A[:3, :3])
    RT = Rinv @ A[:3, 3]
    _, pe = K.ground_plane(Rinv[2], float(RT[2] - 1.65), 375, 1242, want_f64=False)
    frame = _frame(40)
    a = inference_depther(model, frame, calib=calib, graph=False)[0]
    b = inference_depther(model, frame, pe=pe, graph=False)[0]
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), np.abs(a - b).max()
    root, _ = toy
    path, _, _ = _host_route(model)
    npy = np.load(os.path.join(root, 'input', '2011_09_26', 'pe', 'pe_165.npy'))
    a = inference_depther(model, path, graph=False)[0]
    b = inference_depther(model, path, pe=npy, graph=False)[0]
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), np.abs(a - b).max()


def test_adaptive_config_vs_aug_test(toy):
    from gedepth_amd.depth.apis import inference_depther
    model = _model('depthformer_swint_a.py', *toy)
    path, _, ref = _host_route(model)
    got = inference_depther(model, path)[0]
    mx, mean = _rel(got, ref)
    print(f'\n[adaptive engine vs aug_test] max rel {mx:.2e} mean {mean:.2e}')
    assert mx <= 2e-4 and mean <= 1e-5, (mx, mean)


def test_bf16_engine(vanilla):
    from gedepth_amd.depth.apis import inference_depther
    model = vanilla
    frame, pe = _frame(50), _plane(375, 1242)
    ref = inference_depther(model, frame, pe=pe, graph=False)[0]
    saved = [(m, m.kernel_variant) for m in model.modules() if hasattr(m, 'kernel_variant')]
    for m, _ in saved:
        m.kernel_variant = 0
    try:
        for _ in range(3):
            got = inference_depther(model, frame, pe=pe, bf16=True)[0]
    finally:
        for m, v in saved:
            m.kernel_variant = v
    head = model.decode_head
    assert np.isfinite(got).all() and got.min() >= head.min_depth and got.max() <= head.max_depth
    _, mean = _rel(got, ref)
    print(f'\n[bf16 engine vs fp32 engine] mean rel {mean:.2e}; captures {model._ge_inferencers[True].captures}')
    assert mean <= 3e-2, mean


def test_no_flip_config_vs_simple_test(toy):
    from gedepth_amd.depth.apis import inference_depther
    model = _model('depthformer_swint_v.py', *toy, flip=False)
    path, batch, ref = _host_route(model)
    assert len(batch['img']) == 1
    got = inference_depther(model, path, graph=False)[0]
    assert model._ge_inferencers[False].static_in.shape[0] == 1
    mx, mean = _rel(got, ref)
    print(f'\n[no-flip engine vs simple_test] max rel {mx:.2e} mean {mean:.2e}')
    assert mx <= 2e-4 and mean <= 1e-5, (mx, mean)


def test_checkpoint_round_trip(vanilla, tmp_path):
    from gedepth_amd.depth.apis import inference_depther, init_depther
    from gedepth_amd.mmrt.checkpoint import save_checkpoint
    ckpt = str(tmp_path / 'model.pth')
    save_checkpoint(vanilla, ckpt)
    loaded = _exact_variants(init_depther(os.path.join(CFG, 'depthformer_swint_v.py'), ckpt, device='cuda:0'))
    assert not loaded.training and loaded.cfg.model.pretrained is None
    frame, pe = _frame(60), _plane(375, 1242)
    a = inference_depther(loaded, frame, pe=pe, graph=False)[0]
    b = inference_depther(vanilla, frame, pe=pe, graph=False)[0]
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), np.abs(a - b).max()


def test_pinned_upload_keeps_three_arrays_apart_without_synchronising():
    """``PinnedUpload`` alone, one instance: an array, a second of another dtype that fits in the first one's bytes (the same pinned
    buffer, rewritten by the host), a third that makes the buffer grow; nothing synchronises in between.  After one synchronisation at
    the end every device tensor holds its source's bytes: no later host write reached a buffer an earlier copy still read."""
    from gedepth_amd.depth.utils.pinned import PinnedUpload
    rng = np.random.default_rng(7)
    sources = [rng.integers(0, 256, (3, 5, 3), dtype=np.uint8), rng.integers(0, 65536, (2, 7), dtype=np.uint16),
               rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)]
    assert sources[1].nbytes <= sources[0].nbytes < sources[2].nbytes
    upload, sent, buffers = PinnedUpload(), [], []
    for a in sources:
        sent.append(upload(a, torch.device('cuda')))
        buffers.append(upload.buffer)
    assert buffers[0] is buffers[1] and buffers[0].numel() == sources[0].nbytes and buffers[0].is_pinned()
    assert buffers[2] is not buffers[0] and buffers[2].numel() == sources[2].nbytes and buffers[2].is_pinned()
    torch.cuda.synchronize()
    for a, t in zip(sources, sent):
        assert t.is_cuda and tuple(t.shape) == a.shape and t.element_size() == a.itemsize
        assert t.cpu().view(torch.uint8).numpy().tobytes() == a.tobytes(), (a.shape, a.dtype)
    assert sent[1].dtype == torch.uint16 and sent[0].dtype == sent[2].dtype == torch.uint8

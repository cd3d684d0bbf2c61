"""The datasets' device-evaluation methods on the MI355X against the single-frame kernel wrappers, byte for byte.

``KITTIDataset.pre_eval_device*`` and ``DDADDataset.pre_eval_device*`` reach the batched entry points for any number of frames, one
included, so "the batch form equals the one-frame form" compares an entry point with itself.  The comparison that stays independent:
``kernels.depth_metric_sums``, ``depth_metric_sums_strata``, ``error_accumulate``, ``error_image`` and ``depth_metric_sums_resized`` still
call the single-frame entry points, and every dataset method must give their bits on the same prediction and the same ground truth.

Shapes: the KITTI protocol fixes the map at 352 x 1216; three images of two frame sizes, so ``top`` and ``left`` differ inside a batch, and
F = 4 slots for n = 3 images.  DDAD: 12 x 20 maps, ground truths of two sizes, so ``pre_eval_device_batch`` splits the batch in runs."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import memguard
import test_inference_gpu as TI
from toy_kitti import make_toy_kitti

pytestmark = pytest.mark.gpu
SIZES = ((375, 1242), (370, 1224), (375, 1242))


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ KITTI
@pytest.fixture(scope='module')
def kitti(tmp_path_factory):
    """The toy split, its inputs on the device and the single-frame wrappers' results on them: computed once, left unchanged."""
    from gedepth_amd import kernels as K
    from gedepth_amd.depth.core import StrataSpec
    from gedepth_amd.depth.datasets.kitti import KITTIDataset
    root = str(tmp_path_factory.mktemp('kitti_reduce'))
    rng = np.random.default_rng(5)
    ds = KITTIDataset.__new__(KITTIDataset)
    ds.ann_dir, ds.img_infos = root, []
    ds.depth_scale, ds.garg_crop, ds.eigen_crop, ds.min_depth, ds.max_depth = 256, True, False, 1e-3, 80
    for k, (H, W) in enumerate(SIZES):
        depth = np.where(rng.random((H, W)) < 0.05, rng.uniform(1.0, 80.0, (H, W)), 0.0)
        Image.fromarray((depth * 256).astype(np.uint16)).save(os.path.join(root, f'{k}.png'))
        ds.img_infos.append(dict(filename=f'{k}.png', ann=dict(depth_map=f'{k}.png')))
    t = dict(ds=ds, spec=StrataSpec(), rect=ds.eval_rect(352, 1216), limits=(ds.depth_scale, ds.min_depth, ds.max_depth))
    t['preds'] = torch.from_numpy(rng.uniform(1.0, 80.0, (4, 1, 352, 1216)).astype(np.float32)).cuda()      # F = 4 slots, three images
    t['gts'] = [torch.from_numpy(ds.gt_raw(k).copy()).cuda() for k in range(3)]
    t['offsets'] = [(H - 352, int((W - 1216) / 2)) for H, W in SIZES]
    t['grounds'] = [torch.from_numpy(TI._plane(H, W)).cuda() for H, W in SIZES]
    t['frames'] = [(torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda(), top, left)
                   for (H, W), (top, left) in zip(SIZES, t['offsets'])]
    t['sums'] = torch.zeros(3, 10, device='cuda', dtype=torch.float64)
    t['strata'] = torch.zeros(3, t['spec'].count, 10, device='cuda', dtype=torch.float64)
    t['pictures'] = []
    for k, (top, left) in enumerate(t['offsets']):
        args = (t['preds'][k], t['gts'][k], top, left, t['rect'], *t['limits'])
        K.depth_metric_sums(*args, t['sums'][k])
        K.depth_metric_sums_strata(*args, t['strata'][k], t['spec'].edges, t['grounds'][k], t['spec'].ground_tol)
        t['pictures'].append(K.error_image(t['preds'][k], t['gts'][k], t['frames'][k][0], top, left, t['rect'], *t['limits'], want_err=False)[0])
    counted = t['sums'][:, 0].cpu().numpy()
    assert (counted > 1000).all() and np.array_equal(counted, t['strata'][:, :, 0].sum(1).cpu().numpy()), counted
    assert len(set(t['offsets'])) == 2
    return t


def _planes_after(t, images):
    """The planes after ``kernels.error_accumulate`` of these images, in this order."""
    from gedepth_amd import kernels as K
    s = torch.zeros(352, 1216, device='cuda', dtype=torch.float64)
    n = torch.zeros(352, 1216, device='cuda', dtype=torch.int32).view(torch.uint32)
    for k in images:
        K.error_accumulate(t['preds'][k], t['gts'][k], *t['offsets'][k], t['rect'], *t['limits'], s, n)
    return _bytes(s), _bytes(n.view(torch.int32))


def _errors(t, out_dir=None):
    from gedepth_amd.depth.core import ErrorMaps
    errors = ErrorMaps(out_dir)
    errors.begin('cuda', t['rect'])
    return errors


def _planes_of(errors):
    return _bytes(errors.device_sum), _bytes(errors.device_count.view(torch.int32))


def test_plain_rows_are_those_of_the_single_frame_wrapper(kitti):
    t, ds = kitti, kitti['ds']
    one = torch.zeros(3, 10, device='cuda', dtype=torch.float64)
    for k in range(3):
        ds.pre_eval_device(t['preds'][k], k, one[k])
    assert _bytes(one) == _bytes(t['sums'])
    rows = torch.zeros(3, 10, device='cuda', dtype=torch.float64)
    ds.pre_eval_device_batch(t['preds'], [0, 1, 2], rows)
    assert _bytes(rows) == _bytes(t['sums'])


def test_strata_rows_are_those_of_the_single_frame_wrapper(kitti):
    t, ds, spec = kitti, kitti['ds'], kitti['spec']
    one, one_sums = torch.zeros_like(t['strata']), torch.zeros_like(t['sums'])
    for k in range(3):
        ds.pre_eval_device_strata(t['preds'][k], k, one[k], spec, t['grounds'][k], sums_row=one_sums[k])
    assert _bytes(one) == _bytes(t['strata']) and _bytes(one_sums) == _bytes(t['sums'])
    rows, sums = torch.zeros_like(t['strata']), torch.zeros_like(t['sums'])
    ds.pre_eval_device_strata_batch(t['preds'], [0, 1, 2], rows, spec, t['grounds'], sums_rows=sums)
    assert _bytes(rows) == _bytes(t['strata']) and _bytes(sums) == _bytes(t['sums'])
    alone = torch.zeros_like(t['strata'])
    ds.pre_eval_device_strata_batch(t['preds'], [0, 1, 2], alone, spec, t['grounds'])              # without the plain call
    assert _bytes(alone) == _bytes(t['strata'])


def test_error_planes_are_those_of_the_single_frame_wrapper(kitti):
    t, ds = kitti, kitti['ds']
    errors = _errors(t)
    for k in range(3):
        assert ds.pre_eval_device_errors(t['preds'][k], k, errors, t['frames'][k]) is None         # no out_dir, no picture
    assert errors.frames == 3 and _planes_of(errors) == _planes_after(t, [0, 1, 2])
    errors, sums = _errors(t), torch.zeros_like(t['sums'])
    ds.pre_eval_device_errors_batch(t['preds'], [0, 1, 2], errors, t['frames'], sums_rows=sums, count=2)
    assert errors.frames == 2 and _planes_of(errors) == _planes_after(t, [0, 1])                   # the third image stays out
    assert _planes_of(errors) != _planes_after(t, [0, 1, 2])
    assert _bytes(sums) == _bytes(t['sums'])                                                        # but its metric row is written


def test_error_pictures_are_those_of_the_single_frame_wrapper(kitti, tmp_path):
    t, ds = kitti, kitti['ds']
    errors = _errors(t, str(tmp_path))
    for k in range(3):
        got = ds.pre_eval_device_errors(t['preds'][k], k, errors, t['frames'][k])
        assert tuple(got.shape) == (352, 1216, 3) and _bytes(got) == _bytes(t['pictures'][k]), k
    got = ds.pre_eval_device_errors_batch(t['preds'], [0, 1, 2], errors, t['frames'])
    assert tuple(got.shape) == (3, 352, 1216, 3) and all(_bytes(got[k]) == _bytes(t['pictures'][k]) for k in range(3))
    assert errors.frames == 6 and len({_bytes(p) for p in t['pictures']}) == 3
    with pytest.raises(ValueError, match='is not its ground truth'):
        ds.pre_eval_device_errors(t['preds'][1], 1, errors, t['frames'][0])                        # another size's frame


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
def test_one_frame_calls_launch_the_batched_entry_points_inside_their_buffers(kitti, monkeypatch, tmp_path, poison):
    from gedepth_amd import batch_kernels, error_kernels, hip, strata_kernels
    t, ds, spec, k = kitti, kitti['ds'], kitti['spec'], 1
    guard = memguard.Guard(poison)
    monkeypatch.setattr(batch_kernels, '_WS', {})                     # a workspace cached by an earlier test would bypass the frames
    monkeypatch.setattr(strata_kernels, '_WS_BATCH', {})
    guard.install(monkeypatch, [batch_kernels, strata_kernels, error_kernels], binding=hip, frame_copies_on='cuda')     # the upload is framed too
    pred, ground = guard.framed(t['preds'][k]), guard.framed(t['grounds'][k])
    frame = (guard.framed(t['frames'][k][0]),) + t['frames'][k][1:]
    errors = _errors(t, str(tmp_path))
    errors.device_sum = guard.framed(errors.device_sum)
    errors.device_count = guard.framed(errors.device_count.view(torch.int32)).view(torch.uint32)
    sums = guard.proxy.empty(3, 10, device='cuda', dtype=torch.float64)
    rows = guard.proxy.empty(3, spec.count, 10, device='cuda', dtype=torch.float64)
    pics = guard.proxy.empty(3, 352, 1216, 3, device='cuda', dtype=torch.uint8)
    calls = []
    ds.pre_eval_device(pred, k, sums[1])
    calls.append(list(guard.launched))
    del guard.launched[:]
    ds.pre_eval_device_strata(pred, k, rows[1], spec, ground, sums_row=sums[1])
    calls.append(list(guard.launched))
    del guard.launched[:]
    got = ds.pre_eval_device_errors(pred, k, errors, frame, pics[1], sums_row=sums[1], strata=spec, rows=rows[1], ground=ground)
    calls.append(list(guard.launched))
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()              # red zones of the prediction, the upload, the plane, the frame, the workspaces, the rows, planes and pictures
    assert calls == [['ge_depth_metrics_batch'], ['ge_depth_metrics_batch', 'ge_depth_metrics_strata_batch'],
                     ['ge_depth_metrics_batch', 'ge_depth_metrics_strata_batch', 'ge_error_accumulate_batch', 'ge_error_image_batch']]
    for buf in (sums, rows, pics):
        stay = memguard.poisoned(buf, poison).flatten(1).cpu().numpy()
        assert stay[0].all() and stay[2].all() and not stay[1].all(), 'the blocks beside the written one must stay poisoned'
    assert got.data_ptr() == pics[1].data_ptr()
    assert _bytes(sums[1]) == _bytes(t['sums'][k]) and _bytes(rows[1]) == _bytes(t['strata'][k]) and _bytes(pics[1]) == _bytes(t['pictures'][k])
    assert errors.frames == 1 and _planes_of(errors) == _planes_after(t, [k])


# ------------------------------------------------------------------------------------------------ DDAD
def test_ddad_rows_are_those_of_the_single_frame_wrapper(tmp_path):
    from gedepth_amd import kernels as K
    from gedepth_amd.depth.datasets.ddad import DDADDataset
    rng = np.random.default_rng(9)
    ds = DDADDataset.__new__(DDADDataset)
    ds.min_depth, ds.max_depth, ds.img_infos = 1e-3, 200, []
    for k, shape in enumerate(((24, 40), (24, 40), (31, 47))):         # a run of two, then another size
        gt = np.where(rng.random(shape) < 0.5, rng.uniform(1.0, 150.0, shape), 0.0).astype(np.float32)
        np.savez(str(tmp_path / f'{k}.npz'), depth=gt)
        ds.img_infos.append(dict(filename=f'{k}.png', ann=dict(depth_map=str(tmp_path / f'{k}.npz'))))
    preds = torch.from_numpy(rng.uniform(1.0, 150.0, (4, 1, 12, 20)).astype(np.float32)).cuda()
    want = torch.zeros(3, 10, device='cuda', dtype=torch.float64)
    for k in range(3):
        K.depth_metric_sums_resized(preds[k], torch.from_numpy(ds.gt_raw(k)).cuda(), ds.min_depth, ds.max_depth, want[k])
    assert (want[:, 0] > 100).all()
    one = torch.zeros_like(want)
    for k in range(3):
        ds.pre_eval_device(preds[k], k, one[k])
    assert _bytes(one) == _bytes(want)
    rows = torch.zeros_like(want)
    ds.pre_eval_device_batch(preds, [0, 1, 2], rows)
    assert _bytes(rows) == _bytes(want)


# ------------------------------------------------------------------------------------------------ the engines' one name
def test_every_engine_answers_to_the_plural_names(tmp_path):
    from gedepth_amd.depth.apis.batch_inference import BatchDepthInferencer
    from gedepth_amd.depth.apis.inference import engine_for
    root = str(tmp_path)
    model = TI._model('depthformer_swint_v.py', root, make_toy_kitti(root, seed=3))
    eng = engine_for(model)
    assert eng.last_frames is None and eng.last_ground_depths is None
    pe = TI._plane(375, 1242)
    eng(TI._frame(41), pe=pe, graph=False, to_host=False)
    assert len(eng.last_frame) == 3 and eng.last_frames == [eng.last_frame]
    assert len(eng.last_ground_depths) == 1 and eng.last_ground_depths[0] is eng.last_ground_depth
    batched = BatchDepthInferencer(model, 2)                         # no forward: the loop tests of strata and errors read its lists
    batched.last_frames, batched.last_ground_depths = [eng.last_frame], [eng.last_ground_depth]     # what ``batch`` assigns: plain attributes
    assert batched.last_frames == eng.last_frames
    batched.reset()
    assert batched.last_frames is None and batched.last_ground_depths is None and batched.last_n == 0

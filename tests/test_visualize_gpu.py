"""Depth colorization on MI355X: ge_depth_colorize bit-exact to the numpy restatement of the reference's colorize, show_result's image,
and tools/test.py's --show-dir / --format-only / --out / --launcher pytorch end to end on the toy KITTI tree."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gedepth_amd import kernels                                              # noqa: E402
from gedepth_amd.depth.apis.test import replace_str, single_gpu_test         # noqa: E402
from gedepth_amd.depth.utils import colorize                                 # noqa: E402
from gedepth_amd.depth.utils.color_depth import colormap_table              # noqa: E402
from test_visualize_cpu import CASES, case_value, mpl_colorize, table_colorize   # noqa: E402
from toy_kitti import make_toy_kitti                                         # noqa: E402

pytestmark = pytest.mark.gpu
CONFIG = os.path.join(ROOT, 'configs', 'depthformer', 'depthformer_swint_v.py')
SHAPES = [(1, 352, 1216), (1, 384, 640), (37, 53), (3, 40, 66)]             # (37, 53): n % 4 == 1


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


def _expect(value, cmap, vmin, vmax):
    with np.errstate(all='ignore'):
        return table_colorize(value, colormap_table(cmap), vmin, vmax)


@pytest.mark.parametrize('name,transform,vmin,vmax', CASES, ids=[c[0] for c in CASES])
def test_colorize_bit_exact(name, transform, vmin, vmax):
    cmaps = ['magma_r'] + (['jet', 'magma'] if _have_matplotlib() else [])
    for si, shape in enumerate(SHAPES):
        value = case_value(transform, shape, seed=si)
        for cmap in cmaps:
            ref = _expect(value, cmap, vmin, vmax)
            if cmap != 'magma_r':
                with np.errstate(all='ignore'):
                    assert np.array_equal(ref, mpl_colorize(value, cmap, vmin, vmax))
            got = colorize(value, cmap, vmin, vmax)                                     # numpy in, numpy out
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == value.shape + (3,)
            assert np.array_equal(got, ref), (shape, cmap, int((got != ref).any(-1).sum()))
            dev = colorize(torch.from_numpy(value).cuda(), cmap, vmin, vmax)             # CUDA in, CUDA out
            assert dev.is_cuda and dev.dtype == torch.uint8
            assert np.array_equal(dev.cpu().numpy(), ref), (shape, cmap)
    # a non-contiguous CUDA tensor, and a contiguous one that is not 16-byte aligned (the kernel's scalar-load path)
    value = case_value(transform, (64, 2 * 97), seed=7)
    strided = torch.from_numpy(value).cuda()[:, ::2]
    assert not strided.is_contiguous()
    assert np.array_equal(colorize(strided, 'magma_r', vmin, vmax).cpu().numpy(), _expect(np.ascontiguousarray(value[:, ::2]), 'magma_r',
                                                                                          vmin, vmax))
    flat = torch.from_numpy(value).cuda().view(-1)[1:]
    assert flat.is_contiguous() and flat.data_ptr() % 16 != 0
    lut = torch.from_numpy(colormap_table('magma_r')).cuda()
    got = kernels.depth_colorize(flat, vmin, vmax, lut).cpu().numpy()
    assert np.array_equal(got, _expect(value.reshape(-1)[1:], 'magma_r', vmin, vmax))


def _vanilla_model():
    from gedepth_amd.depth.models import build_depther
    from gedepth_amd.mmrt.config import Config
    cfg = Config.fromfile(CONFIG)
    cfg.model.pretrained = None
    torch.manual_seed(0)
    model = build_depther(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.init_weights()
    return cfg, model


def test_show_result_png(tmp_path):
    from PIL import Image
    _, model = _vanilla_model()
    model = model.cuda().eval()
    head = model.decode_head
    depth = case_value(None, (1, 352, 1216), seed=3)
    out = tmp_path / 'x' / 'y' / 'frame.png'
    assert model.show_result('frame.png', [depth], out_file=str(out)) is None
    rgb = np.asarray(Image.open(out).convert('RGB'))
    expect_bgr = _expect(depth, 'magma_r', head.min_depth, head.max_depth)[0]
    assert rgb.shape == (352, 1216, 3) and np.array_equal(rgb, expect_bgr[..., ::-1])
    if _have_matplotlib():
        with np.errstate(all='ignore'):
            assert np.array_equal(rgb, mpl_colorize(depth, 'magma_r', head.min_depth, head.max_depth)[0][..., ::-1])
    # the list inference_depther returns (one (1, 352, 1216) array per frame) is a valid ``result`` as it is
    from gedepth_amd.depth.apis import inference_depther
    from gedepth_amd.mmrt.config import Config
    root = str(tmp_path / 'kitti')
    split = make_toy_kitti(root, frames=1)
    model.cfg = Config.fromfile(CONFIG)
    model.cfg.data.test.data_root, model.cfg.data.test.split = root, split
    img = os.path.join(root, 'input', '2011_09_26', '2011_09_26_drive_0001_sync', 'image_02', 'data', '0000000005.png')
    result = inference_depther(model, img)
    model.show_result(img, result, out_file=str(tmp_path / 'inf.png'))
    got = np.asarray(Image.open(tmp_path / 'inf.png').convert('RGB'))
    assert np.array_equal(got, _expect(result[0], 'magma_r', head.min_depth, head.max_depth)[0][..., ::-1])


@pytest.fixture(scope='module')
def toy_run(tmp_path_factory):
    from gedepth_amd.mmrt.checkpoint import save_checkpoint
    tmp = tmp_path_factory.mktemp('vis')
    root = str(tmp / 'kitti')
    split = make_toy_kitti(root)
    cfg, model = _vanilla_model()
    ckpt = str(tmp / 'model.pth')
    save_checkpoint(model, ckpt)                       # every subprocess evaluates the same weights
    for part in ('train', 'val', 'test'):
        cfg.data[part].data_root, cfg.data[part].split = root, split
    opts = ['--options', f'data.test.data_root={root}', f'data.test.split={split}', 'data.workers_per_gpu=0']
    return dict(tmp=tmp, root=root, split=split, cfg=cfg, model=model, ckpt=ckpt, opts=opts)


def _run(cmd, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    r = subprocess.run(['timeout', '-k', '10', str(timeout)] + cmd, env=env, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        print('---- stdout ----\n' + r.stdout[-6000:] + '\n---- stderr ----\n' + r.stderr[-6000:])
    assert r.returncode == 0, r.returncode
    return r.stdout


def _test_py(t, *args):
    return _run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), CONFIG, t['ckpt']] + list(args) + t['opts'])


def _names(t):
    from gedepth_amd.depth.datasets import build_dataset
    ds = build_dataset(t['cfg'].data.test, dict(test_mode=True))
    return ds, [info['filename'] for info in ds.img_infos]


def test_cli_show_dir_out_and_format_only(toy_run):
    from PIL import Image
    t = toy_run
    ds, names = _names(t)
    assert len(names) == 4
    # PNGs and maps of the same run: bit-identical
    maps_pkl, show = str(t['tmp'] / 'maps.pkl'), t['tmp'] / 'show'
    _test_py(t, '--out', maps_pkl, '--show-dir', str(show))
    with open(maps_pkl, 'rb') as fh:
        maps = pickle.load(fh)
    assert len(maps) == 4 and all(m.shape == (1, 352, 1216) and m.dtype == np.float32 for m in maps)
    head = t['model'].decode_head
    assert sorted(os.listdir(show)) == sorted(replace_str(n) for n in names)
    for n, m in zip(names, maps):
        rgb = np.asarray(Image.open(show / replace_str(n)).convert('RGB'))
        assert np.array_equal(rgb, _expect(m, 'magma_r', head.min_depth, head.max_depth)[0][..., ::-1]), n
    # with --eval: the summary, and the same pictures.  The forward is not bit-reproducible from process to process (float atomics),
    # so a pixel whose depth lies within that noise of a colour-bin edge may take the neighbouring colour
    show_eval = t['tmp'] / 'show_eval'
    out = _test_py(t, '--show-dir', str(show_eval), '--eval', 'x')
    assert 'Summary' in out and 'abs_rel' in out
    assert sorted(os.listdir(show_eval)) == sorted(replace_str(n) for n in names)
    for n in names:
        a = np.asarray(Image.open(show / replace_str(n)).convert('RGB')).astype(np.int32)
        b = np.asarray(Image.open(show_eval / replace_str(n)).convert('RGB')).astype(np.int32)
        differ = (a != b).any(-1)
        assert differ.mean() <= 1e-3 and np.abs(a - b).max() <= 8, (n, differ.mean(), np.abs(a - b).max())
    raw = t['tmp'] / 'raw'
    _test_py(t, '--format-only', '--show-dir', str(raw))
    model = t['model'].cuda().eval()
    from gedepth_amd.depth.datasets import build_dataloader
    plain = single_gpu_test(model, build_dataloader(ds, 1, 0, dist=False, shuffle=False))
    for n, m in zip(names, plain):
        saved = np.load(raw / (n[:-4] + '.npy'))
        assert saved.shape == m.shape and saved.dtype == np.float32
        assert np.abs(saved - m).max() <= 1e-6 * np.abs(m).max(), n


def _dist_cmd(t, world, port, *args):
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}', '--master-addr', '127.0.0.1',
            '--master-port', str(port), os.path.join(ROOT, 'tools', 'test.py'), CONFIG, t['ckpt'], '--launcher', 'pytorch'] + list(args) + \
        t['opts']


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and np.abs(x - y).max() <= 1e-6 * np.abs(y).max()
        else:
            assert np.allclose(np.asarray(x, np.float64), np.asarray(y, np.float64), rtol=1e-5, atol=1e-7, equal_nan=True)


def test_cli_launcher_pytorch_single_rank(toy_run):
    t = toy_run
    single, dist1 = str(t['tmp'] / 'single.pkl'), str(t['tmp'] / 'dist1.pkl')
    _test_py(t, '--eval', 'x', '--out', single)
    out = _run(_dist_cmd(t, 1, 29651, '--eval', 'x', '--out', dist1))
    assert 'Summary' in out
    with open(single, 'rb') as fh_a, open(dist1, 'rb') as fh_b:
        _same_results(pickle.load(fh_b), pickle.load(fh_a))
    # tools/dist_test.sh: the same (it adds --eval abs_rel, as the reference's does)
    sh = str(t['tmp'] / 'sh.pkl')
    _run(['bash', os.path.join(ROOT, 'tools', 'dist_test.sh'), CONFIG, t['ckpt'], '1', '--out', sh] + t['opts'])
    with open(sh, 'rb') as fh_a, open(single, 'rb') as fh_b:
        _same_results(pickle.load(fh_a), pickle.load(fh_b))


def test_cli_launcher_pytorch_world2(toy_run):
    """Two ranks over RCCL: the same maps in dataset order, and every rank writes its own shard's images.  Skipped on a 1-GPU node."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs >= 2 GPUs on the node')
    t = toy_run
    single, dist2 = str(t['tmp'] / 'single_maps.pkl'), str(t['tmp'] / 'dist2.pkl')
    _test_py(t, '--out', single)
    show = t['tmp'] / 'show2'
    _run(_dist_cmd(t, 2, 29653, '--out', dist2, '--show-dir', str(show)))
    with open(single, 'rb') as fh_a, open(dist2, 'rb') as fh_b:
        _same_results(pickle.load(fh_b), pickle.load(fh_a))
    _, names = _names(t)
    assert sorted(os.listdir(show)) == sorted(replace_str(n) for n in names)

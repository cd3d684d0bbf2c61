"""Depth colorization, show_result and the tools/test.py output flags without a GPU: the committed colormap table, the numpy
restatement of the reference's colorize (the tables and arithmetic the gfx950 kernel is held to in test_visualize_gpu.py), the host half
of the kernel contract, argument errors of the CLI, show_result's raw-map path and replace_str."""
import os
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gedepth_amd import hip, kernels                                         # noqa: E402
from gedepth_amd.depth.apis.test import replace_str                          # noqa: E402
from gedepth_amd.depth.models.depther.base import BaseDepther               # noqa: E402
from gedepth_amd.depth.utils.color_depth import colormap_table              # noqa: E402

CONFIG = os.path.join(ROOT, 'configs', 'depthformer', 'depthformer_swint_v.py')
F32 = np.float32


def _normalise(value, vmin, vmax):
    # the first lines of the reference's colorize (depth/utils/color_depth.py), verbatim
    vmin = value.min() if vmin is None else vmin
    vmax = value.max() if vmax is None else vmax
    if vmin != vmax:
        value = (value - vmin) / (vmax - vmin)  # vmin..vmax
    else:
        value = value * 0.
    return value


def mpl_colorize(value, cmap='magma_r', vmin=None, vmax=None):
    """The reference's colorize with matplotlib.cm.get_cmap -> matplotlib.colormaps (get_cmap is gone since 3.9)."""
    import matplotlib
    value = _normalise(value, vmin, vmax)
    value = matplotlib.colormaps[cmap](value, bytes=True)
    return value[..., :3][..., ::-1]


def table_colorize(value, table, vmin=None, vmax=None):
    """The same, with matplotlib's Colormap._get_rgba_and_mask restated in numpy over an (N + 3, 3) BGR table (no matplotlib needed)."""
    xa = np.array(_normalise(value, vmin, vmax), copy=True)
    N = table.shape[0] - 3
    xa *= N
    xa[xa == N] = N - 1
    under, over, bad = xa < 0, xa >= N, np.isnan(xa)
    with np.errstate(invalid='ignore'):
        idx = xa.astype(int)
    idx[under], idx[over], idx[bad] = N, N + 1, N + 2
    return table.take(idx, axis=0, mode='clip')


def contract_colorize(value, table, vmin=None, vmax=None):
    """What ge_depth_colorize computes (include/gedepth_hip.h), with kernels._colorize_bounds as the host half."""
    lo, hi, den, flags = kernels._colorize_bounds(vmin, vmax)
    lo, hi, den = F32(lo), F32(hi), F32(den)
    v = value.astype(F32)
    eq = bool(flags & hip.GE_COLORIZE_EQUAL)
    if flags & (hip.GE_COLORIZE_VMIN_DATA | hip.GE_COLORIZE_VMAX_DATA):
        lo = v.min() if flags & hip.GE_COLORIZE_VMIN_DATA else lo
        hi = v.max() if flags & hip.GE_COLORIZE_VMAX_DATA else hi
        eq, den = bool(lo == hi), F32(hi - lo)
    with np.errstate(all='ignore'):
        x = v * F32(0) if eq else (v - lo) / den
        xa = x * F32(table.shape[0] - 3)
    N = table.shape[0] - 3
    xa[xa == N] = N - 1
    idx = np.zeros(xa.shape, np.int64)
    ok = ~np.isnan(xa) & (xa >= 0) & (xa < N)
    idx[ok] = xa[ok].astype(np.int64)
    idx[np.isnan(xa)], idx[xa < 0], idx[xa >= N] = N + 2, N, N + 1
    return table[idx]


def adversarial(shape, seed, lo=1e-3, hi=80.0, finite=False):
    """float32 values on [lo - 5, hi + 10] with, first, the values where the index rules switch: exact bounds (as Python floats and as
    float32), their float32 neighbours, the zeros, negatives, values above vmax and (unless ``finite``) NaN and +-inf."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(lo - 5.0, hi + 10.0, int(np.prod(shape))).astype(F32)
    specials = []
    for b in (F32(lo), F32(hi), F32(0.3), F32(80.7), F32(5.0)):
        specials += [b, np.nextafter(b, F32(np.inf)), np.nextafter(b, F32(-np.inf))]
    specials += [F32(0.0), F32(-0.0), F32(-1e-30), F32(-1.0), F32(hi + 1e-3), F32(1e30), F32(-1e30), F32(40.0)]
    specials += [F32(lo) + F32(k) * (F32(hi) - F32(lo)) / F32(256) for k in range(0, 257, 16)]        # bin edges
    if not finite:
        specials += [F32(np.nan), F32(np.inf), F32(-np.inf)]
    specials = np.array(specials, F32)[:v.size]
    v[:specials.size] = specials
    v[-specials.size:] = specials[::-1]
    return v.reshape(shape)


# (name, value transform, vmin, vmax): every branch of the reference's normalisation under numpy 2's scalar rules
CASES = [
    ('python-bounds', None, 1e-3, 80.0),
    ('f32-bounds', None, F32(1e-3), F32(80.0)),
    ('mixed-f32-python', None, F32(0.1), 80.0),
    ('python-inexact', None, 0.3, 80.7),
    ('mixed-inexact', None, F32(0.3), 80.7),
    ('int-bounds', None, 0, 80),
    ('equal-bounds', None, 5.0, 5.0),
    ('equal-f32-python', None, F32(5.0), 5.0),
    ('none-none-nan', None, None, None),
    ('none-none-finite', 'finite', None, None),
    ('none-vmax', 'finite', None, 80.0),
    ('vmin-none', 'finite', 1e-3, None),
    ('none-none-inf', 'inf', None, None),
    ('none-none-constant', 'constant', None, None),
]


def case_value(transform, shape, seed):
    if transform == 'constant':
        return np.full(shape, F32(7.25))
    v = adversarial(shape, seed, finite=transform in ('finite', 'inf'))
    if transform == 'inf':
        v.reshape(-1)[3] = np.inf
    return v


def test_committed_magma_r_table_is_matplotlibs():
    matplotlib = pytest.importorskip('matplotlib')
    cm = matplotlib.colormaps['magma_r']
    rgba = np.concatenate([cm(np.arange(cm.N), bytes=True), cm(np.array([-1.0, 2.0, np.nan]), bytes=True)])
    table = colormap_table('magma_r')
    assert table.shape == (259, 3) and table.dtype == np.uint8
    assert np.array_equal(table, rgba[:, :3][:, ::-1])
    assert np.array_equal(table[256], table[0]) and np.array_equal(table[257], table[255]) and not table[258].any()
    for name in ('jet', 'magma'):
        cm = matplotlib.colormaps[name]
        ref = np.concatenate([cm(np.arange(cm.N), bytes=True), cm(np.array([-1.0, 2.0, np.nan]), bytes=True)])[:, :3][:, ::-1]
        assert np.array_equal(colormap_table(name), ref)


@pytest.mark.parametrize('name,transform,vmin,vmax', CASES, ids=[c[0] for c in CASES])
def test_restatements_match_matplotlib(name, transform, vmin, vmax):
    pytest.importorskip('matplotlib')
    value = case_value(transform, (1, 24, 40), seed=len(name))
    with np.errstate(all='ignore'):
        ref = mpl_colorize(value, 'magma_r', vmin, vmax)
        assert ref.shape == value.shape + (3,)
        table = colormap_table('magma_r')
        assert np.array_equal(table_colorize(value, table, vmin, vmax), ref)
        assert np.array_equal(contract_colorize(value, table, vmin, vmax), ref)
        for cmap in ('jet', 'magma'):
            assert np.array_equal(contract_colorize(value, colormap_table(cmap), vmin, vmax), mpl_colorize(value, cmap, vmin, vmax))


def test_colorize_bounds_follow_numpy_scalar_rules():
    lo, hi, den, flags = kernels._colorize_bounds(0.3, 80.7)
    assert flags == 0 and lo == float(F32(0.3)) and hi == float(F32(80.7)) and den == float(F32(80.7 - 0.3))
    assert den != float(F32(80.7) - F32(0.3))                                # Python bounds subtract in float64, not float32
    assert kernels._colorize_bounds(F32(0.3), 80.7)[2] == float(F32(80.7) - F32(0.3))
    assert kernels._colorize_bounds(3.0, 3)[3] == hip.GE_COLORIZE_EQUAL
    assert kernels._colorize_bounds(None, 2.0)[3] == hip.GE_COLORIZE_VMIN_DATA
    assert kernels._colorize_bounds(None, None)[3] == hip.GE_COLORIZE_VMIN_DATA | hip.GE_COLORIZE_VMAX_DATA


def test_cli_lists_new_flags_and_checks_arguments_first():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0
    for flag in ('--out', '--format-only', '--show', '--show-dir', '--eval-options', '--launcher', '--local_rank', '--gpu-collect',
                 '--tmpdir', '--eval', '--options', '--synthetic', '--flip-tta', '--bf16'):
        assert flag in out.stdout, flag
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    for args, msg in ((['--out', 'x.txt'], 'The output file must be a pkl file'),
                      (['--eval', 'x', '--format-only'], '--eval and --format-only cannot be both specified')):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), CONFIG] + args, capture_output=True, text=True,
                           env=env, timeout=300)
        assert r.returncode != 0 and 'ValueError' in r.stderr and msg in r.stderr, r.stderr[-2000:]
    assert os.path.isfile(os.path.join(ROOT, 'tools', 'dist_test.sh'))


def test_cli_dataset_route_needs_a_data_root(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), CONFIG, '--show-dir', str(tmp_path / 'd'), '--options',
                        f'data.test.data_root={tmp_path / "missing"}'], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and 'is not a directory' in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / 'd').exists()


def test_show_result_raw_map_paths(tmp_path):
    depther = types.SimpleNamespace()                  # the raw-map paths never read the model
    depth = np.random.default_rng(0).uniform(0, 80, (1, 6, 10)).astype(F32)
    result = [depth, np.zeros((1, 6, 10), F32)]
    out = tmp_path / 'a' / 'b.npy'
    assert BaseDepther.show_result(depther, 'unused.png', result, format_only=True, out_file=str(out)) is None
    saved = np.load(out)
    assert saved.dtype == np.float32 and np.array_equal(saved, depth)
    with pytest.warns(UserWarning, match='only result depth will be returned'):
        assert BaseDepther.show_result(depther, None, result) is depth
    with pytest.warns(UserWarning, match='only result depth will be returned'):
        assert BaseDepther.show_result(depther, None, result, format_only=True) is depth
    with warnings.catch_warnings():
        warnings.simplefilter('error')                 # show=True only warns (once per process), opens nothing, returns None
        try:
            ret = BaseDepther.show_result(depther, np.zeros((4, 4, 3), np.uint8), result, show=True)
        except UserWarning as w:
            assert 'no display' in str(w)
            ret = None
    assert ret is None


def test_replace_str_as_reference():
    assert replace_str('/abs/path/x.png') == 'abs/path/x.png'
    assert replace_str('2011_09_26/2011_09_26_drive_0001_sync/image_02/data/0000000005.png') == \
        '2011_09_26_2011_09_26_drive_0001_sync_image_02_data_0000000005.png'
    assert replace_str('x.png') == 'x.png'


def test_colorize_rejects_cpu_tensors():
    import torch
    from gedepth_amd.depth.utils import colorize
    with pytest.raises(RuntimeError, match='MI355X only'):
        colorize(torch.zeros(1, 4, 4))

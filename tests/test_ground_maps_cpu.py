"""The ground maps, the parts that need no GPU: the fifth header and its binding, argument validation of ``ge_ground_maps``, the torch
restatement (tests/ground_ref.py) on a hand-made case, and ``BaseDepther.show_ground``'s files."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ground_ref as G
from gedepth_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 10001


def _declared(name):
    header = open(os.path.join(ROOT, 'include', name)).read()
    return set(re.findall(r'\b(ge_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header, flags=re.S)))


def test_ground_header_parses_and_library_exports_it():
    assert list(hip.HEADERS.items())[-1] == ('GROUND_SIGNATURES', 'gedepth_ground.h') and len(hip.HEADERS) == 5
    declared = _declared('gedepth_ground.h')
    assert declared == set(hip.GROUND_SIGNATURES) == {'ge_ground_maps'}
    for other in (hip.SIGNATURES, hip.EVAL_SIGNATURES, hip.DDAD_SIGNATURES, hip.CLOUD_SIGNATURES):
        assert not set(hip.GROUND_SIGNATURES) & set(other)
    c = ctypes
    vp, i, f = c.c_void_p, c.c_int, c.c_float
    assert hip.GROUND_SIGNATURES['ge_ground_maps'] == (i, [vp, vp, vp, c.c_long, vp, f, f, i, vp, vp, i, i, i, i, i, vp])
    if not hip.is_built():
        pytest.fail(f'{hip.LIB_PATH} missing: run gedepth_amd/csrc/build.sh')
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), 'ge_ground_maps')
    fn = hip.lib().ge_ground_maps                                      # lib() has bound the fifth table too
    assert fn.restype is i and list(fn.argtypes) == hip.GROUND_SIGNATURES['ge_ground_maps'][1]


def test_training_header_is_unchanged_by_the_ground_entry_point():
    assert _declared('gedepth_hip.h') == set(hip.SIGNATURES) and len(hip.SIGNATURES) == 102
    assert hip.lib().ge_abi_version() == 7


def test_argument_validation_without_a_gpu():
    """Every check comes before a launch, so fake non-null pointers are never followed."""
    lib = hip.lib()
    p = 4096

    def run(logits=p, y=p, pe=p, height=None, maps=p, valid=p, V=2, h=12, w=20, H=24, W=40):
        return lib.ge_ground_maps(logits, y, pe, 5 * H * W, height, 200.0, 200.0, 1, maps, valid, V, h, w, H, W, None)
    for null in ('y', 'pe', 'maps', 'valid'):
        assert run(**{null: None}) == BAD_ARG, null
        assert run(logits=None, **{null: None}) == BAD_ARG, null      # the vanilla model's call
    for V in (3, 0, -1):
        assert run(V=V) == BAD_ARG, V
    for size in ('h', 'w', 'H', 'W'):
        assert run(**{size: 0}) == BAD_ARG and run(**{size: -4}) == BAD_ARG, size


def _hand_case():
    """2 x 6 output from 1 x 3 necks, flat logits (slope 0, so the offset is the ground depth itself up to rounding).  Ground depth per
    output column, view 0 / view 1 after mirroring: valid / valid, valid / negative, beyond 200 / valid, negative / beyond 200,
    valid / negative, negative / valid."""
    H, W = 2, 6
    v0 = torch.tensor([10.0, 20.0, 300.0, -5.0, 30.0, -1.0])
    v1 = torch.tensor([12.0, -3.0, 25.0, 400.0, -2.0, 40.0])
    img = torch.zeros(2, 5, H, W)
    img[0, 4] = v0.expand(H, W)
    img[1, 4] = v1.flip(0).expand(H, W)                               # view 1 is the mirrored frame
    img[:, 3] = torch.where((img[:, 4] > 0) & (img[:, 4] <= 200), img[:, 4], torch.zeros(())) / 200.0
    logits = torch.zeros(2, 11, 1, 3)
    y = torch.tensor([0.25, 0.5, 0.75]).view(1, 1, 1, 3).repeat(2, 1, 1, 1)
    y[1] += 0.125
    return img, logits, y, v0, v1


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_restatement_on_a_hand_made_case(dtype):
    img, logits, y, v0, v1 = _hand_case()
    views = G.per_view(logits, y, img, dtype=dtype)
    maps, valid = G.merge(views)
    assert maps.shape == (4, 2, 6) and maps.dtype == dtype and valid.dtype == torch.uint8
    assert valid.tolist() == [[2, 1, 1, 0, 1, 1]] * 2                  # 0, 1 and 2 views
    assert set(valid.unique().tolist()) == {0, 1, 2}
    gd = maps[2, 0].double()
    want = torch.tensor([11.0, 20.0, 25.0, 0.0, 30.0, 40.0], dtype=torch.float64)   # the mean, the one valid view (either), none
    assert torch.allclose(gd, want, rtol=1e-6, atol=0) and gd[3] == 0
    assert float(maps[3].abs().max()) <= 1e-6                          # flat logits: slope 0, up to the rounding of sum_c (c - 5) / 11
    b_y, b_t = views['y'][1].flip(-1), views['t'][1].flip(-1)
    assert torch.equal(maps[0], (views['y'][0] + b_y) * 0.5) and torch.equal(maps[1], (views['t'][0] + b_t) * 0.5)
    # the ground term is off * mask * y: zero where the view is invalid
    assert float(views['t'][0][0, 2]) == 0.0 and float(views['t'][0][0, 0]) == pytest.approx(10.0 * float(views['y'][0][0, 0]), rel=1e-6)


def test_restatement_single_view_equals_the_per_view_values():
    img, logits, y, _, _ = _hand_case()
    for v in (0, 1):
        views = G.per_view(logits[v:v + 1], y[v:v + 1], img[v:v + 1])
        maps, valid = G.merge(views)
        assert torch.equal(maps[0], views['y'][0]) and torch.equal(maps[1], views['t'][0]) and torch.equal(maps[3], views['deg'][0])
        assert torch.equal(valid, views['ok'][0].to(torch.uint8)) and set(valid.unique().tolist()) == {0, 1}
        assert torch.equal(maps[2], torch.where(views['ok'][0], views['off'][0], torch.zeros((), dtype=torch.float64)))
    two = G.per_view(logits, y, img)
    assert torch.equal(two['off'][1], G.per_view(logits[1:], y[1:], img[1:])['off'][0])      # the views do not mix before the merge


def test_restatement_vanilla_reads_the_normalised_channel():
    img, _, y, v0, v1 = _hand_case()
    maps, valid = G.ground_maps(None, y, img, dtype=torch.float32)
    assert valid.tolist() == [[2, 1, 1, 0, 1, 1]] * 2
    assert torch.equal(maps[3], torch.zeros(2, 6))
    assert torch.allclose(maps[2, 0], torch.tensor([11.0, 20.0, 25.0, 0.0, 30.0, 40.0]), rtol=1e-6)


def _depther():
    from gedepth_amd.depth.models.depther.base import BaseDepther
    return BaseDepther, types.SimpleNamespace(decode_head=types.SimpleNamespace(min_depth=1e-3, max_depth=80.0))


def _host_dict(slope=True):
    rng = np.random.default_rng(0)
    out = dict(depth=rng.uniform(1, 80, (1, 6, 10)).astype(np.float32), attention=rng.random((6, 10), dtype=np.float32),
               ground_term=rng.uniform(0, 40, (6, 10)).astype(np.float32), ground_depth=rng.uniform(0, 80, (6, 10)).astype(np.float32),
               valid=rng.integers(0, 3, (6, 10)).astype(np.uint8))
    if slope:
        out['slope_deg'] = rng.uniform(-5, 5, (6, 10)).astype(np.float32)
    return out


def test_show_ground_format_only_writes_one_npz(tmp_path):
    Base, depther = _depther()
    result = _host_dict()
    assert Base.show_ground(depther, result, str(tmp_path / 'sub' / 'frame.png'), format_only=True) is None
    assert sorted(os.listdir(tmp_path / 'sub')) == ['frame.npz']
    with np.load(tmp_path / 'sub' / 'frame.npz') as z:
        assert set(z.files) == set(result)
        for k, v in result.items():
            assert z[k].dtype == v.dtype and np.array_equal(z[k], v), k


@pytest.mark.parametrize('slope', [True, False])
def test_show_ground_writes_its_pictures(tmp_path, monkeypatch, slope):
    """The three files, their sizes and the range each map is coloured over; without ``slope_deg`` no slope picture.  ``colorize`` itself
    runs on the device even for a host array (test_visualize_cpu.py::test_colorize_rejects_cpu_tensors), so here a stand-in records its
    arguments; the real pictures are checked in tests/test_ground_maps_gpu.py."""
    from PIL import Image
    from gedepth_amd.depth import utils
    Base, depther = _depther()
    seen = []

    def colorize(value, cmap='magma_r', vmin=None, vmax=None):
        seen.append((cmap, vmin, vmax))
        return np.zeros(np.shape(value) + (3,), np.uint8)
    monkeypatch.setattr(utils, 'colorize', colorize)
    result = _host_dict(slope)
    Base.show_ground(depther, result, str(tmp_path / 'out' / 'frame.png'))
    names = ['frame_attention.png', 'frame_ground.png'] + (['frame_slope.png'] if slope else [])
    assert sorted(os.listdir(tmp_path / 'out')) == sorted(names)
    for n in names:
        assert Image.open(tmp_path / 'out' / n).size == (10, 6)
    want = [('magma_r', 0.0, 1.0)] + ([('magma_r', -5.0, 5.0)] if slope else []) + [('magma_r', 1e-3, 80.0)]
    assert seen == want


def test_cli_ground_dir_argument_errors():
    import importlib.util
    spec = importlib.util.spec_from_file_location('tools_test_cli_ground', os.path.join(ROOT, 'tools', 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = os.path.join(ROOT, 'configs', 'depthformer', 'depthformer_swint_a.py')
    with pytest.raises(ValueError, match='--device-eval'):
        cli.parse_args([cfg, '--ground-dir', 'out', '--eval', 'x'])                  # a host-loop evaluation
    for flag in (['--show-dir', 'd'], ['--ply-dir', 'd'], ['--out', 'r.pkl'], ['--show']):
        with pytest.raises(ValueError, match='--ground-dir cannot be combined'):
            cli.parse_args([cfg, '--ground-dir', 'out'] + flag)
    for argv in (['--ground-dir', 'out'], ['--ground-dir', 'out', '--format-only', '--bf16'],
                 ['--ground-dir', 'out', '--eval', 'x', '--device-eval', '--synthetic', '0']):
        assert cli.parse_args([cfg] + argv).ground_dir == 'out'

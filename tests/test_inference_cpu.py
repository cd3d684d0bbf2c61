"""The single-frame inference API (gedepth_amd/depth/apis/inference.py) and tools/benchmark.py: the checks that need no device."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'depthformer')


@pytest.fixture(scope='module')
def cpu_model():
    from gedepth_amd.depth.apis import init_depther
    return init_depther(os.path.join(CFG, 'depthformer_swint_v.py'), device='cpu')


def test_api_exports_and_config_type():
    from gedepth_amd.depth import apis
    from gedepth_amd.depth.apis import inference_depther, init_depther
    assert callable(init_depther) and callable(inference_depther)
    assert set(apis.__all__) >= {'init_depther', 'inference_depther'}
    with pytest.raises(TypeError, match='filename or Config'):
        init_depther(42)
    with pytest.raises(TypeError, match='filename or Config'):
        init_depther(dict(model=dict()))


def test_init_depther_contract(cpu_model):
    assert not cpu_model.training
    assert cpu_model.cfg.model.pretrained is None and cpu_model.cfg.model.train_cfg is None
    assert next(cpu_model.parameters()).device.type == 'cpu'


def test_no_ground_depth_source_is_a_value_error_before_device_work(cpu_model, tmp_path):
    """A CPU model: any device work (upload, allocation, kernel) would fail differently; the missing source is found first."""
    from gedepth_amd.depth.apis import inference_depther
    frame = np.zeros((375, 1242, 3), np.uint8)
    with pytest.raises(ValueError, match=r'pe=.*calib=.*pe_165\.npy'):
        inference_depther(cpu_model, frame)
    outside = tmp_path / 'frame.png'
    from PIL import Image
    Image.fromarray(frame).save(outside)
    with pytest.raises(ValueError, match='pe_165.npy'):
        inference_depther(cpu_model, [str(outside)])


def test_other_test_pipelines_are_not_implemented():
    from gedepth_amd.depth.apis import inference_depther, init_depther
    from gedepth_amd.depth.apis.inference import kitti_front_spec
    from gedepth_amd.mmrt.config import Config
    model = init_depther(os.path.join(CFG, 'depthformer_v_ddad.py'), device='cpu')
    with pytest.raises(NotImplementedError, match='DDADResize'):
        inference_depther(model, np.zeros((1216, 1936, 3), np.uint8), pe=np.zeros((1216, 1936), np.float32))
    cfg = Config.fromfile(os.path.join(CFG, 'depthformer_a_ddad.py'))
    with pytest.raises(NotImplementedError, match='DDADResize'):
        kitti_front_spec(cfg)


def test_kitti_front_spec_reads_the_config():
    from gedepth_amd.depth.apis.inference import kitti_front_spec
    from gedepth_amd.mmrt.config import Config
    cfg = Config.fromfile(os.path.join(CFG, 'depthformer_swint_v.py'))
    s = kitti_front_spec(cfg)
    assert (s['height'], s['width'], s['views']) == (352, 1216, 2)
    assert s['mean'] == [float(np.float32(v)) for v in (123.675, 116.28, 103.53)] and s['to_rgb']
    assert s['pe_max'] == 200.0 and s['depth_scale'] == 200.0
    aug = next(t for t in cfg.data.test.pipeline if t['type'] == 'MultiScaleFlipAug')
    aug['flip'] = False
    norm = next(t for t in aug['transforms'] if t['type'] == 'Normalize')
    norm['depth_scale'] = 250
    norm['mean'] = [1.0, 2.0, 3.0]
    s = kitti_front_spec(cfg)
    assert s['views'] == 1 and s['depth_scale'] == 250.0 and s['mean'] == [1.0, 2.0, 3.0]
    aug['transforms'].insert(0, dict(type='Resize', keep_ratio=True))
    with pytest.raises(NotImplementedError, match='Resize'):
        kitti_front_spec(cfg)


def test_engine_for_keeps_one_engine_per_config_and_precision(monkeypatch):
    """``engine_for`` with a stub in the engine's place (building the real one is device work): the same object while ``model.cfg`` says
    the same, a new one after the test pipeline or the image prefix changes, one per precision, a caller's ``config`` used as given, and
    the ``ValueError`` of a model without ``cfg``."""
    import types
    from gedepth_amd.depth.apis import inference
    from gedepth_amd.mmrt.config import Config
    built = []

    class Engine:
        def __init__(self, model, bf16=False, config=None):
            (self.spec, self.prefix), self.bf16 = config, bf16
            built.append(self)
    monkeypatch.setattr(inference, 'DepthInferencer', Engine)
    model = types.SimpleNamespace(cfg=Config.fromfile(os.path.join(CFG, 'depthformer_swint_v.py')))
    first = inference.engine_for(model, False)
    assert (first.spec, first.prefix) == (inference.front_spec(model.cfg), inference._img_prefix(model.cfg))
    assert inference.engine_for(model, False) is first and inference.engine_for(model, 0) is first and built == [first]
    assert model._ge_inferencers == {False: first}
    half = inference.engine_for(model, True)
    assert half is not first and half.bf16 is True and model._ge_inferencers == {False: first, True: half}
    kb = next(t for t in model.cfg.data.test.pipeline if t['type'] == 'KBCrop')
    kb['height'], kb['width'] = 320, 1184
    second = inference.engine_for(model, False)
    assert second is not first and (second.spec['height'], second.spec['width']) == (320, 1184)
    assert inference.engine_for(model, False) is second and model._ge_inferencers[False] is second
    model.cfg.data.test.data_root = '/another/tree'
    third = inference.engine_for(model, False)
    assert third is not second and third.prefix != second.prefix and len(built) == 4
    config = inference._config_of(model)
    assert config == (third.spec, third.prefix) and inference.engine_for(model, False, config) is third and len(built) == 4
    with pytest.raises(ValueError, match='model.cfg is missing: build the model with init_depther'):
        inference.engine_for(types.SimpleNamespace(), False)
    with pytest.raises(ValueError, match='model.cfg is missing: build the model with init_depther'):
        inference.engine_for(types.SimpleNamespace(cfg=None), True)
    assert len(built) == 4


def test_benchmark_cli_parses():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'benchmark.py'), '--help'], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    for flag in ('--log-interval', '--mode', '--bf16', '--data', 'checkpoint'):
        assert flag in out.stdout
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import benchmark
        a = benchmark.parse_args(['cfg.py', 'ckpt.pth', '--mode', 'graph', '--bf16'])
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    assert (a.config, a.checkpoint, a.mode, a.bf16, a.log_interval, a.frames) == ('cfg.py', 'ckpt.pth', 'graph', True, 50, 200)

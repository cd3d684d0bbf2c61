"""The 3x3 and 1x1 convolution kernels (csrc/conv3x3.hip, conv3x3_wgrad.hip, conv3x3_c1.hip, conv1x1_wgrad.hip) BIT FOR BIT against float64.

The random-data tests of test_kernels_gpu.py hold these kernels to 1e-2 of the tensor's largest magnitude: one dropped term out of
K = 9 Cin = 1440, a truncation instead of a rounding, or a wrong last pixel of a split-K range passes.  Here the operands are small integers
(tests/conv_exact.py): every product and every fp32 partial sum is exact in any order — MFMA, v_dot2, split-K and per-workgroup fp32 atomics —
so fp32 results must equal the float64 reference and bf16 results its one round-to-nearest-even: ``torch.equal``, no tolerance.  The shapes
are the small ones at which the persistent / prefetching / split-K loops reach their steady state; where that depends on the launcher's split
rule the test recomputes the rule from the device's CU count and asserts the precondition.  tests/test_conv_exact_cpu.py shows (without a
GPU) that the comparison fails for one dropped product, a truncation and two swapped channels."""
import pytest
import torch

import conv_exact as X

pytestmark = pytest.mark.gpu

CL = torch.channels_last
SENTINEL = 7.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gedepth_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ids(v):
    return 'x'.join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _conv3x3_module(c, dev, weight_grad):
    Co, Ci = c.w.shape[:2]
    conv = torch.nn.Conv2d(Ci, Co, 3, padding=1).to(dev).to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(c.w)
        conv.bias.copy_(c.b)
    conv.weight.requires_grad_(weight_grad)
    return conv


def _wgrad_direct(dev, x_cl, dy_cl, geom):
    """ge_conv3x3_nhwc_wgrad on channels-last bf16 device maps -> dW as (Cout, Cin, 3, 3) fp32 (a view of the (O, H, W, I) result)."""
    from gedepth_amd import hip
    N, Ci, Co, H, W = geom
    dw = torch.zeros(Co, 3, 3, Ci, device=dev)
    hip.check(hip.lib().ge_conv3x3_nhwc_wgrad(x_cl.data_ptr(), dy_cl.data_ptr(), dw.data_ptr(), N, H, W, Ci, Co, hip.GE_BF16, hip.stream()),
              'ge_conv3x3_nhwc_wgrad')
    return dw.permute(0, 3, 1, 2)


def _run_conv3x3(dev, c, weight_grad=False):
    """kernels.conv3x3 forward + backward on the case's operands: (y, dx, d_bias, conv, launch names)."""
    from gedepth_amd import kernels
    conv = _conv3x3_module(c, dev, weight_grad)
    xg = c.x.to(dev).contiguous(memory_format=CL).requires_grad_(True)
    assert kernels.conv3x3_ok(conv, xg)
    kernels.PROFILER.enable()
    y = kernels.conv3x3(conv, xg, conv.bias, act=c.slope is not None, slope=1.0 if c.slope is None else c.slope)
    y.backward(c.dy.to(dev))
    kernels.PROFILER.disable()
    names = [r['name'] for r in kernels.PROFILER.summary()]
    assert y.dtype == torch.bfloat16 and kernels._is_cl(y)
    return y, xg.grad, conv.bias.grad, conv, names


@pytest.mark.parametrize('variant', ['1', '2'])
@pytest.mark.parametrize('slope', X.SLOPES, ids=lambda s: f'slope{s}')
@pytest.mark.parametrize('geom', X.CONV3X3_GEOMS, ids=_ids)
def test_conv3x3_exact(dev, geom, slope, variant, monkeypatch):
    """kernels.conv3x3 through autograd on both forward kernels (GE_CONV3X3 = 1: register-staged 8 x 32 tile, 2: LDS-DMA 16 x 32 tile): y and
    dx equal the float64 reference rounded once to bf16, d_bias equals it in fp32; then ge_conv3x3_nhwc_wgrad directly, on the masked bf16
    gradient that the backward really receives: dW equals the reference in fp32.  (The weight gradient of these small maps goes to the
    library inside autograd — below the 10 000-pixel threshold — so the module's weight takes no gradient here.)"""
    monkeypatch.setenv('GE_CONV3X3', variant)
    c = X.conv3x3_case(geom, slope)
    y, dx, db, _, names = _run_conv3x3(dev, c)
    assert sum(n.startswith('conv3x3[') for n in names) == 2                          # forward and data gradient on the MFMA kernel
    what = f'conv3x3 {geom} slope {slope} variant {variant}'
    X.assert_equal(y, c.y, X.NCHW, what + ' y')
    X.assert_equal(dx, c.dx, X.NCHW, what + ' d_x')
    X.assert_equal(db, c.db, ('channel',), what + ' d_bias')
    dw = _wgrad_direct(dev, c.x.to(dev).contiguous(memory_format=CL), c.dyp.to(dev).contiguous(memory_format=CL), geom)
    X.assert_equal(dw, c.dw, X.OIRS, what + ' ge_conv3x3_nhwc_wgrad')


def test_conv3x3_variants_bit_identical_on_random_data(dev, monkeypatch):
    """csrc/conv3x3.hip claims that its two forward kernels do "the same products, same fp32 sums in the same order per accumulator": on
    N(0,1) bf16 data (where the order of the fp32 sums matters) y and dx of the two variants are bit-identical."""
    from gedepth_amd import kernels
    N, Ci, Co, H, W = 1, 160, 64, 13, 37
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, Ci, H, W, generator=g).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).bfloat16().float()
    b = torch.randn(Co, generator=g) * 0.2
    go = torch.randn(N, Co, H, W, generator=g).bfloat16()
    c = X.Conv3x3Case((N, Ci, Co, H, W), 0.5, x, w, b, go, *([None] * 9))
    out = {}
    for variant in ('1', '2'):
        monkeypatch.setenv('GE_CONV3X3', variant)
        y, dx, _, _, names = _run_conv3x3(dev, c)
        assert sum(n.startswith('conv3x3[') for n in names) == 2
        out[variant] = (y.detach().cpu(), dx.cpu())
    assert float(out['1'][0].float().abs().max()) > 0.5 and float(out['1'][1].float().abs().max()) > 0.5
    X.assert_equal(out['2'][0], out['1'][0], X.NCHW, 'y of the LDS-DMA kernel vs the register-staged kernel')
    X.assert_equal(out['2'][1], out['1'][1], X.NCHW, 'd_x of the LDS-DMA kernel vs the register-staged kernel')


@pytest.mark.parametrize('variant', ['1', '2'])
@pytest.mark.parametrize('cout', X.CONV3X3_ABI_COUTS)
def test_conv3x3_c_abi_partial_cout(dev, cout, variant, monkeypatch):
    """ge_conv3x3_nhwc_fwd and ge_conv3x3_nhwc_wgrad through the C ABI with Cout = 40 / 72 (the ABI promises Cout % 8 == 0; the wrappers
    only ever pass multiples of 32): the last 16-byte pieces of a 64-channel tile are cut.  The outputs sit in sentinel-framed buffers: exact
    inside, and the rows before and after keep the sentinel."""
    from gedepth_amd import hip
    monkeypatch.setenv('GE_CONV3X3', variant)
    c = X.conv3x3_abi_case(cout)
    N, Ci, H, W = c.geom
    M = N * H * W
    x = c.x.to(dev).contiguous(memory_format=CL)
    w = c.w.to(dev).contiguous(memory_format=CL)                                      # storage (Cout, 3, 3, Cin)
    b = c.b.to(dev)
    ybuf = torch.full((M + 2, cout), SENTINEL, device=dev, dtype=torch.bfloat16)
    assert ybuf[1:].data_ptr() % 16 == 0
    hip.check(hip.lib().ge_conv3x3_nhwc_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), ybuf[1:M + 1].data_ptr(), N, H, W, Ci, cout, 1, c.slope,
                                            hip.GE_BF16, hip.stream()), 'ge_conv3x3_nhwc_fwd')
    torch.cuda.synchronize()
    y = ybuf[1:M + 1].view(N, H, W, cout).permute(0, 3, 1, 2)
    X.assert_equal(y, c.y, X.NCHW, f'ge_conv3x3_nhwc_fwd Cout {cout} variant {variant}')
    assert bool((ybuf[0] == SENTINEL).all()) and bool((ybuf[M + 1] == SENTINEL).all()), 'ge_conv3x3_nhwc_fwd wrote outside y'
    dy = c.dy.to(dev).contiguous(memory_format=CL)
    wbuf = torch.full((cout * 9 + 2, Ci), SENTINEL, device=dev)
    wbuf[1:cout * 9 + 1].zero_()
    hip.check(hip.lib().ge_conv3x3_nhwc_wgrad(x.data_ptr(), dy.data_ptr(), wbuf[1:].data_ptr(), N, H, W, Ci, cout, hip.GE_BF16, hip.stream()),
              'ge_conv3x3_nhwc_wgrad')
    torch.cuda.synchronize()
    dw = wbuf[1:cout * 9 + 1].view(cout, 3, 3, Ci).permute(0, 3, 1, 2)
    X.assert_equal(dw, c.dw, X.OIRS, f'ge_conv3x3_nhwc_wgrad Cout {cout}')
    assert bool((wbuf[0] == SENTINEL).all()) and bool((wbuf[cout * 9 + 1] == SENTINEL).all()), 'ge_conv3x3_nhwc_wgrad wrote outside dW'


@pytest.mark.parametrize('slope', [None, 0.5], ids=lambda s: f'slope{s}')
def test_conv3x3_wgrad_several_tiles_per_workgroup(dev, slope):
    """ge_conv3x3_nhwc_wgrad where a workgroup walks several tiles, unevenly: (7, 512, 128, 9, 97) = 56 tiles of 8 x 32 for 32 output blocks;
    with ksplit = min(2 CUs / blocks, tiles) = 16 on 256 CUs the workgroups get 3 or 4 tiles (the cross-tile prefetch and its last, partial
    round)."""
    geom = X.CONV3X3_WGRAD_MULTI_TILE
    tiles, ksplit = X.conv3x3_wgrad_split(geom, _cus())
    assert tiles // ksplit >= 3 and tiles % ksplit != 0, (tiles, ksplit, _cus())
    c = X.conv3x3_case(geom, slope)
    dw = _wgrad_direct(dev, c.x.to(dev).contiguous(memory_format=CL), c.dyp.to(dev).contiguous(memory_format=CL), geom)
    X.assert_equal(dw, c.dw, X.OIRS, f'ge_conv3x3_nhwc_wgrad {geom} slope {slope}')


def test_conv3x3_wgrad_autograd_path(dev, monkeypatch):
    """The weight gradient INSIDE kernels.conv3x3's backward: 10 100 pixels reach the 10 000-pixel threshold of _Conv3x3.backward, the
    profiler shows ``conv3x3_wgrad[``, and conv.weight.grad — the (O, H, W, I) result viewed as (O, I, 3, 3) — equals the reference."""
    monkeypatch.delenv('GE_CONV3X3', raising=False)
    geom = X.CONV3X3_WGRAD_AUTOGRAD
    N, Ci, Co, H, W = geom
    assert N * H * W >= 10000
    c = X.conv3x3_case(geom, 0.5)
    y, dx, db, conv, names = _run_conv3x3(dev, c, weight_grad=True)
    assert any(n.startswith('conv3x3_wgrad[') for n in names), names
    assert conv.weight.grad.shape == (Co, Ci, 3, 3) and conv.weight.grad.dtype == torch.float32
    X.assert_equal(conv.weight.grad, c.dw, X.OIRS, f'conv3x3 {geom} d_w (autograd)')
    X.assert_equal(y, c.y, X.NCHW, f'conv3x3 {geom} y')
    X.assert_equal(dx, c.dx, X.NCHW, f'conv3x3 {geom} d_x')
    X.assert_equal(db, c.db, ('channel',), f'conv3x3 {geom} d_bias')


C1_ALL = tuple((g, 'one-unit') for g in X.C1_GEOMS) + ((X.C1_MULTI_UNIT_BWD, 'bwd-walks'), (X.C1_MULTI_UNIT_FWD, 'fwd-walks+bwd-walks'))


@pytest.mark.parametrize('out_fp32', [False, True], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('geom,walks', C1_ALL, ids=_ids)
def test_conv3x3_c1_exact(dev, geom, walks, out_fp32):
    """kernels.conv3x3_c1 forward and backward: y exact in fp32 / rounded once in bf16, dx, d_w (fp32) and d_bias exact.  The two large
    shapes have more units (4 rows x 128 pixels) than the grid cap of the backward (1024 workgroups) / of both directions (forward: 4096),
    so a workgroup walks more than one unit and the backward's per-lane partial d_w lives across units."""
    from gedepth_amd import kernels
    N, Ci, H, W = geom
    units = X.c1_units(N, H, W)
    assert ('fwd-walks' in walks) == (units > X.C1_CAP_FWD) and ('bwd-walks' in walks) == (units > X.C1_CAP_BWD), (units, walks)
    c = X.c1_case(geom, out_fp32)
    conv = torch.nn.Conv2d(Ci, 1, 3, padding=1).to(dev).to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(c.w)
        conv.bias.copy_(c.b)
    xg = c.x.to(dev).contiguous(memory_format=CL).requires_grad_(True)
    assert kernels.conv3x3_c1_ok(conv, xg)
    kernels.PROFILER.enable()
    y = kernels.conv3x3_c1(conv, xg, out_fp32=out_fp32)
    y.backward(c.dy.to(dev))
    kernels.PROFILER.disable()
    names = [r['name'] for r in kernels.PROFILER.summary()]
    assert any(n.startswith('conv3x3_c1[') for n in names) and any(n.startswith('conv3x3_c1_bwd[') for n in names)
    what = f'conv3x3_c1 {geom} {"fp32" if out_fp32 else "bf16"}'
    X.assert_equal(y, c.y, X.NCHW, what + ' y')
    X.assert_equal(xg.grad, c.dx, X.NCHW, what + ' d_x')
    assert conv.weight.grad.shape == (1, Ci, 3, 3)
    X.assert_equal(conv.weight.grad, c.dw, X.OIRS, what + ' d_w')
    X.assert_equal(conv.bias.grad, c.db, ('channel',), what + ' d_bias')


@pytest.mark.parametrize('rows', ['stages', '2053'])
@pytest.mark.parametrize('cout', X.CONV1X1_COUT)
@pytest.mark.parametrize('cin', X.CONV1X1_CIN)
def test_conv1x1_wgrad_exact(dev, cin, cout, rows, monkeypatch):
    """kernels.conv1x1_wgrad (opt-in): Cin 64 / 192 = chunks of 64 / 96 channels, Cout 544 = a second Cout chunk with a single 32-block;
    M = 64 * 3 * ksplit + 37 rows (ksplit = CUs / (n_ci n_co), the launcher's rule): every workgroup streams at least 3 stages, the first
    one a fourth, ragged one; and M = 2048 + 5 (the smallest map the wrapper takes).  dW (fp32) equals the reference."""
    from gedepth_amd import kernels
    M = X.conv1x1_rows(cin, cout, _cus())[0 if rows == 'stages' else 1]
    stages, ksplit = X.conv1x1_wgrad_split(M, cin, cout, _cus())
    if rows == 'stages':
        assert stages // ksplit >= 3 and stages % ksplit == 1 and M % X.CONV1X1_STAGE == 37, (M, stages, ksplit)
    c = X.conv1x1_case(M, cin, cout)
    x = c.x.to(dev).view(1, 1, M, cin).permute(0, 3, 1, 2)                            # a channels-last (1, Cin, 1, M) map IS the row matrix
    dy = c.dy.to(dev).view(1, 1, M, cout).permute(0, 3, 1, 2)
    w = torch.empty(cout, cin, 1, 1, device=dev, dtype=torch.bfloat16)
    monkeypatch.setattr(kernels, 'ENABLED', kernels.ENABLED | {'conv1x1_wgrad'})      # opt-in path, as in test_conv1x1_wgrad_vs_float64
    assert kernels.conv1x1_wgrad_ok(x, dy, w, (1, 1), (0, 0), (1, 1), 1)
    dw = kernels.conv1x1_wgrad(x, dy)
    X.assert_equal(dw, c.dw, X.OI, f'conv1x1_wgrad M {M} {cin}->{cout}')

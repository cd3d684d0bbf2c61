"""csrc/conv1x1_bn.hip (the HAHI neck's conv_proj: 1x1 conv + training BatchNorm + ReLU + position add, kernels.conv1x1_bn_act_pos) where
test_kernels_gpu.test_conv1x1_bn_act_pos_vs_fp32_composition does not look:

* inputs with a channel mean well above the deviation and output gradients with a mean and a component along the normalised activation
  (what training produces): d_gamma, d_beta and the rank-64 corrections ``X A2 + c0`` of the data gradient are then NOT ~0, and the bf16
  storage of A2 meets the raw, un-centred input (tests/test_conv1x1_bn_algebra_cpu.py restates the algebra);
* shapes at which the persistent loops of the three streaming kernels reach their steady state (the cross-tile prefetches run);
* tile and channel edges: fewer rows than a tile, every chunk count of the dgrad loop, a zero weight row, a channel that never fires.

Reference everywhere: float64 conv (a matrix product over the rows) -> batch_norm(training) -> relu -> + pos, differentiated by autograd, on
the same bf16-rounded x, weight, dy and dq.  Yardstick for the gradients: the project's two-pass path (library convolution storing z in
bf16, the bn_act kernels, the position add in torch) on the same inputs, against the same reference:
``e_fused <= max(1.5 e_two_pass, 6e-3)`` in l2 — 1.5 for the different rounding points of the two paths (the margin of
test_token_linear_on_own_gemm_matches_library_path), 6e-3 the bound the first test of this block puts on dW, d_gamma and d_beta (the bf16
storage of g)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import close, gen, l2rel

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
GRADS = ('dx', 'dw', 'dgamma', 'dbeta')
FLOOR = 6e-3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gedepth_amd import hip
    hip.lib()
    return torch.device('cuda:0')


def _make(shape, cout, r, seed=177, tweak=None):
    """block (CPU, seeded as the first test of this block seeds it), x = randn + r * (+-1 per channel) in bf16, pos, and the noise of dy / dq."""
    from gedepth_amd.mmrt.bricks import ConvModule
    g = gen(seed)
    B, Cin, H, W = shape
    block = ConvModule(Cin, cout, 1, norm_cfg=dict(type='BN', requires_grad=True), act_cfg=dict(type='ReLU'))
    with torch.no_grad():
        block.conv.weight.copy_(torch.randn(cout, Cin, 1, 1, generator=g) * 0.2)
        block.norm.weight.copy_(torch.rand(cout, generator=g) + 0.5); block.norm.bias.copy_(torch.randn(cout, generator=g) * 0.3)
        block.norm.running_mean.copy_(torch.randn(cout, generator=g)); block.norm.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
        if tweak is not None:
            tweak(block)
    sign = (torch.randint(0, 2, (Cin,), generator=g) * 2 - 1).float().view(1, Cin, 1, 1)
    x = (torch.randn(*shape, generator=g) + r * sign).to(BF16)
    pos = torch.randn(1, cout, H, W, generator=g)
    return block, x, pos, torch.randn(B, cout, H, W, generator=g), torch.randn(B, H * W, cout, generator=g)


def _reference(block, x, pos, noise_y, noise_q):
    """float64 on the bf16-rounded operands.  The output gradients are built HERE, from the reference's own normalised pre-activation:
    dy (map) and dq (tokens) = randn + 0.7 + zhat, rounded to bf16.  ``pos`` None: no query, no dq."""
    bn = block.norm
    B, Cin, H, W = x.shape
    cout, n = noise_y.shape[1], B * H * W
    xr = x.double().permute(0, 2, 3, 1).reshape(n, Cin).requires_grad_(True)
    wr = block.conv.weight.detach().to(BF16).double().reshape(cout, Cin).requires_grad_(True)
    gam, bet = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
    rm, rv = bn.running_mean.double().clone(), bn.running_var.double().clone()
    z = xr @ wr.t()
    mean, var = z.detach().mean(0), z.detach().var(0, unbiased=False)
    zhat = (z.detach() - mean) / (var + bn.eps).sqrt()
    if n > 1:
        y = F.relu(F.batch_norm(z, rm, rv, gam, bet, True, bn.momentum, bn.eps))
    else:                                                   # F.batch_norm refuses one value per channel; the same formulas, the variance (0) as it is
        y = F.relu((z - z.mean(0)) / (z.var(0, unbiased=False) + bn.eps).sqrt() * gam + bet)
        rm, rv = (1 - bn.momentum) * rm + bn.momentum * mean, (1 - bn.momentum) * rv + bn.momentum * var
    dy = (noise_y.double() + 0.7 + zhat.reshape(B, H, W, cout).permute(0, 3, 1, 2)).to(BF16)
    loss = (y * dy.double().permute(0, 2, 3, 1).reshape(n, cout)).sum()
    q = dq = None
    if pos is not None:
        q = y.reshape(B, H * W, cout) + pos.double().flatten(2).transpose(1, 2)
        dq = (noise_q.double() + 0.7 + zhat.reshape(B, H * W, cout)).to(BF16)
        loss = loss + (q * dq.double()).sum()
    loss.backward()
    return dict(y=y.detach().reshape(B, H, W, cout).permute(0, 3, 1, 2), q=None if q is None else q.detach(), rm=rm, rv=rv,
                dx=xr.grad.reshape(B, H, W, Cin).permute(0, 3, 1, 2), dw=wr.grad.reshape(cout, Cin, 1, 1), dgamma=gam.grad, dbeta=bet.grad,
                dy=dy, dq=dq)


def _run(dev, block, x, pos, dy, dq, fused):
    """The block on the GPU under bf16 autocast: the fused kernels, or (``fused`` False; the caller has put 'conv1x1_bn' into kernels.DISABLED)
    the two-pass path — block(x), tokens + pos in torch."""
    from gedepth_amd import kernels as K
    blk = copy.deepcopy(block).to(dev).train()
    xg = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    q = None
    with torch.autocast('cuda', dtype=BF16):
        if fused:
            assert K.conv1x1_bn_act_pos_ok(blk, xg)
            y, q = K.conv1x1_bn_act_pos(blk, xg, None if pos is None else pos.to(dev))
            assert y.dtype == BF16 and y.is_contiguous(memory_format=torch.channels_last) and (q is None) == (pos is None)
        else:
            assert not K.conv1x1_bn_act_pos_ok(blk, xg)
            y = blk(xg)
            if pos is not None:
                q = (y.flatten(2).transpose(1, 2).float() + pos.to(dev).flatten(2).transpose(1, 2)).to(BF16)
    out = (y.float() * dy.to(dev).float()).sum()
    if q is not None:
        out = out + (q.float() * dq.to(dev).float()).sum()
    out.backward()
    bn = blk.norm
    assert int(bn.num_batches_tracked) == 1
    return dict(y=y.detach(), q=None if q is None else q.detach(), rm=bn.running_mean.detach().clone(), rv=bn.running_var.detach().clone(),
                dx=xg.grad, dw=blk.conv.weight.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad)


def _three(dev, monkeypatch, shape, cout, r, with_pos=True, tweak=None):
    """(reference, fused, two-pass) of one case"""
    from gedepth_amd import kernels as K
    block, x, pos, ny, nq = _make(shape, cout, r, tweak=tweak)
    pos = pos if with_pos else None
    ref = _reference(block, x, pos, ny, nq)
    fused = _run(dev, block, x, pos, ref['dy'], ref['dq'], True)
    monkeypatch.setattr(K, 'DISABLED', set(K.DISABLED) | {'conv1x1_bn'})
    two = _run(dev, block, x, pos, ref['dy'], ref['dq'], False)
    monkeypatch.setattr(K, 'DISABLED', set(K.DISABLED) - {'conv1x1_bn'})
    return ref, fused, two


def _judge(tag, ref, fused, two):
    """outputs and running statistics at the first test's ``close`` bounds (NaN-strict); each gradient against the two-pass yardstick"""
    close(fused['y'].float(), ref['y'], rtol=2 ** -7, atol=2 ** -7, what='y')
    if ref['q'] is not None:
        close(fused['q'].float(), ref['q'], rtol=2 ** -7, atol=2 ** -6, what='q')
    close(fused['rm'], ref['rm'], rtol=1e-4, atol=1e-5, what='running_mean')
    close(fused['rv'], ref['rv'], rtol=1e-4, atol=1e-5, what='running_var')
    ef, et = {k: l2rel(fused[k], ref[k]) for k in GRADS}, {k: l2rel(two[k], ref[k]) for k in GRADS}
    print(f'\n[conv1x1_bn {tag}] l2 errors  fused ' + ' '.join(f'{k} {ef[k]:.2e}' for k in GRADS) + '  |  two-pass ' + ' '.join(f'{k} {et[k]:.2e}' for k in GRADS))
    for k in GRADS:
        assert all(bool(torch.isfinite(t[k]).all()) for t in (fused, two)), k
    bad = {k: (ef[k], et[k]) for k in GRADS if not ef[k] <= max(1.5 * et[k], FLOOR)}
    assert not bad, f'{tag}: fused error above max(1.5 x two-pass, {FLOOR}): {bad}'
    return ef, et


# ====================================================================== 1. offset sweep
@pytest.mark.parametrize('shape,cout,r', [((2, 64, 24, 40), 512, 0), ((2, 64, 24, 40), 512, 4), ((2, 64, 24, 40), 512, 16), ((2, 64, 24, 40), 128, 16)])
def test_offset_inputs_and_correlated_gradients(dev, monkeypatch, shape, cout, r):
    """x = randn + r * (+-1 per channel), dy and dq = randn + 0.7 + zhat: every quantity against float64 autograd, the four gradients no worse
    than max(1.5 x the two-pass path's error, 6e-3).

    Measured on MI355X, l2 error of dx / dW / d_gamma / d_beta (fused | two-pass):
      ->512 r=0   before the c0 compensation 7.41e-03 3.73e-03 1.02e-04 7.61e-05, with it 7.41e-03 3.73e-03 1.02e-04 7.61e-05 | 1.82e-02 1.90e-02 2.50e-04 4.77e-04
      ->512 r=4   before 2.19e-02 3.74e-03 9.97e-05 7.38e-05, with it 7.43e-03 3.74e-03 9.97e-05 7.38e-05 | 6.40e-02 6.50e-02 8.60e-04 2.47e-03
      ->512 r=16  before 8.65e-02 3.74e-03 9.35e-05 7.23e-05, with it 7.51e-03 3.74e-03 9.36e-05 7.23e-05 | 1.31e-01 1.53e-01 4.06e-03 1.05e-02
      ->128 r=16  before 4.66e-02 3.70e-03 9.20e-05 7.15e-05, with it 5.95e-03 3.70e-03 9.22e-05 7.15e-05 | 1.16e-01 1.45e-01 2.80e-03 7.60e-03
    The criterion held before the compensation as well — the two-pass path loses more on these inputs than the fused one did; the growth of
    the fused dx error with r is pinned by test_dx_error_does_not_grow_with_the_offset.
    """
    _sweep(dev, monkeypatch, shape, cout, r)


_SWEEP = {}                    # (shape, cout, r) -> (fused errors, two-pass errors): each case is computed once


def _sweep(dev, monkeypatch, shape, cout, r):
    if (shape, cout, r) not in _SWEEP:
        _SWEEP[shape, cout, r] = _judge(f'{shape}->{cout} r={r}', *_three(dev, monkeypatch, shape, cout, r))
    return _SWEEP[shape, cout, r]


@pytest.mark.parametrize('r', [4, 16])
def test_dx_error_does_not_grow_with_the_offset(dev, monkeypatch, r):
    """The two-pass yardstick is itself at 6e-2 .. 1.3e-1 on offset inputs (it stores z in bf16), so the criterion above lets a dx error
    pass that is ten times the one at r = 0.  What the compensation in c0 buys is a dx error that does not depend on the offset: in the
    restated algebra (tests/test_conv1x1_bn_algebra_cpu.py) the exact-A2 error is flat in r and the compensated form stays within 1.3 x of
    it, hence within 1.3 x of its own error at r = 0.  Without the compensation the ratio measured 3.0 (r = 4) and 11.7 (r = 16); with it 1.00 and 1.01."""
    shape, cout = (2, 64, 24, 40), 512
    e0, er = _sweep(dev, monkeypatch, shape, cout, 0)[0]['dx'], _sweep(dev, monkeypatch, shape, cout, r)[0]['dx']
    print(f'\n[conv1x1_bn offset growth] dx l2 error r=0 {e0:.2e}, r={r} {er:.2e}: ratio {er / e0:.2f}')
    assert er <= 1.3 * e0, (r, er, e0)


# ====================================================================== 2. multi-tile shapes
def launch_geometry(B, HW, cout, cus):
    """How the launch rules of csrc/conv1x1_bn.hip (ge_conv1x1_bn_act_fwd, ge_conv1x1_bn_dgrad, ge_conv1x1_bn_stats) deal the work on ``cus`` CUs."""
    rows, npt = B * HW, -(-HW // 32)
    gx = -(-min(cus * 4, npt * B) // 8) * 8                                  # conv1x1_bn_act_k: workgroups, gx / 8 per XCD
    wgx = gx // 8
    xcd_tiles = [(-(-(npt - x) // 8) if npt > x else 0) * B for x in range(8)]     # tiles of XCD x: position tiles p = x (mod 8), every image
    per_wg = [(n - j0 + wgx - 1) // wgx if n > j0 else 0 for n in xcd_tiles for j0 in (0, wgx - 1)]
    smem = 64 * (cout + 64 + 8) * 2                                          # conv1x1_bn_dgrad_k: tiles of 32 rows over 4 waves per workgroup
    dgrad_tiles = -(-rows // 32)
    dgrad_waves = 4 * min(cus * (2 if smem <= 78 * 1024 else 1), -(-dgrad_tiles // 4))
    gram_blocks = -(-rows // 64)                                             # conv1x1_gram_k: blocks of 64 rows over 4 waves per workgroup
    gram_waves = 4 * (-(-gram_blocks // 4) if gram_blocks < 4 * 256 else 256)
    return dict(act_min=min(per_wg), act_max=max(per_wg), xcd_tiles=xcd_tiles, dgrad_tiles=dgrad_tiles, dgrad_waves=dgrad_waves,
                gram_blocks=gram_blocks, gram_waves=gram_waves)


def _steady(geo):
    """some dgrad waves take a second tile (the cross-tile prefetch runs) and the last sweep is partial; some gram waves take a second block"""
    return geo['dgrad_tiles'] > geo['dgrad_waves'] and geo['dgrad_tiles'] % geo['dgrad_waves'] != 0 and geo['gram_blocks'] > geo['gram_waves']


def multi_tile_shape(kind, cus, cout=128):
    """'even': the smallest (2, 64, H, 280), H a multiple of 8, at which EVERY act_k workgroup takes >= 3 tiles ((2, 64, 176, 280) on 256 CUs);
    'ragged': the smallest (3, 64, H, 187), H odd, with H * W no multiple of 32, an uneven tile count over the XCDs and some act_k workgroup
    at 3 tiles.  Both with the dgrad and gram loops past their first sweep."""
    B, W, hs = (2, 280, range(8, 2048, 8)) if kind == 'even' else (3, 187, range(3, 2048, 2))
    for H in hs:
        geo = launch_geometry(B, H * W, cout, cus)
        if not _steady(geo):
            continue
        if kind == 'even' and geo['act_min'] >= 3:
            return (B, 64, H, W), geo
        if kind == 'ragged' and geo['act_max'] >= 3 and (H * W) % 32 and len(set(geo['xcd_tiles'])) > 1:
            return (B, 64, H, W), geo
    raise AssertionError(f'no {kind} multi-tile shape for {cus} CUs')


@pytest.mark.parametrize('kind', ['even', 'ragged'])
def test_steady_state_of_the_persistent_loops(dev, monkeypatch, kind):
    """Shapes sized from the device's CU count so that the act_k tile prefetch (CB_LOAD_A(t + wgx)), the dgrad cross-tile prefetch
    (CB_LOADG(Fa, tile + tstep, 0)) and the second block of a gram_k wave all run; Cout = 128, r = 4.  Same comparisons as the sweep.

    Measured on MI355X, l2 error of dx / dW / d_gamma / d_beta (fused | two-pass):
      (2, 64, 176, 280) on 256 CUs  6.04e-03 3.74e-03 1.47e-05 1.14e-05 | 6.88e-02 9.21e-02 1.15e-03 2.61e-03   (dx 1.39e-02 before the c0 compensation)
      (3, 64, 117, 187) on 256 CUs  6.12e-03 3.94e-03 1.77e-05 1.38e-05 | 5.92e-02 8.39e-02 6.25e-04 1.96e-03   (dx 1.33e-02 before)
    """
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    shape, geo = multi_tile_shape(kind, cus)
    print(f'\n[conv1x1_bn multi-tile {kind}] {cus} CUs -> {shape}: {geo}')
    assert geo['dgrad_tiles'] > geo['dgrad_waves'] and geo['dgrad_tiles'] % geo['dgrad_waves'] != 0
    assert geo['gram_blocks'] > geo['gram_waves']
    if kind == 'even':
        assert geo['act_min'] >= 3
    else:
        assert geo['act_max'] >= 3 and (shape[2] * shape[3]) % 32 != 0 and len(set(geo['xcd_tiles'])) > 1
    _judge(f'multi-tile {kind} {shape}', *_three(dev, monkeypatch, shape, 128, 4))


def test_multi_tile_shape_on_256_cus():
    shape, geo = multi_tile_shape('even', 256)
    assert shape == (2, 64, 176, 280) and geo['act_min'] == 3 and geo['dgrad_waves'] == 2048 and geo['gram_waves'] == 1024, (shape, geo)


# ====================================================================== 3. edges
EDGES = [((1, 64, 3, 5), 128, True), ((3, 64, 1, 31), 128, True), ((3, 64, 3, 11), 128, True), ((3, 64, 3, 11), 128, False),      # rows 15, 93, 99: < 32, HW < 32
         ((2, 64, 7, 9), 128, True), ((2, 64, 7, 9), 384, True), ((2, 64, 7, 9), 640, True), ((2, 64, 7, 9), 1024, True)]          # dgrad chunks 1, 3, 5, 8


@pytest.mark.parametrize('shape,cout,with_pos', EDGES)
def test_tile_and_channel_edges(dev, monkeypatch, shape, cout, with_pos):
    """Fewer rows than one 32-token tile / 64-row Gram block, HW < 32 with several images, no position map; Cout 384 and 640 (odd chunk count
    of the dgrad loop, a second blockIdx.y group with idle waves in act_k), 1024 (one dgrad workgroup per CU).  r = 4, same comparisons."""
    _judge(f'edge {shape}->{cout} pos={with_pos}', *_three(dev, monkeypatch, shape, cout, 4, with_pos=with_pos))


def test_one_row(dev):
    """(1, 64, 1, 1): one value per channel, variance exactly 0, zhat = 0: y = relu(beta), and dx = dW = d_gamma = 0 by cancellation of terms
    of size a |g| |w| with a = gamma / sqrt(eps).  No two-pass yardstick here (the reference gradients are 0); the bounds are those of the
    arithmetic: G = g x and s m1 / n are single exact products, so dW and d_gamma cancel to fp32 level (2^-20 of the cancelling terms leaves
    16 ulps); in dx = g A1 + c0 the one rounding that does not cancel is A1's bf16 storage, half an ulp of 8 significand bits = 2^-8 of
    sum_c |g_c| a_c |w_ci| per element at the most (+ 5 % for the fp32 sums and the stored result's own rounding).  d_beta is the one
    bf16-rounded g: 2^-8 again."""
    shape, cout = (1, 64, 1, 1), 128
    block, x, pos, ny, nq = _make(shape, cout, 4)
    ref = _reference(block, x, pos, ny, nq)
    fused = _run(dev, block, x, pos, ref['dy'], ref['dq'], True)
    close(fused['y'].float(), ref['y'], rtol=2 ** -7, atol=2 ** -7, what='y')
    close(fused['y'].float().flatten(), F.relu(block.norm.bias.detach()), rtol=2 ** -7, atol=2 ** -7, what='y = relu(beta)')
    close(fused['q'].float(), ref['q'], rtol=2 ** -7, atol=2 ** -6, what='q')
    close(fused['rm'], ref['rm'], rtol=1e-4, atol=1e-5, what='running_mean')
    close(fused['rv'], ref['rv'], rtol=1e-4, atol=1e-5, what='running_var')
    for k in ('dx', 'dw', 'dgamma'):
        assert float(ref[k].abs().max()) <= 1e-9, k                         # the reference agrees that they vanish
    gabs = ((ref['dy'].double().flatten() + ref['dq'].double().flatten()) * (ref['y'].flatten() > 0)).abs()        # (Cout)
    a = block.norm.weight.detach().double() / block.norm.eps ** 0.5
    wabs = block.conv.weight.detach().to(BF16).double().reshape(cout, 64).abs()
    xabs = x.double().flatten().abs()
    cond = dict(dx=((gabs * a) @ wabs).view(1, 64, 1, 1), dw=((gabs * a)[:, None] * xabs[None]).view(cout, 64, 1, 1), dgamma=gabs * a / block.norm.weight.detach().double() * (wabs @ xabs))
    print('\n[conv1x1_bn one row] max |dx| %.3e (bound %.3e)  max |dW| %.3e  max |dgamma| %.3e' % (
        float(fused['dx'].abs().max()), float(1.05 * 2 ** -8 * cond['dx'].max()), float(fused['dw'].abs().max()), float(fused['dgamma'].abs().max())))
    for k, u in (('dx', 1.05 * 2 ** -8), ('dw', 2 ** -20), ('dgamma', 2 ** -20)):
        got = fused[k].detach().double().cpu()
        assert bool((got.abs() <= u * cond[k]).all()), (k, float((got.abs() / cond[k].clamp_min(1e-300)).max()), u)       # NaN-strict: NaN <= x is False
    close(fused['dbeta'], ref['dbeta'], rtol=1.01 * 2 ** -8, atol=0, what='dbeta')             # d_beta = g, stored in bf16: half an ulp


def test_zero_weight_row(dev, monkeypatch):
    """A weight row of zeros: z = 0, variance exactly 0 (rstd = 1 / sqrt(eps)), the channel's output is relu(beta) to the bit, nothing is
    non-finite, and the gradients (d_gamma_c = 0, dW_c = a_c sum g_c (x - m), large) hold the common criterion."""
    c = 5

    def tweak(block):
        block.conv.weight[c].zero_()
        block.norm.bias[c] = 0.75
    ref, fused, two = _three(dev, monkeypatch, (2, 64, 7, 9), 128, 4, tweak=tweak)
    assert bool((fused['y'][:, c].float() == 0.75).all()) and bool((ref['y'][:, c] == 0.75).all())
    for k, v in fused.items():
        assert v is None or bool(torch.isfinite(v).all()), k
    assert float(fused['dgamma'][c]) == 0.0                               # w_c = 0 multiplies every term of it
    _judge('zero weight row', ref, fused, two)


def test_channel_that_never_fires(dev, monkeypatch):
    """beta_c = -50 (|zhat| <= sqrt(rows) = 11.3, gamma <= 1.5): y_c = 0 everywhere, so g_c = 0: d_gamma_c = d_beta_c = 0 exactly, dW_c finite"""
    c = 7

    def tweak(block):
        block.norm.bias[c] = -50.0
    ref, fused, two = _three(dev, monkeypatch, (2, 64, 7, 9), 128, 4, tweak=tweak)
    assert bool((fused['y'][:, c] == 0).all())
    assert float(fused['dgamma'][c]) == 0.0 and float(fused['dbeta'][c]) == 0.0
    assert bool(torch.isfinite(fused['dw'][c]).all()) and bool(torch.isfinite(fused['dx']).all())
    _judge('channel that never fires', ref, fused, two)


# ====================================================================== 4. reproducibility
@pytest.mark.parametrize('shape', [(2, 64, 24, 40), (3, 64, 3, 7)])
def test_fixed_order_reductions_are_bit_reproducible(dev, shape):
    """Two runs on the same inputs: y, q, the running statistics and d_beta come from reductions with a fixed order (per-workgroup partials
    summed in fp64 in index order) and must agree to the bit.  dW and dx are not asserted: the weight-gradient kernel flushes G = g^T X with
    fp32 atomics.  d_gamma is formed from that same G, so it can be asserted only where G has one contributor per element — up to 64 rows,
    one stage of ge_conv1x1_nhwc_wgrad: the (3, 64, 3, 7) case; at 1920 rows its agreement is printed (measured: not bit-identical)."""
    block, x, pos, ny, nq = _make(shape, 512, 4)
    ref = _reference(block, x, pos, ny, nq)
    a, b = (_run(dev, block, x, pos, ref['dy'], ref['dq'], True) for _ in range(2))
    rows = shape[0] * shape[2] * shape[3]
    same_dgamma = bool(torch.equal(a['dgamma'], b['dgamma']))
    print(f'\n[conv1x1_bn reproducibility {shape}] d_gamma bit-identical: {same_dgamma}; dW: {bool(torch.equal(a["dw"], b["dw"]))}; dx: {bool(torch.equal(a["dx"], b["dx"]))}')
    for k in ('y', 'q', 'rm', 'rv', 'dbeta') + (('dgamma',) if rows <= 64 else ()):
        assert torch.equal(a[k], b[k]), k

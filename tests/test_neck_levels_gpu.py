"""The HAHI neck's level-token kernels on the MI355X (csrc/nhwc.hip, include/gedepth_neck.h, gedepth_amd/neck_kernels.py) under red zones and
poison (tests/memguard.py): every output, gradient and workspace of the wrappers is carved out of a poisoned frame, so an element that is
not written fails the value comparison under both poison bytes and a write outside an output fails ``Guard.check``.

Shapes: B = 2 and levels (3, 5), (2, 3), (1, 2): 23 rows per image with level starts 0, 15, 21 — no level begins on a multiple of the rows a
workgroup takes per iteration; C = 16 and C = 512 (the model's 64-lane row), bf16 and fp32.

* ``*_rows`` BatchNorm: output, running statistics and all gradients ``torch.equal`` with ``kernels.bn_act`` per level and ``torch.cat``.
* ``ge_add_rows_levels``: ``torch.equal`` with ``kernels.add_rows(x, cat(pos_l + emb_l))``.
* ``ge_level_colsum`` against float64: per column |err| <= n * 2^-24 * sum|x|, n the rows summed (the fp32 worst case).
* ``ge_token_grad_sum`` against float64: |err| <= 2^-8 |ref| + 2^-22 * sum_k |x_k| (one bf16 rounding plus the fp32 adds).
* the neck itself, level route against GE_DISABLE=neck_levels: see ``test_neck_level_route_against_the_old_route``."""
import numpy as np
import pytest
import torch

import memguard

pytestmark = pytest.mark.gpu
B, LEVELS = 2, ((3, 5), (2, 3), (1, 2))
ROWS = [h * w for h, w in LEVELS]
N = sum(ROWS)
DTYPES = {'bf16': torch.bfloat16, 'f32': torch.float32}
CASES = [(16, 'bf16'), (16, 'f32'), (512, 'bf16'), (512, 'f32')]
CL = torch.channels_last


def _install(monkeypatch, poison):
    from gedepth_amd import hip, neck_kernels
    guard = memguard.Guard(poison)
    monkeypatch.setattr(neck_kernels, '_WS', {})                    # a workspace cached by an earlier test would bypass the frames
    guard.install(monkeypatch, [neck_kernels], binding=hip)
    return guard


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(*shape, generator=_gen(seed)).to(dtype).cuda()


def _bns(C, seed):
    out = []
    for l in range(len(LEVELS)):
        bn = torch.nn.BatchNorm2d(C).cuda().train()
        with torch.no_grad():
            bn.weight.copy_(_randn((C,), seed + 10 * l) * 0.5 + 1.0)
            bn.bias.copy_(_randn((C,), seed + 10 * l + 1) * 0.3)
            bn.running_mean.copy_(_randn((C,), seed + 10 * l + 2) * 0.1)
        out.append(bn)
    return out


# ------------------------------------------------------------------------------------------------ BatchNorm + ReLU into / out of level rows
@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('C,tag', CASES)
def test_bn_rows_carry_the_bits_of_bn_act_and_cat(monkeypatch, C, tag, poison):
    from gedepth_amd import kernels as K
    from gedepth_amd import neck_kernels as NK
    dt = DTYPES[tag]
    maps = [_randn((B, C, h, w), 3 + l, dt).contiguous(memory_format=CL) for l, (h, w) in enumerate(LEVELS)]
    dy = _randn((B, N, C), 11, dt)
    # the existing path: bn_act per level, cat; its backward slices dy and packs every slice
    ref_x = [m.clone(memory_format=torch.preserve_format).requires_grad_() for m in maps]
    ref_bn = _bns(C, 100)
    ref = torch.cat([K.bn_act(x, bn, 0.0).flatten(2).transpose(1, 2) for x, bn in zip(ref_x, ref_bn)], 1)
    ref.backward(dy)

    guard = _install(monkeypatch, poison)
    xs = [guard.framed(m).requires_grad_() for m in maps]
    bns = _bns(C, 100)
    got = NK.bn_act_levels(xs, bns, [0.0] * len(LEVELS))
    got.backward(guard.framed(dy))
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()
    assert 'ge_bn_act_nhwc_fwd_rows' in guard.launched and 'ge_bn_act_nhwc_bwd_rows' in guard.launched
    assert tuple(got.shape) == (B, N, C) and torch.equal(got, ref), 'forward'
    for l in range(len(LEVELS)):
        assert torch.equal(bns[l].running_mean, ref_bn[l].running_mean) and torch.equal(bns[l].running_var, ref_bn[l].running_var), l
        assert int(bns[l].num_batches_tracked) == int(ref_bn[l].num_batches_tracked) == 1
        assert xs[l].grad.is_contiguous(memory_format=CL) and torch.equal(xs[l].grad, ref_x[l].grad), f'dx of level {l}'
        assert torch.equal(bns[l].weight.grad, ref_bn[l].weight.grad), f'dgamma of level {l}'
        assert torch.equal(bns[l].bias.grad, ref_bn[l].bias.grad), f'dbeta of level {l}'


# ------------------------------------------------------------------------------------------------ position add with the level embedding
@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('C,tag', CASES)
def test_add_rows_levels_carries_the_bits_of_add_rows(monkeypatch, C, tag, poison):
    from gedepth_amd import kernels as K
    from gedepth_amd import neck_kernels as NK
    x, pos, emb = _randn((B, N, C), 21, DTYPES[tag]), _randn((N, C), 22), _randn((4, C), 23)          # four embedding rows, three levels
    starts = np.cumsum([0] + ROWS)
    rows = torch.cat([pos[starts[l]:starts[l + 1]] + emb[l].view(1, -1) for l in range(len(ROWS))], 0)
    ref = K.add_rows(x, rows)
    guard = _install(monkeypatch, poison)
    got = NK.add_rows_levels(guard.framed(x), guard.framed(pos), guard.framed(emb), ROWS)
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()
    assert guard.launched == ['ge_add_rows_levels'] and torch.equal(got, ref)


@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('C,tag', CASES)
def test_level_colsum_vs_float64(monkeypatch, C, tag, poison):
    from gedepth_amd import neck_kernels as NK
    x = _randn((B, N, C), 31, DTYPES[tag])
    guard = _install(monkeypatch, poison)
    got = NK.level_colsum(guard.framed(x), ROWS, 4)
    torch.cuda.synchronize()
    monkeypatch.undo()
    frames = guard.check()                                             # the output, the workspace, the input
    assert guard.launched == ['ge_level_colsum'] and tuple(got.shape) == (4, C) and got.dtype == torch.float32
    assert any(f.kind == 'empty' and f.dtype == torch.uint8 for f in frames), 'the workspace was framed'
    x64, starts = x.double().cpu(), np.cumsum([0] + ROWS)
    for l in range(len(ROWS)):
        seg = x64[:, starts[l]:starts[l + 1]].reshape(-1, C)
        err = (got[l].double().cpu() - seg.sum(0)).abs()
        bound = seg.shape[0] * 2.0 ** -24 * seg.abs().sum(0)
        print(f'level_colsum C={C} {tag} level {l}: max err / bound = {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all()), (l, float((err / bound).max()))
    assert not bool(got[3].any()), 'an empty level sums to zero'


# ------------------------------------------------------------------------------------------------ gradient fan-in
@pytest.mark.parametrize('poison', memguard.POISONS, ids=lambda p: f'{p:02x}')
@pytest.mark.parametrize('with_parts', [False, True], ids=['dense', 'parts'])
@pytest.mark.parametrize('n_addends', [1, 2, 3])
@pytest.mark.parametrize('C,tag', CASES)
def test_token_grad_sum_vs_float64(monkeypatch, C, tag, n_addends, with_parts, poison):
    from gedepth_amd import neck_kernels as NK
    dt, pitch, col = DTYPES[tag], C + 32, 16
    guard = _install(monkeypatch, poison)
    addends = [guard.framed(_randn((B, N, C), 41 + k, dt)) for k in range(n_addends)]
    parts = None
    if with_parts:                                                     # level l's rows inside a (B * N_l, C + 32) matrix, from column 16
        wide = [guard.framed(_randn((B * n, pitch), 51 + l, dt)) for l, n in enumerate(ROWS)]
        parts = [w.view(B, n, pitch)[:, :, col:col + C] for w, n in zip(wide, ROWS)]
    got = NK.token_grad_sum(addends, [(w, col) for w in wide] if with_parts else None)
    torch.cuda.synchronize()
    monkeypatch.undo()
    guard.check()
    assert guard.launched == ['ge_token_grad_sum'] and tuple(got.shape) == (B, N, C) and got.dtype == dt
    terms = [a.double().cpu() for a in addends] + ([torch.cat([p.double().cpu() for p in parts], 1)] if with_parts else [])
    ref, mag = sum(terms), sum(t.abs() for t in terms)
    err, bound = (got.double().cpu() - ref).abs(), 2.0 ** -8 * ref.abs() + 2.0 ** -22 * mag
    print(f'token_grad_sum C={C} {tag} {n_addends} addends parts={with_parts}: max err / bound = {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------------------------------------ the neck
def _neck_run(golden, amp, disabled, monkeypatch):
    """One training forward + backward of the tiny neck of tests/golden/hahi.npz (Swin-T widths, 32 x 48 ... 2 x 3 maps, channels-last) ->
    (outputs, {name: gradient}) of the parameters and the five inputs."""
    from gedepth_amd import kernels as K
    from gedepth_amd.depth.models.necks.hahi import HAHIHeteroNeck
    from gedepth_amd.depth.models.utils import to_channels_last
    from oracle.fill import load_filled
    g = golden('hahi')
    chans = [64, 96, 192, 384, 768]
    m = HAHIHeteroNeck(in_channels=chans, out_channels=chans, embedding_dim=512, scales=[1] * 5,
                       positional_encoding=dict(type='SinePositionalEncoding', num_feats=256))
    load_filled(m, 'hahi')
    m = m.cuda().train()
    to_channels_last(m)
    feats = [torch.from_numpy(np.asarray(g[f'in{i}'])).cuda().contiguous(memory_format=CL).requires_grad_() for i in range(5)]
    monkeypatch.setattr(K, 'DISABLED', set(K.DISABLED) | set(disabled))
    monkeypatch.setattr(K, 'FALLBACKS', {})
    torch.manual_seed(7)                                               # the dropout seeds come from the host generator
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
        outs = m(feats)
    loss = sum((o.float() * torch.randn(o.shape, generator=_gen(60 + i)).cuda()).sum() for i, o in enumerate(outs))
    loss.backward()
    torch.cuda.synchronize()
    assert not K.FALLBACKS, K.FALLBACKS
    grads = {n: p.grad.detach().float() for n, p in m.named_parameters() if p.grad is not None}
    grads.update({f'in{i}': f.grad.detach().float() for i, f in enumerate(feats) if f.grad is not None})
    monkeypatch.undo()
    return [o.detach() for o in outs], grads


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def test_neck_level_route_against_the_old_route(monkeypatch, golden):
    """The level route and GE_DISABLE=neck_levels under the same seed.  The forward computes the same values in the same order.

    bf16 autocast (how the model trains): the outputs are ``torch.equal``.  The gradients differ where sums changed: the two fan-ins (one
    fp32 sum and one rounding instead of pairwise sums in the storage type) and the level embedding's gradient (fp32 partials instead of
    ATen's reductions).  Against the fp32 run of the old route: each fan-in is within 2^-8 of the exact sum (one rounding; the old route
    rounds after every pairwise add), and the backward is linear in it, so the level route's relative l2 error may exceed the old route's
    own error against the same reference by at most the two fan-ins in series, 2 * 2^-8.

    fp32: the old route does not repeat its own bits here (its fp32 sampling kernels accumulate with atomics: two runs of it differ by
    ~3e-6 in the outputs), so equality cannot be asked of anything.  Outputs: the tolerance of test_hahi_neck_fixture (rtol 2e-4, atol
    2e-5).  Gradients: only the order of fp32 adds differs, 2^-22 sum|x_k| per fan-in element; with a factor 40 for cancellation in the
    sums and in the linear maps behind them that is 1e-5 relative l2, on top of twice the relative l2 between two fp32 runs of the old
    route (the reference's own scatter, measured in the test).

    Measured on MI355X (the log line prints the largest figures over all gradients): fp32 4.9e-6 against the old route, where two runs of
    the old route differ by 5.2e-5; bf16 largest excess over the old route's error 5.1e-4."""
    out_new32, g_new32 = _neck_run(golden, False, (), monkeypatch)
    out_old32, g_old32 = _neck_run(golden, False, ('neck_levels',), monkeypatch)
    _, g_old32b = _neck_run(golden, False, ('neck_levels',), monkeypatch)
    out_new16, g_new16 = _neck_run(golden, True, (), monkeypatch)
    out_old16, g_old16 = _neck_run(golden, True, ('neck_levels',), monkeypatch)
    for i, (a, b) in enumerate(zip(out_new16, out_old16)):
        assert a.dtype == b.dtype and torch.equal(a, b), f'bf16 output {i}'
    for i, (a, b) in enumerate(zip(out_new32, out_old32)):
        assert a.dtype == b.dtype and bool(((a - b).abs() <= 2e-5 + 2e-4 * b.abs()).all()), f'fp32 output {i}: {float((a - b).abs().max()):.3e}'
    assert set(g_new32) == set(g_old32) == set(g_new16) == set(g_old16) and 'level_embed' in g_new32 and 'in1' in g_new32
    worst32, worst16 = ('', 0.0, 0.0), ('', -1.0)
    for name in sorted(g_old32):
        ref = g_old32[name]
        e32, e_self = _rel_l2(g_new32[name], ref), _rel_l2(g_old32b[name], ref)
        e_new, e_old = _rel_l2(g_new16[name], ref), _rel_l2(g_old16[name], ref)
        worst32 = max(worst32, (name, e32, e_self), key=lambda t: t[1])
        worst16 = max(worst16, (name, e_new - e_old), key=lambda t: t[1])
        assert e32 <= 1e-5 + 2 * e_self, f'fp32 {name}: relative l2 {e32:.3e} against the old route (two runs of the old route: {e_self:.3e})'
        assert e_new <= e_old + 2 * 2.0 ** -8, f'bf16 {name}: relative l2 {e_new:.3e} (old route {e_old:.3e}) against the fp32 old route'
    print(f'neck level route: fp32 largest relative l2 against the old route {worst32[1]:.3e} ({worst32[0]}; two runs of the old route '
          f'{worst32[2]:.3e}); bf16 largest excess over the old route\'s error {worst16[1]:.3e} ({worst16[0]})')

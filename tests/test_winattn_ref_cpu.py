"""tests/winattn_ref.py is right: the float64 core against the CPU oracle and the reference project's fixture, the routed inputs against their
expected gather in every arithmetic, and the hand-written backward of the tolerance model against autograd.  No GPU."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import winattn_ref as R
from oracle import gedepth_oracle as O
from oracle.fill import fill_state_dict

GEOMS = [(2, 3, 5, 3), (1, 7, 7, 3), (1, 8, 15, 6), (2, 13, 6, 12), (1, 14, 21, 24)]      # (B, H, W, nH): those of test_window_attn_gpu.py
SCALE = 32 ** -0.5


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _wrapped(x, hw, P, nH, shift):
    """``core`` between the qkv and proj Linears: the whole of ShiftWindowMSA."""
    qkv = F.linear(x, P['a.w_msa.qkv.weight'], P['a.w_msa.qkv.bias'])
    o = R.core(qkv, P['a.w_msa.qkv.bias'], P['a.w_msa.relative_position_bias_table'], hw[0], hw[1], nH, shift, SCALE)
    return F.linear(o, P['a.w_msa.proj.weight'], P['a.w_msa.proj.bias'])


def _weights(C, nH, salt):
    names = [('a.w_msa.relative_position_bias_table', (169, nH)), ('a.w_msa.qkv.weight', (3 * C, C)), ('a.w_msa.qkv.bias', (3 * C,)),
             ('a.w_msa.proj.weight', (C, C)), ('a.w_msa.proj.bias', (C,))]
    return {k: v.double() for k, v in fill_state_dict(names, salt).items()}


@pytest.mark.parametrize('geom', GEOMS)
@pytest.mark.parametrize('shift', [0, 3])
def test_core_matches_oracle_in_float64(geom, shift):
    B, H, W, nH = geom
    C = nH * 32
    P = _weights(C, nH, 'winattn_ref')
    P['a.w_msa.relative_position_bias_table'] = P['a.w_msa.relative_position_bias_table'] + torch.randn(169, nH, generator=gen(1), dtype=torch.float64)
    x = torch.randn(B, H * W, C, generator=gen(H * 100 + W + shift), dtype=torch.float64)
    go = torch.randn(B, H * W, C, generator=gen(7), dtype=torch.float64)
    got, ref = [], []
    for fn, res in ((lambda xx, PP: _wrapped(xx, (H, W), PP, nH, shift), got), (lambda xx, PP: O.shift_window_msa(xx, (H, W), PP, 'a', nH, shift), ref)):
        Pc = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        xc = x.clone().requires_grad_(True)
        out = fn(xc, Pc)
        out.backward(go)
        res += [out.detach(), xc.grad] + [Pc[k].grad for k in sorted(Pc)]
    for name, a, b in zip(['out', 'dx'] + sorted(P), got, ref):
        assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), (name, (a - b).abs().max().item(), b.abs().max().item())


@pytest.mark.parametrize('tag,hw', [('a', (11, 35)), ('b', (10, 9))])
@pytest.mark.parametrize('shift', [0, 3])
def test_core_matches_reference_fixture(golden, tag, hw, shift):
    """Against outputs of the reference's own ShiftWindowMSA (tests/golden/shift_window_msa.npz), at the fixture's float32 tolerance."""
    g = golden('shift_window_msa')
    spec = json.loads(str(g['spec']))
    P = {'a.' + k: v.double() for k, v in fill_state_dict([(n, s) for n, s in spec], 'shift_window_msa').items()}
    out = _wrapped(torch.from_numpy(np.asarray(g[f'x_{tag}{shift}'])).double(), hw, P, 3, shift)
    ref = torch.from_numpy(np.asarray(g[f'out_{tag}{shift}'])).double()
    assert bool(((out - ref).abs() <= 1e-5 + 1e-4 * ref.abs()).all()), (out - ref).abs().max().item()


def test_tables_are_a_partition_of_the_tokens():
    for H, W in ((3, 5), (8, 15), (13, 6), (14, 21)):
        for shift in (0, 3):
            tok, reg = R.tables(H, W, shift)
            real = tok[tok >= 0]
            assert sorted(real.tolist()) == list(range(H * W))
            assert tok.shape == reg.shape == (-(-H // 7) * -(-W // 7), 49)
            assert int(reg.max()) == (8 if shift else 0)


def _table(nH, seed, magnitude=2.0):
    return (torch.rand(169, nH, generator=gen(seed), dtype=torch.float64) * 2 - 1) * magnitude


@pytest.mark.parametrize('geom', GEOMS)
@pytest.mark.parametrize('shift', [0, 3])
def test_routed_inputs_are_an_exact_gather(geom, shift):
    B, H, W, nH = geom
    r = R.routed_inputs(B, H, W, nH, shift, seed=11, amplitude=8)
    tab = _table(nH, 12)
    assert r['dv'] is not None and r['n_cross'] == 0
    assert torch.equal(r['qkv'], r['qkv'].bfloat16().double()) and torch.equal(r['qkv_bias'], r['qkv_bias'].bfloat16().double())
    C = nH * 32
    v = r['qkv'][:, :, 2 * C:].view(B, H * W, nH, 32)
    assert bool((v.abs().amax(3) == 7).all()) and r['qkv_bias'].abs().max() <= 7                # every tile's amax is exactly 7
    out = R.core(r['qkv'], r['qkv_bias'], tab, H, W, nH, shift, SCALE)
    assert (out - r['out']).abs().max().item() < 1e-100
    for arith in ('f32', 'bf16'):
        o, dqkv, dqb, dtab = R.model(r['qkv'], r['qkv_bias'], tab, r['go'], H, W, nH, shift, SCALE, arith)
        assert torch.equal(o.double(), r['out']), arith
        assert torch.equal(dqkv[:, :, 2 * C:].double(), r['dv']), arith
        assert not bool(dqkv[:, :, :2 * C].any()) and not bool(dtab.any()) and not bool(dqb.any()), arith


@pytest.mark.parametrize('geom', GEOMS)
def test_routed_cross_region_beats_the_mask_only_at_amplitude_8(geom):
    """-100 is added, not a removal: a matching score of 362 in another region still wins; one of 23 does not."""
    B, H, W, nH = geom
    tab = _table(nH, 12)
    r = R.routed_inputs(B, H, W, nH, 3, seed=13, amplitude=8, cross_region=True)
    if geom == (1, 8, 15, 6):         # its real tokens share one region in every window (the other regions hold pads only): nothing to cross
        assert r['n_cross'] == 0 and r['dv'] is not None
        return
    assert r['dv'] is None and r['n_cross'] > 0
    assert (R.core(r['qkv'], r['qkv_bias'], tab, H, W, nH, 3, SCALE) - r['out']).abs().max().item() < 1e-100
    for arith in ('f32', 'bf16'):
        assert torch.equal(R.model(r['qkv'], r['qkv_bias'], tab, r['go'], H, W, nH, 3, SCALE, arith)[0].double(), r['out']), arith
    r2 = R.routed_inputs(B, H, W, nH, 3, seed=13, amplitude=2, cross_region=True)
    assert r2['n_cross'] == r['n_cross']
    # with the mask ignored the match (score 23 against 0) would still take 1 - 48 e^-19 of the weight: the output would be the gather
    o2 = R.core(r2['qkv'], r2['qkv_bias'], tab, H, W, nH, 3, SCALE)
    assert (o2 - r2['out']).abs().max().item() > 1.0


@pytest.mark.parametrize('geom,shift', [((2, 3, 5, 3), 3), ((1, 8, 15, 6), 3), ((1, 14, 21, 24), 0)])
def test_model_backward_matches_autograd_of_core(geom, shift):
    B, H, W, nH = geom
    C = nH * 32
    g = gen(5)
    qkv = torch.randn(B, H * W, 3 * C, generator=g, dtype=torch.float64).requires_grad_(True)
    qb = torch.randn(3 * C, generator=g, dtype=torch.float64).requires_grad_(True)
    tab = torch.randn(169, nH, generator=g, dtype=torch.float64).requires_grad_(True)
    go = torch.randn(B, H * W, C, generator=g, dtype=torch.float64)
    heads = (0, nH - 1)
    for hs in (None, heads):
        for t in (qkv, qb, tab):
            t.grad = None
        out = R.core(qkv, qb, tab, H, W, nH, shift, SCALE, heads=hs)
        _, cols = R.columns(nH, hs)
        out.backward(go[:, :, cols[:len(cols) // 3]])
        o, dqkv, dqb, dtab = R.model(qkv.detach(), qb.detach(), tab.detach(), go, H, W, nH, shift, SCALE, 'f64', heads=hs)
        hl = list(range(nH)) if hs is None else list(hs)
        for name, a, b in (('out', o, out.detach()), ('dqkv', dqkv, qkv.grad[:, :, cols]), ('dqb', dqb, qb.grad[cols]), ('dtab', dtab, tab.grad[:, hl])):
            assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1e-30), (name, hs)
        if hs is not None:                                 # the other heads' inputs get no gradient
            rest = torch.ones(3 * C, dtype=torch.bool)
            rest[cols] = False
            assert not bool(qkv.grad[:, :, rest].any()) and not bool(qb.grad[rest].any())


def test_model_error_levels():
    """The budgets the GPU tests take from ``model``: float32 costs 1e-7, the bf16 roundings 1e-3 on out and d_qkv."""
    B, H, W, nH, shift = 2, 11, 20, 6, 3
    C = nH * 32
    g = gen(3)
    qkv = torch.randn(B, H * W, 3 * C, generator=g).bfloat16().double().requires_grad_(True)
    qb = (0.3 * torch.randn(3 * C, generator=g)).bfloat16().double().requires_grad_(True)
    tab = (0.5 * torch.randn(169, nH, generator=g)).double().requires_grad_(True)
    go = torch.randn(B, H * W, C, generator=g).bfloat16().double()
    out = R.core(qkv, qb, tab, H, W, nH, shift, SCALE)
    out.backward(go)
    ref = (out.detach(), qkv.grad, qb.grad, tab.grad)
    for arith, lo, hi in (('f32', 0.0, 2e-6), ('bf16', 2e-4, 1e-2)):
        got = R.model(qkv.detach(), qb.detach(), tab.detach(), go, H, W, nH, shift, SCALE, arith)
        for name, a, b in zip(('out', 'dqkv'), got, ref):
            l2, mx = R.errors(a, b)
            assert lo <= l2 <= hi and mx <= 2 * hi, (arith, name, l2, mx)

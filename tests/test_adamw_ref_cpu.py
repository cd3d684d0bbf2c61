"""tests/adamw_ref.py against torch itself, in float64 on the CPU: the reference of the optimizer's GPU tests (tests/test_optim_gpu.py) is shown
to be right without any of the code under test."""
import torch

from adamw_ref import adamw_step, clip_coef
from gedepth_amd.mmrt.optim import CosineAnnealingLr


def test_reference_matches_float64_torch_adamw_with_clipping():
    """20 steps of ``clip_grad_norm_`` + ``torch.optim.AdamW`` on float64 parameters: warm-up + cosine lr (a new value every step), a decayed
    and an undecayed group, gradient norms on both sides of ``max_norm``.  Both sides are float64 and differ only in the association of the
    same operations (torch: lerp for m, the clip coefficient applied in place, addcdiv), so every element agrees to 1e-12 relative."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(7, 5), (33,), (3, 2, 3, 3), (1,), (64,)]
    decayed = [True, False, True, False, True]
    params = [torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_(True) for s in shapes]
    b1, b2, eps, wd, max_norm = 0.9, 0.999, 1e-8, 0.01, 9.0
    opt = torch.optim.AdamW([dict(params=[p for p, d in zip(params, decayed) if d], weight_decay=wd),
                             dict(params=[p for p, d in zip(params, decayed) if not d], weight_decay=0.0)],
                            lr=1e-3, betas=(b1, b2), eps=eps, foreach=False)
    sched = CosineAnnealingLr(1e-2, 20, min_lr_ratio=1e-3, warmup='linear', warmup_iters=6, warmup_ratio=1e-2)
    sizes = [p.numel() for p in params]
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])
    p = flat(params).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    decay = torch.cat([torch.full((n,), d) for n, d in zip(sizes, decayed)])
    clipped, lrs = [], set()
    for it in range(20):
        lr = sched.apply(opt, it)
        lrs.add(lr)
        scale = (0.3, 3.0)[it % 2] if it < 18 else 1.0                     # |g| is about 10.5 * scale: 3.2, 32 and 10.5 around max_norm = 9 ...
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * scale for s in shapes]
        if it == 19:                                                       # ... and one step just inside the bound
            total = flat(grads).norm()
            grads = [g * (0.999 * max_norm / total) for g in grads]
        for q, g in zip(params, grads):
            q.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        p, m, v, gn = adamw_step(p, flat(grads), m, v, decay, lr, b1, b2, eps, wd, it + 1, max_norm)
        clipped.append(bool(clip_coef(gn, max_norm) < 1))
        assert abs(float(gn) - float(norm)) <= 1e-12 * float(norm)
        for name, ours, theirs in (('p', p, flat(params)), ('m', m, flat([opt.state[q]['exp_avg'] for q in params])),
                                   ('v', v, flat([opt.state[q]['exp_avg_sq'] for q in params]))):
            err = ((ours - theirs).abs() / theirs.abs().clamp_min(1e-300)).max().item()
            assert err <= 1e-12, (it, name, err)
    assert len(lrs) == 20 and 5 <= sum(clipped) <= 15 and not clipped[19], (clipped, sorted(lrs))


def test_reference_clip_coefficient_edges():
    assert float(clip_coef(3.0, 0.0)) == 1.0                               # max_norm = 0: no clipping
    assert float(clip_coef(0.5, 1.0)) == 1.0
    assert abs(float(clip_coef(4.0, 1.0)) - 1 / (4 + 1e-6)) < 1e-16
    assert float(clip_coef(float('inf'), 1.0)) == 0.0
    assert torch.isnan(clip_coef(float('nan'), 1.0))                       # torch's clamp propagates NaN
    # an explicit grad_norm is used as given (a slice of a larger arena is clipped by the arena's norm)
    one = torch.ones(4, dtype=torch.float64)
    p, m, v, gn = adamw_step(one, one, 0 * one, 0 * one, torch.zeros(4), 0.1, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, grad_norm=10.0)
    assert float(gn) == 10.0 and torch.allclose(m, one * 0.1 / (10 + 1e-6), rtol=1e-15, atol=0)

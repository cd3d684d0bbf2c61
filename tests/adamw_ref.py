"""Float64 AdamW with global-norm gradient clipping on flat tensors: the reference the optimizer tests compare the HIP kernels with
(imported like ``f64ref``).  Plain element-wise torch operations in the order torch documents for ``clip_grad_norm_`` followed by
``torch.optim.AdamW``; nothing here comes from the code under test.  tests/test_adamw_ref_cpu.py holds it against torch itself."""
import torch


def clip_coef(grad_norm, max_norm):
    """``clip_grad_norm_``: min(1, max_norm / (norm + 1e-6)); ``max_norm <= 0`` means no clipping.  A NaN norm gives a NaN coefficient
    (torch clamps, and clamp propagates NaN)."""
    grad_norm = torch.as_tensor(grad_norm, dtype=torch.float64)
    if max_norm <= 0:
        return torch.ones_like(grad_norm)
    return torch.clamp(max_norm / (grad_norm + 1e-6), max=1.0)


def adamw_step(p, g, m, v, decay, lr, b1, b2, eps, wd, t, max_norm, grad_norm=None):
    """One step from the state (p, m, v) with gradient ``g``; ``t`` is the number of this step (1 for the first).  ``decay``: bool / 0-1
    mask of the elements that take weight decay.  ``grad_norm``: the global L2 norm to clip by (default: the norm of ``g``).
    Returns (p, m, v, grad_norm) as new float64 tensors on the device of ``p``."""
    p, g, m, v = (x.detach().double() for x in (p, g, m, v))
    if grad_norm is None:
        grad_norm = g.pow(2).sum().sqrt()
    grad_norm = torch.as_tensor(grad_norm, dtype=torch.float64, device=p.device)
    g = g * clip_coef(grad_norm, max_norm)
    p = torch.where(decay.to(p.device).bool(), p * (1 - lr * wd), p)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / (1 - b2 ** t) ** 0.5 + eps
    p = p - (lr / (1 - b1 ** t)) * (m / denom)
    return p, m, v, grad_norm

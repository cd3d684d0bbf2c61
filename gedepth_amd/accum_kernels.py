"""Wrapper of the gradient accumulation (csrc/accum.hip; include/gedepth_accum.h): ``grad_accum`` writes (``first``) or adds one flat fp32
gradient arena into another and, when given a float64 scalar, adds the squared L2 norm of the result to it in the same pass.  The header
states the arithmetic; ``FusedAdamW.accumulate`` (mmrt/optim.py) is the caller."""
import torch

from . import hip


def grad_accum(acc, grad, first, sumsq=None, n=None):
    """``acc[:n] = grad[:n]`` (``first``) or ``acc[:n] += grad[:n]`` on the current stream, without synchronising; ``sumsq`` (one float64
    on the device, zeroed by the caller) receives ``+= sum(acc[:n] ** 2)`` in float64.  ``n``: all of ``grad`` by default."""
    n = grad.numel() if n is None else int(n)
    if not 0 <= n <= min(acc.numel(), grad.numel()):
        raise ValueError(f'grad_accum: n = {n} with {acc.numel()} accumulator and {grad.numel()} gradient elements')
    if sumsq is not None and sumsq.numel() < 1:
        raise ValueError('grad_accum: sumsq must hold one float64')
    hip.call('ge_grad_accum', hip.ptr(acc, torch.float32, 'acc'), hip.ptr(grad, torch.float32, 'grad'), n, int(bool(first)),
             hip.ptr(sumsq, torch.float64, 'sumsq'), hip.stream())
    return acc

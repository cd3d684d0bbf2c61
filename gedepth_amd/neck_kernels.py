"""Wrappers of the HAHI neck's level-token kernels (csrc/nhwc.hip; include/gedepth_neck.h).  The neck's self-attention runs on one token
matrix (B, N, C) whose N rows are the concatenated levels of the pyramid.  These ops write, read and sum that matrix level by level where
it lives, instead of building it with ``torch.cat`` and taking its gradients apart with copies and pairwise adds:

``bn_act_levels``      BatchNorm + ReLU of every level's pre-BN map straight into the level's rows; the backward reads them in place
``add_rows_levels``    tokens + (sine rows + level embedding), the embedding's gradient from ``level_colsum`` in one read
``token_grad_sum``     up to three dense gradients and one strided part per level summed in fp32 in one pass
``fan_out`` / ``fan_out_levels``   aliases of one tensor whose gradients all arrive at one backward, which is that sum

They launch through ``kernels._launch`` (profiler, bench's kernel list) and live in a module of their own for the reason eval_kernels.py gives."""
import ctypes

import torch

from . import hip
from .kernels import _c, _cl_ok, _es, _f32, _launch, _tag

MAX_LEVELS = 8                     # GE_NECK_MAX_LEVELS of include/gedepth_neck.h
_WS = {}                           # (device, stream, C, K) -> column-sum workspace (launches are stream-ordered)


def _starts(level_rows, n_levels=None):
    """Rows per level -> (host array of n_levels + 1 row starts, n_levels, N); levels past ``len(level_rows)`` are empty."""
    n_levels = len(level_rows) if n_levels is None else n_levels
    if not 1 <= len(level_rows) <= n_levels <= MAX_LEVELS or any(r < 0 for r in level_rows):
        raise ValueError(f'a level table takes 1 .. {MAX_LEVELS} levels of non-negative size, got {tuple(level_rows)} for {n_levels} levels')
    starts, acc = [0], 0
    for l in range(n_levels):
        acc += int(level_rows[l]) if l < len(level_rows) else 0
        starts.append(acc)
    return (ctypes.c_long * len(starts))(*starts), n_levels, acc


def _workspace(device, C, K):
    key = (device, hip.stream(), C, K)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.empty(int(hip.lib().ge_nhwc_workspace(C, K)), device=device, dtype=torch.uint8)
    return ws


def _vec_ok(t):
    vn = 8 if t.dtype == torch.bfloat16 else 4
    return t.is_cuda and t.dtype in (_f32, torch.bfloat16) and t.shape[-1] % vn == 0 and t.shape[-1] // vn <= 256


# ------------------------------------------------------------------------------------------------ BatchNorm + ReLU into level rows
class _BNActLevels(torch.autograd.Function):
    """``torch.cat([tokens(bn_act(x_l)) for l], 1)`` without the cat: level l's kernel writes rows [start_l, start_l + H_l W_l) of every image
    of the (B, N, C) result, and the backward reads the same rows of the incoming gradient.  ``tensors`` = x_0 .. x_{L-1}, then
    (gamma_l, beta_l) per level; ``meta[l]`` = (running_mean, running_var, eps, momentum, slope)."""

    @staticmethod
    def forward(ctx, meta, *tensors):
        L = len(meta)
        xs, wb = tensors[:L], tensors[L:]
        B, C = xs[0].shape[:2]
        rows = [x.shape[2] * x.shape[3] for x in xs]
        N, es, dt = sum(rows), _es(xs[0]), hip.dtype_code(xs[0])
        out = torch.empty(B, N, C, device=xs[0].device, dtype=xs[0].dtype)
        stats = torch.empty(L, 2, C, device=out.device, dtype=_f32)
        ws = torch.empty(int(hip.lib().ge_nhwc_workspace(C, 2)), device=out.device, dtype=torch.uint8)
        saved, start = [], 0
        for l, (x, n) in enumerate(zip(xs, rows)):
            assert _cl_ok(x) and tuple(x.shape[:2]) == (B, C) and x.dtype == out.dtype
            w, b = _c(wb[2 * l].detach().to(_f32)), _c(wb[2 * l + 1].detach().to(_f32))
            rm, rv, eps, momentum, slope = meta[l]
            _launch(f'bn_act_rows_fwd[{B}x{C}x{x.shape[2]}x{x.shape[3]} {_tag(x)}]', 3 * x.numel() * es, 'ge_bn_act_nhwc_fwd_rows', x.data_ptr(),
                    hip.ptr(w), hip.ptr(b), out.data_ptr() + start * C * es, n, N, hip.ptr(stats[l, 0]), hip.ptr(stats[l, 1]), hip.ptr(rm, _f32),
                    hip.ptr(rv, _f32), hip.ptr(ws), B * n, C, eps, momentum, slope, dt, hip.stream())
            saved += [x, w, b]
            start += n
        ctx.save_for_backward(stats, *saved)
        ctx.slopes = [m[4] for m in meta]
        return out

    @staticmethod
    def backward(ctx, d):
        stats, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        L = len(ctx.slopes)
        x0 = saved[0]
        B, C = x0.shape[:2]
        d = _c(d.to(x0.dtype))
        N, es, dt = d.shape[1], _es(x0), hip.dtype_code(x0)
        dwb = torch.empty(L, 2, C, device=d.device, dtype=_f32)
        ws = torch.empty(int(hip.lib().ge_nhwc_workspace(C, 2)), device=d.device, dtype=torch.uint8)
        dxs, start = [], 0
        for l in range(L):
            x, w, b = saved[3 * l:3 * l + 3]
            n = x.shape[2] * x.shape[3]
            dx = torch.empty_like(x)
            _launch(f'bn_act_rows_bwd[{B}x{C}x{x.shape[2]}x{x.shape[3]} {_tag(x)}]', 5 * x.numel() * es, 'ge_bn_act_nhwc_bwd_rows',
                    d.data_ptr() + start * C * es, n, N, x.data_ptr(), hip.ptr(w), hip.ptr(b), hip.ptr(stats[l, 0]), hip.ptr(stats[l, 1]),
                    dx.data_ptr(), hip.ptr(dwb[l, 0]), hip.ptr(dwb[l, 1]), hip.ptr(ws), B * n, C, ctx.slopes[l], dt, hip.stream())
            dxs.append(dx)
            start += n
        return (None, *dxs, *(dwb[l, k] for l in range(L) for k in range(2)))


def bn_act_levels_ok(maps):
    """The pre-BN maps of all levels can go through ``bn_act_levels``: channels-last HIP maps of one dtype, batch and width."""
    x0 = maps[0]
    return (1 <= len(maps) <= MAX_LEVELS and all(_cl_ok(x) and x.dtype == x0.dtype and tuple(x.shape[:2]) == tuple(x0.shape[:2]) for x in maps))


def bn_act_levels(maps, bns, slopes):
    """Training-mode BatchNorm2d ``bns[l]`` + leaky-ReLU(``slopes[l]``) of every channels-last map ``maps[l]`` (B, C, H_l, W_l), returned as the
    token matrix (B, sum H_l W_l, C) of the concatenated levels.  Updates the running statistics and ``num_batches_tracked`` like ``bn_act``;
    output, statistics and gradients carry the bits of ``kernels.bn_act`` per level followed by ``torch.cat``."""
    meta = [(bn.running_mean, bn.running_var, float(bn.eps), float(bn.momentum), float(s)) for bn, s in zip(bns, slopes)]
    out = _BNActLevels.apply(meta, *maps, *(p for bn in bns for p in (bn.weight, bn.bias)))
    for bn in bns:
        bn.num_batches_tracked.add_(1)
    return out


# ------------------------------------------------------------------------------------------------ position add with the level embedding
def level_colsum(x, level_rows, n_levels=None):
    """x (B, N, C) dense -> (n_levels, C) f32: the column sums of every level's rows over the batch, in one read of x."""
    B, N, C = x.shape
    starts, L, total = _starts(level_rows, n_levels)
    assert total == N and x.is_contiguous()
    out = torch.empty(L, C, device=x.device, dtype=_f32)
    _launch(f'level_colsum[{B}x{N}x{C} {_tag(x)}]', x.numel() * _es(x), 'ge_level_colsum', hip.ptr(x, name='x'), B, N, C,
            ctypes.cast(starts, ctypes.c_void_p), L, hip.ptr(out), hip.ptr(_workspace(x.device, C, L)), hip.dtype_code(x), hip.stream())
    return out


class _AddRowsLevels(torch.autograd.Function):

    @staticmethod
    def forward(ctx, tok, pos_rows, emb, level_rows):
        tok = _c(tok)
        B, N, C = tok.shape
        starts, L, total = _starts(level_rows, emb.shape[0])
        assert total == N and tuple(pos_rows.shape) == (N, C) and emb.shape[1] == C
        out = torch.empty_like(tok)
        _launch(f'add_rows_levels[{B}x{N}x{C} {_tag(tok)}]', 2 * tok.numel() * _es(tok) + N * C * 4, 'ge_add_rows_levels', hip.ptr(tok, name='tokens'),
                hip.ptr(pos_rows, _f32, 'pos'), hip.ptr(_c(emb.detach()), _f32, 'emb'), hip.ptr(out), B, N, C, ctypes.cast(starts, ctypes.c_void_p), L,
                hip.dtype_code(tok), hip.stream())
        ctx.level_rows, ctx.n_levels = tuple(level_rows), L
        return out

    @staticmethod
    def backward(ctx, d):
        d_emb = level_colsum(_c(d), ctx.level_rows, ctx.n_levels) if ctx.needs_input_grad[2] else None
        return d, None, d_emb, None


def add_rows_levels(tokens, pos_rows, emb, level_rows):
    """tokens (B, N, C) + (pos_rows (N, C) f32 + emb[level of the row] (rows of the (L, C) f32 embedding)), one pass and one rounding: the
    bits of ``kernels.add_rows(tokens, cat(pos_l + emb_l))``.  Gradient to ``tokens`` (the incoming one) and to ``emb`` (``level_colsum``)."""
    return _AddRowsLevels.apply(tokens, pos_rows, emb, tuple(int(r) for r in level_rows))


# ------------------------------------------------------------------------------------------------ gradient fan-in
def _part_args(part, B, C):
    """A part -> (rows per image, pointer, pitch, column offset, dtype), or None when it has to be packed first.  ``part`` is either a
    (B, N_l, C) view whose rows lie ``pitch`` apart in one dense (B * N_l, pitch) matrix (the pointer is the view's own: column offset 0),
    or ``(matrix, col)``: the dense (B * N_l, pitch) matrix itself and the first of its C columns to read."""
    if isinstance(part, tuple):
        wide, col = part
        assert wide.dim() == 2 and wide.is_contiguous() and wide.shape[0] % B == 0 and 0 <= col and col + C <= wide.shape[1]
        return wide.shape[0] // B, wide.data_ptr(), wide.shape[1], int(col), wide.dtype
    assert part.shape[0] == B and part.shape[2] == C
    n, pitch = part.shape[1], part.stride(1)
    if part.stride(2) != 1 or pitch < C or (B > 1 and part.stride(0) != n * pitch):
        return None
    return n, part.data_ptr(), pitch, 0, part.dtype


def token_grad_sum(addends, parts=None):
    """Sum of up to three dense (B, N, C) tensors and, with ``parts``, of one (B, N_l, C) tensor per level laid side by side along N; fp32
    sum, one rounding, one pass.  A part that is a column range of a wider row matrix is read in place (``_part_args``); ``parts`` alone
    need a (B, N_l, C) view first, which gives the shape."""
    addends = [_c(a) for a in addends]
    ref = addends[0] if addends else parts[0]
    B, C = ref.shape[0], ref.shape[2]
    assert len(addends) <= 3 and _vec_ok(ref) and all(a.shape == ref.shape and a.dtype == ref.dtype for a in addends)
    es, vn = _es(ref), 16 // _es(ref)
    n_parts, ptrs, pitch, col, starts, keep = 0, None, None, None, None, []
    if parts:
        args = []
        for p in parts:
            a = _part_args(p, B, C)
            if a is None or a[1] % 16 or a[2] % vn or a[3] % vn:
                p = p.contiguous()
                keep.append(p)                                         # alive until the launch is queued
                a = (p.shape[1], p.data_ptr(), C, 0, p.dtype)
            assert a[4] == ref.dtype
            args.append(a)
        starts, n_parts, N = _starts([a[0] for a in args])
        ptrs = (ctypes.c_void_p * n_parts)(*(a[1] for a in args))
        pitch = (ctypes.c_long * n_parts)(*(a[2] for a in args))
        col = (ctypes.c_long * n_parts)(*(a[3] for a in args))
    else:
        N = ref.shape[1]
    assert not addends or ref.shape[1] == N
    out = torch.empty(B, N, C, device=ref.device, dtype=ref.dtype)
    a = [hip.ptr(t, name='addend') for t in addends] + [None] * (3 - len(addends))
    cast = lambda arr: None if arr is None else ctypes.cast(arr, ctypes.c_void_p)
    _launch(f'token_grad_sum[{B}x{N}x{C} {_tag(ref)} {len(addends)}{"+parts" if parts else ""}]', (len(addends) + bool(parts) + 1) * out.numel() * es,
            'ge_token_grad_sum', a[0], a[1], a[2], cast(ptrs), cast(pitch), cast(col), cast(starts), n_parts, hip.ptr(out), B, N, C,
            hip.dtype_code(ref), hip.stream())
    return out


class _FanOut(torch.autograd.Function):
    """n aliases of x; the engine hands their gradients to ONE backward, which sums them in one pass instead of pairwise ``add_``."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        return (gs[0] if len(gs) == 1 else token_grad_sum(gs)), None


def fan_out(x, n):
    """x (B, N, C) -> n tensors that alias it, for n consumers (n <= 3)."""
    assert 1 <= n <= 3
    return _FanOut.apply(x, n)


class _FanOutLevels(torch.autograd.Function):
    """x (B, N, C) -> (an alias of x, its per-level row ranges as ``torch.split(x, level_rows, 1)`` gives them); the backward is one
    ``token_grad_sum`` of the alias's gradient and the levels' gradients, each read where its producer left it."""

    @staticmethod
    def forward(ctx, x, level_rows):
        ctx.set_materialize_grads(False)
        ctx.meta = (tuple(x.shape), x.dtype, x.device, level_rows)
        return (x.view_as(x), *x.split(list(level_rows), 1))

    @staticmethod
    def backward(ctx, g, *parts):
        (B, N, C), dtype, device, level_rows = ctx.meta
        if all(p is None for p in parts):
            return g, None
        parts = [torch.zeros(B, n, C, device=device, dtype=dtype) if p is None else p for p, n in zip(parts, level_rows)]
        return token_grad_sum([] if g is None else [g], parts), None


def fan_out_levels(x, level_rows):
    return _FanOutLevels.apply(x, tuple(int(r) for r in level_rows))

"""Red zones and poisoned buffers for the tests of the HIP wrappers (imported like ``f64ref``; no conftest, no start-up hook).

The wrappers take every output, gradient and workspace from ``torch.empty`` / ``torch.zeros`` (and their ``*_like`` forms).  A recycled block
of the caching allocator is mapped and mostly zero, so a kernel that writes a little past a buffer, leaves part of an output unwritten or
reads a workspace before writing it passes a value test.  ``Guard`` replaces the ``torch`` global of a module with a proxy whose allocators
carve every tensor out of the middle of a larger ``uint8`` buffer that is filled with a poison byte:

    [ guard | alignment pad | interior (the tensor) | round-up to 256 B | guard ]      all of it poison before the tensor is handed out

* ``check()``: every byte outside the interior still holds the poison byte (an overrun of up to ``guard`` bytes on either side).
* two poison bytes, ``0xFF`` (bf16 / fp32 NaN, integer -1) and ``0x7F`` (about 3.4e38 in both float types, a huge positive integer): a read of
  an unwritten or out-of-range element that reaches a result shows up as NaN / 1e38 in the value comparison, or as a result that differs
  between the two runs.
* ``poisoned()`` / ``unwritten()``: an element of an ``empty`` allocation that holds the poison pattern under BOTH bytes at the same position
  was never stored (one run alone can collide with a real value).
* ``framed(tensor)``: the same frame around a copy of a test input, so that an out-of-range READ picks up poison.
* the launch log: the names of the library entry points called while installed.

What this method cannot see: an overrun that lands beyond the guard (1 MiB each side by default), and an out-of-range read whose value is
discarded or masked before it reaches a result.  The module knows nothing about the GPU: it frames whatever device an allocation names, CPU
included, which is how tests/test_memguard_cpu.py tests it.
"""
import linecache
import os
import sys

import torch

GUARD = 1 << 20
ALIGN = 256
POISONS = (0xFF, 0x7F)
_HERE = os.path.abspath(__file__)
_real = {n: getattr(torch, n) for n in ('empty', 'zeros', 'empty_like', 'zeros_like')}      # bound before any proxy can shadow them


def _round_up(n, m):
    return (n + m - 1) // m * m


def _call_site():
    """(file, line, source text) of the nearest caller outside this module."""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return ('?', 0, '')
    return (f.f_code.co_filename, f.f_lineno, linecache.getline(f.f_code.co_filename, f.f_lineno).strip())


def _dense_strides(t):
    """Strides of ``t`` if it is non-overlapping and dense, else None."""
    dims = sorted((d for d in range(t.dim()) if t.shape[d] != 1), key=lambda d: t.stride(d))
    expect = 1
    for d in dims:
        if t.stride(d) != expect:
            return None
        expect *= t.shape[d]
    return tuple(t.stride())


def _preserved_strides(t):
    """What ``torch.preserve_format`` gives a new tensor like ``t``: its strides if it is dense, dense strides in the same dimension order if it
    is a strided slice, contiguous strides if it overlaps itself (an expanded view)."""
    dense = _dense_strides(t)
    if dense is not None:
        return dense
    if any(t.stride(d) == 0 and t.shape[d] > 1 for d in range(t.dim())):
        return _strides_for(t.shape, None)
    strides, acc = [0] * t.dim(), 1
    for d in sorted(range(t.dim()), key=lambda d: (t.stride(d), -d)):
        strides[d] = acc
        acc *= max(int(t.shape[d]), 1)
    return tuple(strides)


def _strides_for(shape, memory_format):
    n = len(shape)
    if memory_format in (None, torch.contiguous_format, torch.preserve_format):
        order = list(range(n))
    elif memory_format == torch.channels_last:
        assert n == 4, 'channels_last needs a 4-D shape'
        order = [0, 2, 3, 1]
    elif memory_format == torch.channels_last_3d:
        assert n == 5, 'channels_last_3d needs a 5-D shape'
        order = [0, 2, 3, 4, 1]
    else:
        raise TypeError(f'memguard: memory_format {memory_format} is not handled')
    strides, acc = [0] * n, 1
    for d in reversed(order):
        strides[d] = acc
        acc *= max(int(shape[d]), 1)
    return tuple(strides)


class Frame:
    """One framed allocation: ``raw`` the whole uint8 buffer, the interior at bytes [lo, lo + nbytes), ``tensor`` the view handed out."""

    def __init__(self, raw, lo, nbytes, tensor, site, kind, poison):
        self.raw, self.lo, self.nbytes, self.tensor, self.site, self.kind, self.poison = raw, lo, nbytes, tensor, site, kind, poison
        self.shape, self.dtype = tuple(tensor.shape), tensor.dtype

    def describe(self):
        return f'{os.path.basename(self.site[0])}:{self.site[1]} `{self.site[2][:90]}` {self.kind} {self.shape} {self.dtype} on {self.raw.device}'

    def interior_bytes(self):
        return self.raw[self.lo:self.lo + self.nbytes]

    def poisoned(self):
        """Flat bool tensor over the interior's elements (storage order): True where every byte of the element is the poison byte."""
        es = self.tensor.element_size()
        return (self.interior_bytes().view(-1, es) == self.poison).all(1)


class _Proxy:
    """Stands in for the ``torch`` module in another module's globals: the four allocators are framed, everything else is ``torch``'s."""

    def __init__(self, guard):
        object.__setattr__(self, '_guard', guard)

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        return self._guard._new(size, kw, 'empty')

    def zeros(self, *size, **kw):
        return self._guard._new(size, kw, 'zeros')

    def empty_like(self, t, **kw):
        return self._guard._like(t, kw, 'empty')

    def zeros_like(self, t, **kw):
        return self._guard._like(t, kw, 'zeros')


class Guard:

    def __init__(self, poison, guard=GUARD):
        assert 0 <= poison <= 255 and guard >= 0 and guard % ALIGN == 0
        self.poison, self.guard = int(poison), int(guard)
        self.frames = []                   # recorded since the last check()
        self.launched = []                 # entry points that went through ``call`` of the wrapped binding, in order
        self.direct = []                   # entry points called on the library handle itself (size queries, predicates, direct launches)
        self.proxy = _Proxy(self)
        self._busy = False

    # ------------------------------------------------------------------ allocation
    def _carve(self, shape, strides, dtype, device, kind, site, requires_grad=False):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        es = _real['empty'](0, dtype=dtype).element_size()
        nbytes = numel * es
        busy, self._busy = self._busy, True           # allocations of the harness itself are never framed again by the copy hooks
        try:
            raw = _real['empty'](self.guard + ALIGN + _round_up(nbytes, ALIGN) + self.guard, dtype=torch.uint8, device=device)
            raw.fill_(self.poison)
            lo = self.guard + (-(raw.data_ptr() + self.guard)) % ALIGN
            flat = raw[lo:lo + nbytes].view(dtype)
            if kind == 'zeros':
                flat.zero_()
            t = flat.as_strided(shape, strides) if numel else flat.view(shape)
        finally:
            self._busy = busy
        if requires_grad:
            t.requires_grad_(True)
        self.frames.append(Frame(raw, lo, nbytes, t, site, kind, self.poison))
        return t

    def _new(self, size, kw, kind):
        site = _call_site()
        kw = dict(kw)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        if 'size' in kw:
            size = tuple(kw.pop('size'))
        dtype = kw.pop('dtype', None) or torch.get_default_dtype()
        device = kw.pop('device', None)
        memory_format = kw.pop('memory_format', None)
        requires_grad = kw.pop('requires_grad', False)
        if kw.pop('pin_memory', False) or kw.pop('out', None) is not None or kw.pop('layout', torch.strided) != torch.strided:
            raise TypeError('memguard: pinned / out= / non-strided allocations are not framed')
        if kw:
            raise TypeError(f'memguard: allocator arguments {sorted(kw)} are not handled')
        return self._carve(size, _strides_for(size, memory_format), dtype, device, kind, site, requires_grad)

    def _like(self, t, kw, kind):
        site = _call_site()
        kw = dict(kw)
        dtype = kw.pop('dtype', None) or t.dtype
        device = kw.pop('device', None) or t.device
        memory_format = kw.pop('memory_format', torch.preserve_format)
        requires_grad = kw.pop('requires_grad', False)
        if kw.pop('layout', torch.strided) != torch.strided or kw.pop('pin_memory', False):
            raise TypeError('memguard: pinned / non-strided allocations are not framed')
        if kw:
            raise TypeError(f'memguard: allocator arguments {sorted(kw)} are not handled')
        strides = _preserved_strides(t) if memory_format == torch.preserve_format else _strides_for(t.shape, memory_format)
        return self._carve(t.shape, strides, dtype, device, kind, site, requires_grad)

    def framed(self, t, site=None):
        """A copy of ``t`` (same shape, strides if dense, dtype, device) inside a poisoned frame: for inputs made by a test."""
        site = site or _call_site()
        with torch.no_grad():
            strides = _dense_strides(t) or _strides_for(t.shape, None)
            out = self._carve(t.shape, strides, t.dtype, t.device, 'input', site)
            busy, self._busy = self._busy, True
            try:
                out.copy_(t)
            finally:
                self._busy = busy
        return out

    # ------------------------------------------------------------------ installation
    def install(self, monkeypatch, modules, binding=None, frame_copies_on=None):
        """``modules``: their ``torch`` global becomes the proxy (looked up at call time, so autograd backward passes are covered).
        ``binding``: the module that binds the native library (``call(name, *args)`` and ``lib()``): both are wrapped to log entry-point names.
        ``frame_copies_on``: a device; while installed, ``Tensor.to`` / ``.cuda`` / ``.contiguous`` results that are new tensors on that device
        and do not take part in autograd are re-homed into frames — the way inputs of a test body written without the harness get framed."""
        for m in modules:
            monkeypatch.setattr(m, 'torch', self.proxy)
        if binding is not None:
            real_call, real_lib = binding.call, binding.lib

            def call(name, *args):
                self.launched.append(name)
                return real_call(name, *args)

            class _Lib:
                def __getattr__(_, name):
                    fn = getattr(real_lib(), name)
                    if not name.startswith('ge_'):
                        return fn

                    def logged(*a):
                        self.direct.append(name)
                        return fn(*a)
                    return logged
            lib = _Lib()
            monkeypatch.setattr(binding, 'call', call)
            monkeypatch.setattr(binding, 'lib', lambda: lib)
        if frame_copies_on is not None:
            dev = torch.device(frame_copies_on)
            for name in ('to', 'cuda', 'contiguous'):
                monkeypatch.setattr(torch.Tensor, name, self._copy_hook(getattr(torch.Tensor, name), dev))
        return self

    def _copy_hook(self, real, dev):
        def hooked(t, *a, **kw):
            out = real(t, *a, **kw)
            if (self._busy or out is t or not isinstance(out, torch.Tensor) or out.requires_grad or out.layout != torch.strided or out.numel() == 0
                    or out.device.type != dev.type or (dev.index is not None and out.device.index != dev.index) or out.is_quantized):
                return out
            if out.data_ptr() == t.data_ptr() and out.device == t.device:             # a view / alias, not a copy
                return out
            if _dense_strides(out) is None:
                return out
            site = _call_site()
            res = self.framed(out, site)
            if isinstance(out, torch.nn.Parameter):
                res = torch.nn.Parameter(res, requires_grad=False)
            return res
        return hooked

    # ------------------------------------------------------------------ checks
    def check(self):
        """Every guard byte of every frame recorded since the last check still equals the poison byte.  Returns the frames it looked at."""
        frames, self.frames = self.frames, []
        if any(f.raw.is_cuda for f in frames):
            torch.cuda.synchronize()
        busy, self._busy = self._busy, True
        try:
            dirty = []
            by_dev = {}
            for f in frames:
                by_dev.setdefault(f.raw.device, []).append(f)
            for dev, fs in by_dev.items():
                counts = torch.stack([(f.raw[:f.lo] != f.poison).sum() + (f.raw[f.lo + f.nbytes:] != f.poison).sum() for f in fs]).cpu().tolist()
                dirty += [f for f, c in zip(fs, counts) if c]
            reports = []
            for f in dirty:
                for side, seg, base in (('before', f.raw[:f.lo], -f.lo), ('after', f.raw[f.lo + f.nbytes:], 0)):
                    idx = (seg != f.poison).nonzero().flatten()
                    if idx.numel():
                        first, last = int(idx[0]) + base, int(idx[-1]) + base
                        where = (f'bytes {first} .. {last} relative to the interior start' if side == 'before'
                                 else f'bytes +{first} .. +{last} past the interior end')
                        reports.append(f'{f.describe()}: {idx.numel()} guard bytes changed {side} the tensor ({where}; element size {f.tensor.element_size()})')
        finally:
            self._busy = busy
        assert not reports, 'red zone overwritten:\n  ' + '\n  '.join(reports[:12])
        return frames


def poisoned(tensor, poison):
    """Bool tensor of ``tensor``'s shape: True where the element's bytes all equal ``poison`` (for a tensor an op returned)."""
    t = tensor.detach()
    flat = t.contiguous().view(-1).view(torch.uint8).view(-1, t.element_size())
    return (flat == poison).all(1).view(t.shape)


def unwritten(mask_a, mask_b):
    """Positions that held the poison pattern under both poison bytes: never stored."""
    return mask_a.cpu() & mask_b.cpu()


def assert_written(mask_a, mask_b, what=''):
    bad = unwritten(mask_a, mask_b).flatten().nonzero().flatten()
    assert bad.numel() == 0, (f'{what}: {bad.numel()} of {mask_a.numel()} elements were never written (they hold the poison pattern under both '
                              f'poison bytes); first flat index {int(bad[0])}, last {int(bad[-1])}')

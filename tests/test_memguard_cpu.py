"""tests/memguard.py catches what it claims, shown on CPU tensors with small fake "ops" run through a throw-away module whose ``torch``
global is the harness's proxy; and the NaN-strict ``close()`` of tests/test_kernels_gpu.py."""
import linecache
import types

import pytest
import torch

import memguard

SMALL = 4096                                          # guard width of these tests (the default 1 MiB works the same, slower)


def _module(src):
    m = types.ModuleType('memguard_fake_ops')
    m.torch = torch
    name = '<memguard_fake_ops>'
    linecache.cache[name] = (len(src), None, src.splitlines(True), name)          # so that a call site can be quoted
    exec(compile(src, name, 'exec'), m.__dict__)
    return m


OPS = '''
def good(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    return out

def store_before(x):
    out = torch.empty(x.shape, dtype=x.dtype)
    out.copy_(x * 2)
    out.as_strided((1,), (1,), out.storage_offset() - 3).fill_(1.0)          # element -3: inside the frame the harness owns
    return out

def store_after(x):
    out = torch.empty(x.shape, dtype=x.dtype)
    out.copy_(x * 2)
    out.as_strided((1,), (1,), out.storage_offset() + out.numel() + 5).fill_(1.0)
    return out

def last_row_unwritten(x):
    out = torch.empty_like(x)
    out[:-1].copy_(x[:-1] * 2)
    return out

def reads_workspace_first(x):
    ws = torch.empty(16, dtype=torch.float32)
    total = ws.sum()                                    # read before write
    ws.fill_(0.0)
    return x.sum() + total

def host_staging():
    return torch.empty(10, dtype=torch.int32).pin_memory()
'''


@pytest.fixture
def ops():
    return _module(OPS)


def _install(monkeypatch, ops, poison):
    return memguard.Guard(poison, guard=SMALL).install(monkeypatch, [ops])


@pytest.mark.parametrize('poison', memguard.POISONS)
def test_correct_op_passes(monkeypatch, ops, poison):
    g = _install(monkeypatch, ops, poison)
    x = g.framed(torch.arange(12.0).view(3, 4))
    y = ops.good(x)
    frames = g.check()
    assert [f.kind for f in frames] == ['input', 'empty'] and frames[1].site[2].startswith('out = torch.empty_like')
    assert torch.equal(y, torch.arange(12.0).view(3, 4) * 2) and not bool(memguard.poisoned(y, poison).any())
    assert g.check() == []                               # the record restarts after a check


@pytest.mark.parametrize('poison', memguard.POISONS)
@pytest.mark.parametrize('op,side,where', [('store_before', 'before', 'bytes -12 .. -'), ('store_after', 'after', 'bytes +20 .. +')])
def test_store_outside_the_output_is_reported_with_side_and_offset(monkeypatch, ops, poison, op, side, where):
    g = _install(monkeypatch, ops, poison)
    getattr(ops, op)(torch.ones(3, 4))
    with pytest.raises(AssertionError) as e:
        g.check()
    msg = str(e.value)
    assert f'changed {side} the tensor' in msg and where in msg and '(3, 4) torch.float32' in msg and 'out = torch.empty(x.shape' in msg, msg
    assert ('before' if side == 'after' else 'after') + ' the tensor' not in msg


def test_unwritten_last_row_is_caught_across_the_two_poisons(monkeypatch, ops):
    masks = {}
    for poison in memguard.POISONS:
        with monkeypatch.context() as mp:
            g = _install(mp, ops, poison)
            x = torch.ones(3, 4)
            if poison == 0x7F:
                x[0, 0] = torch.tensor([poison] * 4, dtype=torch.uint8).view(torch.float32).item() / 2    # 2 x == the poison value: a collision in ONE run
            y = ops.last_row_unwritten(x)
            g.check()
            masks[poison] = memguard.poisoned(y, poison)
    assert bool(masks[0x7F][0, 0])                                              # the single-run collision is there ...
    bad = memguard.unwritten(*masks.values())
    assert bad.tolist() == [[False] * 4, [False] * 4, [True] * 4]              # ... and does not count; the unwritten row does
    with pytest.raises(AssertionError, match='4 of 12 elements were never written'):
        memguard.assert_written(*masks.values(), what='last_row_unwritten')
    memguard.assert_written(masks[0xFF][:2], masks[0x7F][:2])


def test_read_before_write_differs_between_the_poisons(monkeypatch, ops):
    res = []
    for poison in memguard.POISONS:
        with monkeypatch.context() as mp:
            g = _install(mp, ops, poison)
            res.append(ops.reads_workspace_first(torch.ones(4)))
            g.check()
    assert torch.isnan(res[0]) and not torch.isfinite(res[1]) or res[1] > 1e38          # NaN under 0xFF, 16 x 3.4e38 (overflow) under 0x7F
    assert not torch.equal(res[0], res[1])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.uint8, torch.float64])
def test_allocations_keep_shape_strides_dtype_flags_and_alignment(dtype):
    g = memguard.Guard(0xFF, guard=SMALL)
    P = g.proxy
    cl = torch.channels_last
    a = P.empty((2, 8, 3, 5), dtype=dtype, memory_format=cl)
    ref = torch.empty((2, 8, 3, 5), dtype=dtype, memory_format=cl)
    assert a.shape == ref.shape and a.stride() == ref.stride() and a.dtype == dtype
    assert a.is_contiguous(memory_format=cl) and not a.is_contiguous()
    b = P.empty(2, 3, 5, dtype=dtype)
    assert b.is_contiguous() and b.stride() == (15, 5, 1)
    z = P.zeros(7, dtype=dtype)
    assert z.shape == (7,) and not bool(z.any())
    for like, src in ((P.empty_like, a), (P.zeros_like, a), (P.empty_like, b), (P.empty_like, a.permute(0, 2, 3, 1)), (P.empty_like, a[:, :1]),
                      (P.empty_like, b[:, :, ::2])):
        t, want = like(src), torch.empty_like(src)
        assert t.shape == want.shape and t.stride() == want.stride() and t.dtype == want.dtype
        assert t.is_contiguous() == want.is_contiguous() and t.is_contiguous(memory_format=cl) == want.is_contiguous(memory_format=cl) if t.dim() == 4 else True
    assert P.empty_like(a, dtype=torch.float32).dtype == torch.float32 and not bool(P.zeros_like(a).any())
    frames = g.check()
    assert all(f.tensor.data_ptr() % memguard.ALIGN == 0 for f in frames)
    assert all(f.lo >= SMALL and f.raw.numel() - f.lo - f.nbytes >= SMALL for f in frames)
    assert bool(frames[0].poisoned().all()) and not bool(frames[2].poisoned().any())        # empty: all poison; zeros: none
    assert P.float32 is torch.float32 and P.nn is torch.nn                                    # everything else is torch's


def test_host_staging_tensor_can_be_pinned(monkeypatch, ops):
    g = _install(monkeypatch, ops, 0x7F)
    try:
        torch.empty(1).pin_memory()
    except RuntimeError:
        pytest.skip('pinned host memory is not available here')
    t = ops.host_staging()
    assert t.shape == (10,) and t.dtype == torch.int32 and t.is_pinned()
    g.check()


def test_copy_hooks_frame_new_tensors_of_a_test_body(monkeypatch):
    g = memguard.Guard(0xFF, guard=SMALL).install(monkeypatch, [], frame_copies_on='cpu')
    x = torch.arange(24.0).view(2, 3, 4)
    y = x.to(torch.bfloat16)                            # a new tensor: framed
    w = x.requires_grad_(True).to(torch.float64)        # part of the autograd graph: left alone
    v = x.detach().permute(0, 2, 1).contiguous()
    assert x.detach().to(torch.float32).data_ptr() == x.data_ptr()
    frames = g.check()
    assert [f.kind for f in frames] == ['input', 'input'] and frames[0].tensor is y and frames[1].tensor is v
    assert torch.equal(y.float(), x.detach()) and w.grad_fn is not None and torch.equal(v, x.detach().permute(0, 2, 1))


def test_launch_log_records_entry_points(monkeypatch):
    calls = []
    binding = types.SimpleNamespace(call=lambda name, *a: calls.append((name, a)), lib=lambda: types.SimpleNamespace(ge_size=lambda n: 2 * n, other=5))
    g = memguard.Guard(0xFF, guard=SMALL).install(monkeypatch, [], binding=binding)
    binding.call('ge_thing_fwd', 1, 2)
    assert binding.lib().ge_size(4) == 8 and binding.lib().other == 5
    assert g.launched == ['ge_thing_fwd'] and g.direct == ['ge_size'] and calls == [('ge_thing_fwd', (1, 2))]


def test_close_is_nan_and_inf_strict():
    from test_kernels_gpu import close
    ref = torch.tensor([1.0, 2.0, 3.0])
    close(ref.clone(), ref)
    close(ref + 1e-6, ref)
    for bad in (float('nan'), float('inf'), float('-inf')):
        got = ref.clone()
        got[1] = bad
        with pytest.raises(AssertionError, match='1 non-finite'):
            close(got, ref, what='x')
    with pytest.raises(AssertionError):
        close(ref + 1.0, ref)

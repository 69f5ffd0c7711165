"""The red-zone harness (tests/_redzone.py) checked on CPU tensors: a check that cannot fail checks nothing.  Everything here stays on the CPU;
the arena's device is "cpu", so the proxy carves what is asked for with device="cpu"."""
import sys
import types

import pytest
import torch

import _redzone as rz

MiB = 1 << 20


def _arena(n=4 * MiB):
    a = rz.Arena(n, "cpu")
    return a, rz.TorchProxy(a)


def _offset(a, t):
    return t.data_ptr() - a.base


def test_clean_run_reports_nothing():
    a, tp = _arena()
    x = tp.empty(299, dtype=torch.float32, device="cpu"); tp.zeros(7, 3, dtype=torch.int32, device="cpu"); tp.empty(0, dtype=torch.float16, device="cpu")
    x[:] = 1.0                                               # a store up to the last element is no overrun
    assert a.check() == []


@pytest.mark.parametrize("dtype,n", [(torch.float32, 299), (torch.float16, 301), (torch.uint8, 13), (torch.int32, 5)])
def test_one_byte_and_one_element_past_the_end(dtype, n):
    a, tp = _arena()
    tp.empty(64, dtype=torch.float32, device="cpu")
    x = tp.empty(n, dtype=dtype, device="cpu"); line = sys._getframe().f_lineno
    tp.empty(64, dtype=torch.float32, device="cpu")
    end = _offset(a, x) + n * dtype.itemsize
    a.buf[end] = 0x5A                                        # one byte
    assert a.check() == [(f"tests/test_redzone_cpu.py:{line}", (n,), dtype, 0, 1)]
    a.buf[end] = rz.fill_byte(dtype)
    assert a.check() == []
    a.buf[end:end + dtype.itemsize] = 0x5A                   # one element
    assert a.check() == [(f"tests/test_redzone_cpu.py:{line}", (n,), dtype, 0, dtype.itemsize)]


def test_store_that_starts_4k_past_the_end():
    a, tp = _arena()
    x = tp.zeros(10, 10, dtype=torch.float32, device="cpu"); line = sys._getframe().f_lineno
    tp.zeros(3, dtype=torch.int64, device="cpu")
    end = _offset(a, x) + 400
    a.buf[end + 4096:end + 4096 + 8] = 0
    assert a.check() == [(f"tests/test_redzone_cpu.py:{line}", (10, 10), torch.float32, 4096, 8)]


def test_store_before_the_start_goes_to_the_previous_buffers_zone():
    a, tp = _arena()
    x = tp.empty(5, dtype=torch.int32, device="cpu"); line = sys._getframe().f_lineno
    y = tp.empty(100, dtype=torch.float32, device="cpu")
    a.buf[_offset(a, y) - 1] = 7                             # the byte in front of y: the last byte of x's zone (zero-filled, x is an integer buffer)
    (site, shape, dtype, off, cnt), = a.check()
    assert (site, shape, dtype, cnt) == (f"tests/test_redzone_cpu.py:{line}", (5,), torch.int32, 1)
    assert off == _offset(a, y) - 1 - (_offset(a, x) + 20) and off >= rz.ZONE - 1


def test_store_before_the_first_buffer():
    a, tp = _arena()
    x = tp.empty(5, dtype=torch.float32, device="cpu"); line = sys._getframe().f_lineno
    a.buf[_offset(a, x) - 4:_offset(a, x)] = 0
    assert a.check() == [(f"tests/test_redzone_cpu.py:{line}", (5,), torch.float32, -4, 4)]


def test_the_last_zone_is_a_mebibyte():
    a, tp = _arena()
    x = tp.empty(5, dtype=torch.float32, device="cpu")
    a.buf[_offset(a, x) + 20 + MiB - 1] = 0
    assert [b[3:] for b in a.check()] == [(MiB - 1, 1)]


def test_empty_is_poisoned_zeros_are_zero_and_zones_take_the_buffers_fill():
    a, tp = _arena()
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        e = tp.empty(3, 5, dtype=dt, device="cpu")
        assert e.shape == (3, 5) and e.dtype == dt and bool(torch.isnan(e).all())
        assert bool(torch.isnan(tp.empty_like(e)).all())
    e8 = tp.empty(7, dtype=torch.uint8, device="cpu")
    assert bool((e8 == 0xFF).all())                          # e4m3 NaN (S.1111.111)
    if hasattr(torch, "float8_e4m3fn"):
        assert bool(torch.isnan(e8.view(torch.float8_e4m3fn).float()).all())
    for dt in (torch.int32, torch.int64, torch.int16, torch.bool):
        i = tp.empty(9, dtype=dt, device="cpu")
        assert bool((i == 0).all())
        end = _offset(a, i) + 9 * dt.itemsize
        assert bool((a.buf[end:end + rz.ZONE] == 0).all())
    z = tp.zeros(4, 4, dtype=torch.float32, device="cpu")
    end = _offset(a, z) + 64
    assert bool((z == 0).all()) and bool((a.buf[end:end + rz.ZONE] == 0xFF).all())
    assert bool((tp.zeros_like(z) == 0).all()) and bool((tp.ones(3, dtype=torch.float16, device="cpu") == 1).all())
    f = tp.full((2, 3), 2.5, dtype=torch.float32, device="cpu")
    assert bool((f == 2.5).all()) and bool((tp.full_like(f, 7.0) == 7.0).all()) and bool((tp.ones_like(f) == 1).all())
    assert tp.full((2,), 3, device="cpu").dtype == torch.int64 and tp.full((2,), True, device="cpu").dtype == torch.bool
    for make in (tp.empty, tp.zeros, tp.ones):                # no dtype: the default type, as torch's own
        assert make(2, 3, device="cpu").dtype == torch.float32 and make((2, 3), device="cpu").shape == (2, 3)
    assert tp.full((2,), 1.5, device="cpu").dtype == torch.float32 and tp.randn(2, device="cpu").dtype == torch.float32
    assert a.check() == []


def test_alignment_is_256_absolute_and_the_end_is_exact():
    a, tp = _arena()
    assert a.bufs == []
    sizes = [(torch.uint8, 1), (torch.uint8, 3), (torch.float16, 7), (torch.uint8, 255), (torch.float32, 299), (torch.uint8, 257), (torch.int16, 1)]
    ts = [tp.empty(n, dtype=dt, device="cpu") for dt, n in sizes]
    prev_end = 0
    for (dt, n), t, b in zip(sizes, ts, a.bufs):
        assert t.data_ptr() % 256 == 0                       # the absolute address, whatever the arena's own base is
        start = _offset(a, t)
        assert (b[0], b[1]) == (start, start + n * dt.itemsize)          # no rounding of the end
        assert rz.ZONE <= start - prev_end < rz.ZONE + 256
        a.buf[b[1]] = 1                                      # the first byte behind the last element is zone already
        assert [(o[1], o[3]) for o in a.check()] == [((n,), 0)]
        a.buf[b[1]] = b[2]
        prev_end = b[1]
    assert a.check() == []


def test_views_keep_the_arena_alive_and_like_keeps_strides():
    a, tp = _arena()
    x = tp.zeros(4, 6, dtype=torch.float32, device="cpu")
    xt = x.t()
    y = tp.empty_like(xt)
    assert y.shape == xt.shape and y.stride() == xt.stride() and a.contains(y.data_ptr())
    s = tp.empty_strided((3, 4), (8, 1), dtype=torch.float32, device="cpu")
    assert s.stride() == (8, 1) and a.bufs[-1][1] - a.bufs[-1][0] == 20 * 4 and not y._is_view() and not s._is_view()
    del a, tp
    x += 1
    assert bool((x == 1).all())


def test_carved_tensors_are_no_views_for_autograd():
    """outputs and saved tensors of a custom Function come from the arena; carving and filling more buffers afterwards must not count as
    an in-place change of them"""
    a, tp = _arena()

    class Twice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            y = tp.empty_like(x); z = tp.empty(x.shape, dtype=x.dtype, device="cpu")
            y.copy_(2 * x); z.copy_(3 * x)
            ctx.save_for_backward(y)
            return y, z

        @staticmethod
        def backward(ctx, gy, gz):
            (y,) = ctx.saved_tensors
            return 2 * gy + 3 * gz + 0 * y

    x = tp.tensor([1.0, 2.0, 3.0], device="cpu", requires_grad=True)
    y, z = Twice.apply(x)
    assert not y._is_view() and not z._is_view() and not x._is_view() and a.contains(y.data_ptr()) and a.contains(z.data_ptr())
    tp.zeros(5, device="cpu"); tp.full((3,), 1.0, device="cpu")
    (y.sum() + z.sum()).backward()
    assert x.grad.tolist() == [5.0, 5.0, 5.0] and a.check() == []


def test_values_come_from_torch_unchanged():
    a, tp = _arena()
    g1 = torch.Generator().manual_seed(5); g2 = torch.Generator().manual_seed(5)
    assert torch.equal(tp.randn(3, 5, generator=g1, device="cpu"), torch.randn(3, 5, generator=g2))
    assert torch.equal(tp.rand(7, generator=g1, device="cpu"), torch.rand(7, generator=g2))
    t = tp.tensor([[1.5, 2.0]], dtype=torch.float16, device="cpu", requires_grad=True)
    assert t.requires_grad and t.is_leaf and a.contains(t.data_ptr()) and t.tolist() == [[1.5, 2.0]]
    assert tp.arange(5, device="cpu").tolist() == [0, 1, 2, 3, 4] and a.contains(tp.arange(5, device="cpu").data_ptr())
    assert not a.contains(tp.tensor([1.0]).data_ptr()) and not a.contains(tp.zeros(3).data_ptr())      # no device asked for: torch's own
    assert a.check() == []


def test_exhausted_arena_raises():
    a, tp = _arena(2 * MiB)
    tp.empty(MiB // 2, dtype=torch.uint8, device="cpu")
    with pytest.raises(rz.ArenaExhausted):
        tp.empty(MiB // 2, dtype=torch.uint8, device="cpu")                # the last zone would fall below 1 MiB
    assert len(a.bufs) == 1
    with pytest.raises(rz.ArenaExhausted):
        rz.Arena(MiB, "cpu")


def test_a_factory_that_is_not_overridden_raises():
    a, tp = _arena()
    with pytest.raises(RuntimeError, match="not a factory the red-zone proxy carves"):
        tp.eye(3, device="cpu")
    with pytest.raises(RuntimeError, match="not a factory"):
        tp.randperm(4, device="cpu")
    assert tp.eye(3).shape == (3, 3)                          # without a device it is torch's
    assert tp.float32 is torch.float32 and tp.no_grad is torch.no_grad and tp.autograd is torch.autograd and tp.Tensor is torch.Tensor
    with pytest.raises(AttributeError):
        tp.no_such_function


def _module():
    m = types.ModuleType("redzone_victim")
    m.torch = torch
    exec("def make(n):\n    return torch.empty(n, dtype=torch.float32, device='cpu')\n", m.__dict__)
    return m


def test_guard_swaps_torch_counts_pointers_and_restores():
    m = _module()
    cache = types.SimpleNamespace(ws={"old": 1})
    with rz.guard(m, nbytes=4 * MiB, device="cpu", caches=[(cache, "ws")]) as g:
        assert isinstance(m.torch, rz.TorchProxy) and cache.ws == {}
        cache.ws["new"] = 2
        x = m.make(299)
        assert g.arena.contains(x.data_ptr())
        torch.zeros(3).data_ptr()
    assert m.torch is torch and cache.ws == {"old": 1} and "data_ptr" not in torch.Tensor.__dict__
    assert (g.inside, g.outside) == (1, 1)
    x[:] = 3.0                                                # still valid: the view keeps the storage
    assert bool((x == 3).all())


def test_guard_fails_on_an_overrun_and_when_nothing_was_guarded():
    m = _module()
    with pytest.raises(AssertionError, match=r"red zone: bytes changed outside a buffer.*\(299,\) torch.float32: 4 bytes from offset 0"):
        with rz.guard(m, nbytes=4 * MiB, device="cpu", caches=[]) as g:
            x = m.make(299)
            x.data_ptr()
            torch.as_strided(x, (300,), (1,))[299] = 0.0      # one float past the end
    assert m.torch is torch
    with pytest.raises(AssertionError, match="the guard was not active"):
        with rz.guard(m, nbytes=4 * MiB, device="cpu", caches=[]):
            torch.zeros(3).data_ptr()
    with pytest.raises(ZeroDivisionError):                    # an error of the body is the body's, and everything is restored
        with rz.guard(m, nbytes=4 * MiB, device="cpu", caches=[]):
            1 / 0
    assert m.torch is torch and "data_ptr" not in torch.Tensor.__dict__


def test_every_guarded_case_is_an_existing_parametrisation():
    """tests/test_redzone_gpu.py adds no shapes of its own: each case names an existing test and, for every parametrize mark of it, one of
    the mark's own value sets; what is left over in the signature is a fixture."""
    import importlib
    import inspect
    import test_redzone_gpu as rg
    ids = [rg.case_id(c) for c in rg.CASES]
    assert len(set(ids)) == len(ids)
    for module, name, kw in rg.CASES:
        fn = getattr(importlib.import_module(module), name)
        covered = set()
        for mark in getattr(fn, "pytestmark", []):
            if mark.name != "parametrize":
                continue
            names = [n.strip() for n in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
            sets = [tuple(getattr(v, "values", v)) if len(names) > 1 else (v,) for v in mark.args[1]]
            assert tuple(kw[n] for n in names) in sets, (module, name, names, kw)
            covered.update(names)
        assert covered == set(kw), (module, name, kw)
        assert set(inspect.signature(fn).parameters) - covered <= {"oracle_c", "monkeypatch"}, (module, name)
    for mod in ("test_raster_views_gpu", "test_render_view_vs_views_gpu", "test_absgrad_gpu"):
        assert "test_raster_gpu" in [m.__name__ for m in rg.helper_modules_of(importlib.import_module(mod))]      # helpers of other modules are guarded too


def test_proxy_factories_give_what_torch_gives():
    """shape, type, strides and (where defined) values of every overridden factory, in the argument forms the guarded modules use"""
    a, tp = _arena()
    x = torch.arange(24, dtype=torch.float16).reshape(2, 3, 4)
    xi = torch.arange(6, dtype=torch.int32).reshape(3, 2)
    calls = [("empty", (5,), {}), ("empty", (2, 3), {}), ("empty", ((2, 3),), {}), ("empty", (torch.Size([4, 1]),), {}), ("empty", (0,), {}),
             ("empty", (3,), dict(dtype=torch.int64)), ("zeros", (4,), {}), ("zeros", (2, 2), dict(dtype=torch.uint8)), ("zeros", ([3, 1],), {}),
             ("ones", (3,), {}), ("ones", (2, 1), dict(dtype=torch.int32)), ("full", ((3,), -1), dict(dtype=torch.int32)), ("full", ((2, 2), 0.5), {}),
             ("full", ((4,), float("nan")), {}), ("full", ((2,), 7), {}), ("empty_like", (x,), {}), ("empty_like", (x.permute(2, 0, 1),), {}),
             ("empty_like", (x,), dict(dtype=torch.float32)), ("zeros_like", (xi,), {}), ("zeros_like", (x.transpose(0, 1),), {}),
             ("ones_like", (xi.t(),), {}), ("full_like", (x, 2.0), {}), ("tensor", ([1, 2, 3],), {}), ("tensor", (2.5,), dict(dtype=torch.float16)),
             ("tensor", (x.numpy(),), {}), ("arange", (7,), {}), ("arange", (2, 9, 3), dict(dtype=torch.int32)), ("linspace", (0.0, 1.0, 5), {}),
             ("empty_strided", ((2, 3), (1, 2)), {}), ("empty_strided", ((2, 3), (4, 1)), dict(dtype=torch.int16))]
    for name, args, kw in calls:
        want = getattr(torch, name)(*args, **kw)
        got = getattr(tp, name)(*args, device="cpu", **kw)
        assert (got.shape, got.dtype, got.stride()) == (want.shape, want.dtype, want.stride()), (name, args, kw)
        assert a.contains(got.data_ptr()) or got.numel() == 0 and a.bufs[-1][0] == a.bufs[-1][1]
        assert not got._is_view()
        if not name.startswith("empty"):
            assert torch.equal(got.nan_to_num(), want.nan_to_num()), (name, args, kw)
    assert a.check() == []

"""Red zones around every buffer a guarded test hands to the library.

The library's contract (include/gaussctrl_hip.h) is that the caller owns every buffer, workspaces included, and that the *_workspace_bytes
queries say how large a workspace must be.  torch's caching allocator hides a breach of it: it rounds every request up to 512 bytes,
carves small ones out of 2 MiB blocks and recycles memory, so a kernel that stores a few elements past an output, reads past an input or
needs more workspace than its query returns still computes the right values.  Here every buffer is carved out of ONE ordinary allocation
with a poisoned zone behind it, so an overrun lands in memory the test owns (nothing faults) and is seen:

  Arena(nbytes, device)  one uint8 tensor and a bump allocator over it: a red zone first, and one of >= 16 KiB after every buffer (>= 1 MiB
                         after the last).  A buffer starts at an absolute address that is a multiple of 256 (the padding in front of it
                         belongs to the zone before) and ends exactly: its zone begins at the first byte after its last element.  Nothing is
                         ever freed; an exhausted arena raises.
  fill                   float buffers (fp32 / f16 / bf16, and the uint8 that holds e4m3 or raw workspace bytes) and their zones are 0xFF bytes,
                         a NaN in each of those types: whatever is computed from an over-read float fails the wrapped test's own comparison.
                         Integer buffers and their zones are 0x00: an index read from outside its array is still a valid index, so no test
                         turns an over-read into a wild access.  `empty*` buffers are left poisoned; `zeros*` / `full*` are carved, then set.
  Arena.check()          synchronises, compares every zone with its fill, returns the offenders.
  TorchProxy             stands in for the module global `torch` of the guarded modules (each does `import torch` and none uses Tensor.new_*):
                         the factory functions carve from the arena when asked for the arena's device; every other torch function refuses a
                         device= of that kind, so a new allocation site cannot slip past.
  guard(*modules)        the context manager the GPU cases run in (tests/test_redzone_gpu.py).

This module is a plain helper like _margins.py (tests/test_redzone_cpu.py checks it on CPU tensors)."""
import contextlib
import os
import sys
import types

import torch

from _margins import within

ZONE = 16 << 10
LAST_ZONE = 1 << 20
ALIGN = 256
_HERE = os.path.abspath(__file__)
_FLOAT_FILL = (torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.uint8) + tuple(
    getattr(torch, n) for n in ("float8_e4m3fn", "float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz") if hasattr(torch, n))


class ArenaExhausted(RuntimeError):
    pass


def fill_byte(dtype):
    return 0xFF if dtype in _FLOAT_FILL else 0x00


def _site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    return "?" if f is None else f"{os.path.relpath(f.f_code.co_filename, os.path.dirname(os.path.dirname(_HERE)))}:{f.f_lineno}"


class Arena:
    def __init__(self, nbytes, device):
        self.device = torch.device(device)
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.base = self.buf.data_ptr()
        self.nbytes = int(nbytes)
        self.end = 0                    # first byte after the last carved buffer
        self.bufs = []                  # (start, end, fill, site, shape, dtype)
        self.lead_fill = 0xFF
        if self.nbytes < ZONE + ALIGN + LAST_ZONE:
            raise ArenaExhausted(f"an arena needs at least {ZONE + ALIGN + LAST_ZONE} bytes for its first and last zones, got {self.nbytes}")
        self.buf[:ZONE + ALIGN].fill_(self.lead_fill)

    def contains(self, address):
        return self.base <= address < self.base + self.nbytes

    def carve(self, shape, dtype, stride=None):
        """a poisoned buffer of this shape and type (contiguous, or with the strides given) with its zone behind it"""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        if stride is not None and n:                          # elements from the first to the last one addressed
            n = 1 + sum((k - 1) * int(st) for k, st in zip(shape, stride))
        n *= dtype.itemsize
        start = -(-(self.base + self.end + ZONE) // ALIGN) * ALIGN - self.base
        end = start + n
        if end + LAST_ZONE > self.nbytes:
            raise ArenaExhausted(f"red-zone arena of {self.nbytes} bytes exhausted by {shape} {dtype} at {_site()} "
                                 f"({len(self.bufs)} buffers, {self.end} bytes carved): give the case a larger arena")
        fill = fill_byte(dtype)
        if not self.bufs and fill != self.lead_fill:          # the first zone has no buffer in front of it: it takes the fill of the one behind
            self.lead_fill = fill
            self.buf[:start].fill_(fill)
        self.buf[start:end + LAST_ZONE].fill_(fill)
        self.bufs.append((start, end, fill, _site(), shape, dtype))
        self.end = end
        # a tensor of its own on the arena's storage, not a view of self.buf: views would share one version counter (every later fill
        # of a zone would invalidate what autograd saved) and custom Functions may not return views of a common base
        assert start % dtype.itemsize == 0
        t = torch.empty(0, dtype=dtype, device=self.device)
        if stride is None:
            return t.set_(self.buf.untyped_storage(), start // dtype.itemsize, shape)
        return t.set_(self.buf.untyped_storage(), start // dtype.itemsize, shape, tuple(int(st) for st in stride))

    def _zones(self):
        """(zone start, zone end, fill, index of the buffer it follows or -1 for the first zone)"""
        if not self.bufs:
            return [(0, ZONE + ALIGN, self.lead_fill, -1)]
        z = [(0, self.bufs[0][0], self.lead_fill, -1)]
        for i, b in enumerate(self.bufs):
            z.append((b[1], self.bufs[i + 1][0] if i + 1 < len(self.bufs) else b[1] + LAST_ZONE, b[2], i))
        return z

    def check(self):
        """-> [(allocation site file:line, shape, dtype, offset of the first changed byte from the end of the buffer, changed bytes)];
        a change in the very first zone is reported against the first buffer with a negative offset (from its START)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        zones = self._zones()
        total = torch.zeros((), dtype=torch.int64, device=self.device)
        for s, e, fill, _ in zones:
            total += (self.buf[s:e] != fill).sum()
        if int(total) == 0:
            return []
        out = []
        for s, e, fill, i in zones:
            bad = (self.buf[s:e] != fill).nonzero().flatten()
            if bad.numel():
                first = int(bad[0])
                if i < 0:
                    b = self.bufs[0] if self.bufs else (e, e, fill, "(first zone)", (), torch.uint8)
                    out.append((b[3], b[4], b[5], first - e, int(bad.numel())))
                else:
                    b = self.bufs[i]
                    out.append((b[3], b[4], b[5], first, int(bad.numel())))
        return out


def _size(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(args[0])
    return tuple(args)


_TAKEN = ("dtype", "device", "requires_grad", "pin_memory", "memory_format", "layout")


class TorchProxy(types.ModuleType):
    """`torch` for a guarded module: everything is torch's own, except that tensors asked for on the arena's device come out of the arena."""

    def __init__(self, arena):
        super().__init__("torch")
        self.__dict__["_arena"] = arena
        self.__dict__["_kind"] = arena.device.type

    # -- which calls are the arena's
    def _mine(self, device):
        return device is not None and torch.device(device).type == self._kind

    def _finish(self, t, kw):
        return t.requires_grad_(True) if kw.get("requires_grad") else t

    def __getattr__(self, name):
        real = getattr(torch, name)
        if not isinstance(real, (types.BuiltinFunctionType, types.FunctionType)):
            return real

        def refuse_device(*a, **kw):
            if self._mine(kw.get("device")):
                raise RuntimeError(f"torch.{name}(..., device={kw['device']!r}) is not a factory the red-zone proxy carves (tests/_redzone.py): "
                                   "add it there, so that this buffer gets a red zone too")
            return real(*a, **kw)
        return refuse_device

    # -- uninitialised / constant buffers: carved, left poisoned or set
    def _carved(self, args, kw, value, like=None, infer=False):
        dtype = kw.get("dtype") or (like.dtype if like is not None else None)
        if dtype is None:                                     # torch.full takes the type of its value, every other factory the default type
            dtype = torch.get_default_dtype() if not infer or isinstance(value, float) else torch.bool if isinstance(value, bool) else torch.int64
        extra = set(kw) - set(_TAKEN)
        if extra:
            raise RuntimeError(f"red-zone proxy: unsupported factory arguments {sorted(extra)}")
        if like is None:
            if kw.get("memory_format") not in (None, torch.contiguous_format):
                raise RuntimeError("red-zone proxy: memory_format of a factory that is not *_like is not supported")
            t = self._arena.carve(_size(args), dtype)
        else:
            m = torch.empty_like(like, dtype=dtype, device="meta", **({"memory_format": kw["memory_format"]} if "memory_format" in kw else {}))
            t = self._arena.carve(m.shape, dtype, None if m.is_contiguous() else m.stride())
        if value is not None:
            t.fill_(value)
        return self._finish(t, kw)

    def empty(self, *args, **kw):
        return self._carved(args, kw, None) if self._mine(kw.get("device")) else torch.empty(*args, **kw)

    def zeros(self, *args, **kw):
        return self._carved(args, kw, 0) if self._mine(kw.get("device")) else torch.zeros(*args, **kw)

    def ones(self, *args, **kw):
        return self._carved(args, kw, 1) if self._mine(kw.get("device")) else torch.ones(*args, **kw)

    def full(self, size, fill_value, **kw):
        if not self._mine(kw.get("device")):
            return torch.full(size, fill_value, **kw)
        if torch.is_tensor(fill_value):
            kw.setdefault("dtype", fill_value.dtype)
        return self._carved((tuple(size),), kw, fill_value, infer=True)

    def empty_like(self, x, **kw):
        return self._carved((), kw, None, like=x) if self._mine(kw.get("device", x.device)) else torch.empty_like(x, **kw)

    def zeros_like(self, x, **kw):
        return self._carved((), kw, 0, like=x) if self._mine(kw.get("device", x.device)) else torch.zeros_like(x, **kw)

    def ones_like(self, x, **kw):
        return self._carved((), kw, 1, like=x) if self._mine(kw.get("device", x.device)) else torch.ones_like(x, **kw)

    def full_like(self, x, fill_value, **kw):
        return self._carved((), kw, fill_value, like=x) if self._mine(kw.get("device", x.device)) else torch.full_like(x, fill_value, **kw)

    def empty_strided(self, size, stride, **kw):
        if not self._mine(kw.get("device")):
            return torch.empty_strided(size, stride, **kw)
        extra = set(kw) - set(_TAKEN)
        if extra:
            raise RuntimeError(f"red-zone proxy: unsupported factory arguments {sorted(extra)}")
        return self._finish(self._arena.carve(size, kw.get("dtype") or torch.get_default_dtype(), stride), kw)

    # -- buffers with contents: torch makes the values (same bits as without the guard), the arena holds them
    def _copied(self, real, args, kw):
        if not self._mine(kw.get("device")):
            return real(*args, **kw)
        rg = kw.pop("requires_grad", False)
        src = real(*args, **kw)
        t = self._arena.carve(src.shape, src.dtype)
        t.copy_(src)
        return t.requires_grad_(True) if rg else t

    def tensor(self, *args, **kw):
        return self._copied(torch.tensor, args, kw)

    def rand(self, *args, **kw):
        return self._copied(torch.rand, args, kw)

    def randn(self, *args, **kw):
        return self._copied(torch.randn, args, kw)

    def randint(self, *args, **kw):
        return self._copied(torch.randint, args, kw)

    def arange(self, *args, **kw):
        return self._copied(torch.arange, args, kw)

    def linspace(self, *args, **kw):
        return self._copied(torch.linspace, args, kw)


_active = []          # the proxy of the guard that is running, if any
reached = set()       # entry points of the library that were looked up while a device guard was running (all guards of the process)


class _Calls:
    """the loaded library, remembering which entry points are asked for"""

    def __init__(self, real):
        self.__dict__["_real"] = real

    def __getattr__(self, name):
        reached.add(name)
        return getattr(self._real, name)


def on_device(t, device):
    """`t.to(device).contiguous()` for the inputs of a test, always a fresh copy with the same bits: under a guard it is carved from the
    arena, so an over-read of the input is seen (t.to(device) is torch's own allocation and would bypass the guard)"""
    out = (_active[-1] if _active else torch).empty(tuple(t.shape), dtype=t.dtype, device=device)
    out.copy_(t)
    return out


def _cuda_module_caches():
    """the scratch caches of the ops layer, (owner, name): emptied for the guarded body so that they are allocated again inside the arena"""
    from gaussctrl_amd.sd import ops as sd_ops
    return [(sd_ops, n) for n in ("_gn_ws", "_zero_page", "_disp_ws", "_abl_cache")]


class Guard:
    def __init__(self, arena):
        self.arena, self.inside, self.outside = arena, 0, 0

    def count(self, address):
        if address:
            if self.arena.contains(address):
                self.inside += 1
            else:
                self.outside += 1


@contextlib.contextmanager
def guard(*modules, nbytes=2 << 30, device="cuda:0", caches=None):
    """Run the body with `torch` of the given modules (the product modules that allocate, and the test modules whose body runs) replaced by
    a proxy over a fresh arena; afterwards every zone must be as it was filled.  The entry points of the library that the body looks up are
    collected in `reached`.

    Device pointers are counted where they leave for the library, at Tensor.data_ptr: _lib.call and _lib.ptr call it, and so does the ops
    layer where it fills the descriptors of the GEMM, attention and transformer head / tail entry points directly (wrapping ptr and _p
    alone would see no pointer of those).  The share outside the arena (inputs a test built with .to(device), results of torch
    arithmetic, gradients autograd allocated) is logged through within(); no pointer inside at all means the guard was not active, and fails."""
    arena = Arena(nbytes, device)
    proxy = TorchProxy(arena)
    g = Guard(arena)
    saved = [(m, m.__dict__["torch"]) for m in modules]
    caches = _cuda_module_caches() if caches is None else caches
    held = [(o, n, dict(getattr(o, n))) for o, n in caches]
    real_data_ptr = torch.Tensor.data_ptr
    own = "data_ptr" in torch.Tensor.__dict__

    def data_ptr(t):
        a = real_data_ptr(t)
        if t.device.type == arena.device.type:
            g.count(a)
        return a
    from gaussctrl_amd import _lib as L
    real_lib = L.lib() if arena.device.type == "cuda" else None
    try:
        if real_lib is not None:
            L._lib = _Calls(real_lib)
        for o, n, _ in held:
            getattr(o, n).clear()
        for m, _ in saved:
            setattr(m, "torch", proxy)
        torch.Tensor.data_ptr = data_ptr
        _active.append(proxy)
        yield g
    finally:
        if real_lib is not None:
            L._lib = real_lib
        if _active and _active[-1] is proxy:
            _active.pop()
        if own:
            torch.Tensor.data_ptr = real_data_ptr
        else:
            del torch.Tensor.data_ptr
        for m, t in saved:
            setattr(m, "torch", t)
        for o, n, was in held:                   # (arena-backed entries go: they would keep every arena alive, and count as outside later)
            d = getattr(o, n); d.clear(); d.update(was)
    bad = arena.check()
    n = sum(b[4] for b in bad)
    msg = "; ".join(f"{site} {shape} {dtype}: {cnt} bytes from offset {off}" for site, shape, dtype, off, cnt in bad[:8])
    if bad:
        print("red zone:", msg)
    assert g.inside > 0, f"no device pointer inside the arena ({g.outside} outside): the guard was not active"
    within("red zone: share of device pointers outside the arena", g.outside / (g.inside + g.outside), 1.0)
    try:
        within("red zone: bytes changed outside a buffer", n, 0)
    except AssertionError as e:
        raise AssertionError(f"{e} -- {msg}") from None

"""CPU: the typed binding of the C ABI (gaussctrl_amd/_lib.py).  The signature table against the prototypes of include/*.h (names, order,
every parameter's letter, the return kind: a wrong letter is a wrong launch), the loader's argtypes / restype against the table, what
call() refuses before anything is launched, its error text, its return values without a GPU, what a proxy at `_lib._lib` sees, and the
arity of every call() site of the host modules."""
import ctypes
import os

import pytest

import _abi_header as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_MODULES = ["gsplat_ops.py", "sd/ops.py", "train_ops.py", "refine.py", "mcmc.py", "bilagrid.py", "edit_region.py", "dist.py"]
INT_VALUED = {"gc_abi_version", "gc_dn_gemm_row_stat_slots"}       # `int` that is a value, not a status code (no GC_E* meaning)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")):
        ge.build()
    from gaussctrl_amd import _lib
    return _lib


def test_table_is_the_headers():
    """no library needed: header by header, the table's names in the header's order, one letter per parameter (int i, int64_t q, float f,
    size_t z, any pointer p, a final `void *stream` s) and the return kind (C `int` is e, a checked status, or i for the two value queries)"""
    from gaussctrl_amd import _lib
    assert sorted(_lib.ABI) == A.headers()
    total = 0
    for header in A.headers():
        protos = A.prototypes(header)
        assert list(_lib.ABI[header]) == [p.name for p in protos], header
        assert sorted(p.name for p in protos) == sorted(set(A.names(header, "gc") + A.names(header, "gcx"))), header   # no prototype the parser missed
        for p in protos:
            ret, letters = A.signature(p)
            kind, got = _lib.ABI[header][p.name].split(":")
            assert got == letters, (p.name, got, letters)
            assert {"e": "i"}.get(kind, kind) == ret and (kind == "i") == (p.name in INT_VALUED), (p.name, kind, ret)
            assert "s" not in letters[:-1]
        total += len(protos)
    assert total == len(_lib.SIGNATURES) == 104
    assert len(_lib.SYMBOLS) == 98 and len(_lib.EXT_SYMBOLS) == 4 and len(_lib.POSE_SYMBOLS) == 2
    assert sorted(_lib.SYMBOLS + _lib.EXT_SYMBOLS + _lib.POSE_SYMBOLS) == sorted(_lib.SIGNATURES)
    assert _lib.EXT_SETS["gaussctrl_pose.h"] is _lib.POSE_SYMBOLS and _lib.EXT_SETS["gaussctrl_bilagrid.h"] is _lib.EXT_SYMBOLS


def test_loader_types_are_the_table(L):
    ct = {"i": ctypes.c_int, "q": ctypes.c_int64, "f": ctypes.c_float, "z": ctypes.c_size_t, "p": ctypes.c_void_p, "s": ctypes.c_void_p}
    rt = {"e": ctypes.c_int, "i": ctypes.c_int, "z": ctypes.c_size_t, "c": ctypes.c_char_p, "v": None}
    lib = L.lib()
    for name, sig in L.SIGNATURES.items():
        kind, letters = sig.split(":")
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [ct[c] for c in letters], name
        assert fn.restype is rt[kind], name


def test_every_host_call_site_passes_the_table_arity(L):
    """call() checks the count at run time; this holds every site of the product modules to it without running one (argument tuples handed
    on with * are counted by their elements), and finds no untyped spelling left"""
    seen = set()
    for mod in HOST_MODULES:
        calls = A.host_calls("gaussctrl_amd/" + mod)
        assert calls, mod
        for names, n, line in calls:
            for name in names:
                assert L._PLANS[name][1] == n, (mod, line, name, n)
                seen.add(name)
        text = open(os.path.join(ROOT, "gaussctrl_amd", mod)).read()
        for old in ("L.ptr(", "L.i32(", "L.i64(", "L.f32(", "L.check(", "L.lib()", "stream_ptr("):
            assert old not in text, (mod, old)
    assert len(seen) >= 85


def _trace_args(L, C=0):
    """gc_trace_mask_views as tests/test_trace_abi_cpu.py calls it (host memory, refused on its first check with C = 0), without the stream"""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return [C, 4, 8, 1, 16, 16, 1, 1, p, p, p, p, p, p, p, p], buf


def test_call_refuses_wrong_counts_and_widths_before_the_foreign_call(L, monkeypatch):
    args, _keep = _trace_args(L)
    reached = []

    class Spy:                                              # the typed functions behind a proxy that notes every foreign call that returns
        def __getattr__(self, name):
            fn = getattr(real, name)

            def f(*a):
                r = fn(*a)
                reached.append(name)
                return r
            return f
    real = L.lib()
    monkeypatch.setattr(L, "_lib", Spy())
    monkeypatch.setattr(L, "stream_handle", lambda: 0)      # (no GPU here; C = 0 throughout: were a conversion to pass, the library refuses)
    with pytest.raises(TypeError):
        L.call("gc_trace_mask_views", *args[:-1])
    with pytest.raises(TypeError):
        L.call("gc_trace_mask_views", *args, None)
    with pytest.raises(ctypes.ArgumentError):
        L.call("gc_trace_mask_views", 0.0, *args[1:])                  # float where int is declared
    with pytest.raises(ctypes.ArgumentError):
        L.call("gc_trace_mask_views", ctypes.c_int64(0), *args[1:])    # an int64 wrapper where int is declared
    with pytest.raises(ctypes.ArgumentError):
        L.call("gc_trace_mask_views", args[0], ctypes.c_int(4), *args[2:])   # ... and an int wrapper where int64_t is
    with pytest.raises(ctypes.ArgumentError):
        L.call("gc_raster_scan_workspace_bytes", 2.5)
    with pytest.raises(KeyError):
        L.call("gc_no_such_entry_point")
    assert reached == []
    # the direct form keeps working through the typed functions and does not raise on a status
    assert real.gc_trace_mask_views(*[L.i32(a) if k in (0, 3, 4, 5, 6, 7) else L.i64(a) if k in (1, 2) else a for k, a in enumerate(args)],
                                    ctypes.c_void_p(0)) == -1


def test_error_text_and_return_kinds_without_a_gpu(L):
    from gaussctrl_amd.sd import ops
    d = ops.GemmDesc()
    d.dtype = 1; d.mode = 0; d.M, d.N, d.K = 6144, 640, 640
    d.lda = 640; d.out = 1; d.ldc = 640; d.zeros = 1; d.rows_per_batch = 1024
    sel = ops.GemmSelection()
    d.kernel_variant = 0x2000 | ops.GC_GEMM_VAR_K4_ONLY                # an undefined bit: the inputs of test_undefined_variant_bits_are_refused
    with pytest.raises(L.GaussCtrlHipError) as e:
        L.call("gc_dn_gemm_selection", ctypes.byref(d), ctypes.byref(sel))
    text = str(e.value)
    assert text.startswith("gc_dn_gemm_selection failed (code -1): ") and "kernel_variant" in text and "0x2000" in text
    d.kernel_variant = ops.GC_GEMM_VAR_K4_ONLY
    assert L.call("gc_dn_gemm_selection", ctypes.byref(d), ctypes.byref(sel)) == 0 and sel.kernel == 1
    # every other return kind is handed back: size_t, plain int, const char *, void -- none of them looks up a stream
    wsb = L.call("gc_dn_gemm_workspace_bytes", ctypes.byref(d))
    assert type(wsb) is int and wsb == L.lib().gc_dn_gemm_workspace_bytes(ctypes.byref(d))
    assert L.call("gc_dn_gemm_row_stat_slots", ctypes.byref(d)) == L.lib().gc_dn_gemm_row_stat_slots(ctypes.byref(d)) > 0
    assert L.call("gc_abi_version") >= 1
    assert isinstance(L.call("gc_last_error_string"), bytes)
    q = [ctypes.c_int64(0) for _ in range(4)]
    assert L.call("gc_dn_transformer_tail_layout", *[ctypes.byref(v) for v in q]) is None and all(v.value > 0 for v in q)
    assert L.call("gc_raster_scan_workspace_bytes", 5000) == L.lib().gc_raster_scan_workspace_bytes(L.i64(5000)) >= 12
    # an object with data_ptr in a pointer position goes through it (where the red-zone guard counts device pointers); None is NULL
    class T:
        def data_ptr(self):
            return ctypes.addressof(d)
    assert L.call("gc_dn_gemm_workspace_bytes", T()) == wsb


def test_a_proxy_at_the_handle_sees_every_call(L, monkeypatch):
    """bench.py's LibTimer and tests/_redzone.py's _Calls stand at `_lib._lib`; tests/test_abi.py puts plain Python methods behind
    `_lib.lib`: call() looks the function up by name on the handle every time, hands it exactly the header's arguments, and reads the
    stream rule from the table, never from the function it is handed"""
    seen = []

    class Proxy:
        def __getattr__(self, name):
            def f(*a):
                seen.append((name, a))
                return b"proxy text" if name == "gc_last_error_string" else 7 if name == "gc_refine_plan_workspace_bytes" else 0
            return f
    monkeypatch.setattr(L, "_lib", Proxy())
    monkeypatch.setattr(L, "stream_handle", lambda: 0x5EED)
    args, _keep = _trace_args(L, C=1)
    assert L.call("gc_trace_mask_views", *args) == 0
    assert L.call("gc_refine_plan_workspace_bytes", 12) == 7
    L.call("gc_trace_mask_views", *args)
    assert [n for n, _ in seen] == ["gc_trace_mask_views", "gc_refine_plan_workspace_bytes", "gc_trace_mask_views"]
    assert len(seen[0][1]) == len(A.prototypes("gaussctrl_trace.h")[0].params) == 17 and seen[0][1][-1] == 0x5EED
    assert seen[1][1] == (12,)
    monkeypatch.setattr(L, "_lib", type("Failing", (Proxy,), {"__getattr__": lambda self, name: (
        lambda *a: b"proxy text" if name == "gc_last_error_string" else -3)})())
    with pytest.raises(L.GaussCtrlHipError, match=r"gc_trace_mask_views failed \(code -3\): proxy text"):
        L.call("gc_trace_mask_views", *args)

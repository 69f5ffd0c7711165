"""Host cost of one library call through the typed binding, against the spelling it replaced, on the same built library, no GPU needed.

  old   the loader of before: a handle with only restype set, every argument wrapped by hand at the call site
        (L.check(lib.gc_x(L.i64(N), L.ptr(t), ..., stream), "gc_x"))
  new   _lib.call("gc_x", N, t, ...): argtypes from the signature table, tensors converted and the stream appended inside

  A  gc_dn_gemm_selection: a two-argument host query that succeeds
  B  gc_trace_mask_views with C = 0: 17 arguments, 8 of them tensors, refused on its first check (as tests/test_trace_abi_cpu.py calls
     it), so both spellings end in the same GaussCtrlHipError, which is caught; the stream lookup is stubbed to NULL for both

The two spellings run interleaved, REPEATS times LOOPS calls each; per repeat the mean microseconds per call.  The bar for the typed path:
its mean no higher than the old spelling's beyond the old spelling's own spread over the repeats.

    python scripts/bind_overhead.py [OUT.txt]
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from gaussctrl_amd import _lib as L
from gaussctrl_amd.sd import ops

LOOPS, REPEATS = 20000, 7


def old_handle():
    l = C.CDLL(L.LIB_PATH)
    l.gc_last_error_string.restype = C.c_char_p
    for s in L.SIGNATURES:
        if s.endswith("_bytes"):
            getattr(l, s).restype = C.c_size_t
        elif s != "gc_last_error_string":
            getattr(l, s).restype = C.c_int
    return l


def main(out=None):
    old = old_handle()
    L.lib()
    L.stream_handle = lambda: 0                       # no GPU here: NULL stream for both spellings
    d = ops.GemmDesc()
    d.dtype = 1; d.mode = 0; d.M, d.N, d.K = 6144, 640, 640
    d.lda = 640; d.out = 1; d.ldc = 640; d.zeros = 1; d.rows_per_batch = 1024
    sel = ops.GemmSelection()
    t = [torch.zeros(64) for _ in range(8)]
    Cv, N, M, H, W, tx, ty = 0, 4, 8, 16, 16, 1, 1

    def check_old(rc, what):
        if rc != 0:
            raise L.GaussCtrlHipError(f"{what} failed (code {rc}): {old.gc_last_error_string().decode('utf-8', 'replace')}")

    def a_old():
        check_old(old.gc_dn_gemm_selection(C.byref(d), C.byref(sel)), "gc_dn_gemm_selection")

    def a_new():
        L.call("gc_dn_gemm_selection", C.byref(d), C.byref(sel))

    def b_old():
        try:
            check_old(old.gc_trace_mask_views(L.i32(Cv), L.i64(N), L.i64(M), L.i32(1), L.i32(H), L.i32(W), L.i32(tx), L.i32(ty), L.ptr(t[0]), L.ptr(t[1]),
                                              L.ptr(t[2]), L.ptr(t[3]), L.ptr(t[4]), L.ptr(t[5]), L.ptr(t[6]), L.ptr(t[7]), C.c_void_p(L.stream_handle())),
                      "gc_trace_mask_views")
        except L.GaussCtrlHipError:
            pass

    def b_new():
        try:
            L.call("gc_trace_mask_views", Cv, N, M, 1, H, W, tx, ty, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7])
        except L.GaussCtrlHipError:
            pass

    def us(f):
        t0 = time.perf_counter()
        for _ in range(LOOPS):
            f()
        return 1e6 * (time.perf_counter() - t0) / LOOPS
    lines = [f"bind_overhead: {LOOPS} calls per repeat, {REPEATS} interleaved repeats, microseconds per call (python {sys.version.split()[0]})"]
    for case, fo, fn in (("A gc_dn_gemm_selection (2 arguments, succeeds)", a_old, a_new),
                         ("B gc_trace_mask_views, C = 0 (17 arguments, refused, error raised and caught)", b_old, b_new)):
        us(fo); us(fn)                                # warm
        o, n = [], []
        for _ in range(REPEATS):
            o.append(us(fo)); n.append(us(fn))
        mean = lambda v: sum(v) / len(v)
        lines.append(case)
        lines.append("  old   " + " ".join(f"{x:.2f}" for x in o) + f"   mean {mean(o):.2f}  spread {max(o) - min(o):.2f}")
        lines.append("  new   " + " ".join(f"{x:.2f}" for x in n) + f"   mean {mean(n):.2f}  spread {max(n) - min(n):.2f}")
        lines.append(f"  new - old = {mean(n) - mean(o):+.2f} us per call: " + ("within" if mean(n) <= mean(o) + (max(o) - min(o)) else "OUTSIDE") + " the old spelling's spread")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)

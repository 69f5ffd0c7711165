"""CPU: the C-ABI library loads and exports every symbol include/gaussctrl_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

from _abi_header import names as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")):
        ge.build()
    return os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")


def test_header_symbols_exported(built):
    lib = ctypes.CDLL(built)
    decl = _declared()
    assert len(decl) >= 15
    missing = [n for n in decl if not hasattr(lib, n)]
    assert not missing, missing


def test_loader_symbol_list_matches_header(built):
    from gaussctrl_amd import _lib
    assert sorted(_lib.SYMBOLS) == _declared()
    l = _lib.lib()
    assert l.gc_abi_version() >= 1
    assert l.gc_raster_scan_workspace_bytes(ctypes.c_int64(5000)) >= 3 * 4


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 100003, (1 << 20) + 1])
def test_binning_workspace_sizes_keep_their_layout(built, n):
    """The *_workspace_bytes functions of the two-level binning are ABI (callers allocate by them): per view two ping-pong item buffers (pairs: a key
    and a value array of 4 n + 4 bytes each; triples: 12 n + 16 bytes), two [256][workgroups of 4096] digit tables, the scan scratch (one word per
    2048 entries of max(table, n), + 1) and 256 bytes for the ticket, every part rounded up to 256 bytes -- whatever computes the layout inside."""
    from gaussctrl_amd import _lib
    l = _lib.lib()
    al = lambda x: (x + 255) & ~255
    m = max(n, 1)
    nb = max(1, -(-m // 4096))
    tail = 2 * al(4 * 256 * nb) + al(4 * (-(-max(256 * nb, m) // 2048) + 1)) + 256
    pair, tri = 4 * al(4 * m + 4) + tail, 2 * al(12 * m + 16) + tail
    i64, i32 = ctypes.c_int64, ctypes.c_int
    assert l.gc_raster_depth_order_workspace_bytes(i64(n)) == pair and l.gc_raster_bin_workspace_bytes(i64(n)) == pair
    for c in (0, 1, 8):
        assert l.gc_raster_depth_order_views_workspace_bytes(i64(n), i32(c)) == pair * max(c, 1)
        assert l.gc_raster_bin_views_workspace_bytes(i64(n), i32(c)) == pair * max(c, 1)
        assert l.gc_raster_order_boxes_views_workspace_bytes(i64(n), i32(c)) == tri * max(c, 1)


def test_documented_entry_point_count_is_current():
    """DESIGN.md / INTEGRATION.md state how many entry points the header declares: the number must be the header's (it went stale twice)"""
    n = len(_declared())
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        found = [int(m) for m in re.findall(r"(\d+) (?:`extern \"C\"` )?entry points", text)]
        assert found, doc
        assert all(f == n for f in found), (doc, found, n)


def test_product_path_refuses_cpu_tensors(built):
    import torch
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd._lib import GaussCtrlHipError
    with pytest.raises(GaussCtrlHipError):
        ops.spherical_harmonics(3, torch.zeros(4, 3), torch.zeros(4, 16, 3))


def test_no_oracle_import_in_product():
    """the product package must never import oracle/ (parity claims depend on it)."""
    pkg = os.path.join(ROOT, "gaussctrl_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith(".py"):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dp, fn)


def test_library_has_no_packed_fp32_arithmetic(built):
    """DESIGN.md 7.0 (round 4): v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 return wrong results in lanes 48..63 on the MI355X boxes of this
    pool whenever a wavefront of ANOTHER process issues MFMAs on the same SIMD (profiles/r04_packed_fp32_fault.txt; found through the
    two-ranks-on-one-GPU test).  The library is built with the SLP and loop vectorizers off, which is where every one of them came from;
    this holds the disassembly of the shipped code objects at zero."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("packed_fp32_audit", os.path.join(ROOT, "scripts", "packed_fp32_audit.py"))
    audit = importlib.util.module_from_spec(spec); spec.loader.exec_module(audit)
    found, functions = audit.audit(built)
    assert functions > 300, functions            # every translation unit's code object was found
    assert not found, found


def test_descriptor_structs_match_the_header(tmp_path):
    """the ctypes mirrors of gc_gemm_desc / gc_attn_desc (gaussctrl_amd/sd/ops.py) have the size and the last-field offset the C compiler
    gives the header's structs: a field added on one side only would shift every later argument silently."""
    import subprocess
    from gaussctrl_amd.sd import ops
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gaussctrl_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(gc_gemm_desc), offsetof(gc_gemm_desc, softmax_keys), sizeof(gc_attn_desc),'
                   ' offsetof(gc_attn_desc, workspace_bytes)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(ops.GemmDesc), ops.GemmDesc.softmax_keys.offset, ctypes.sizeof(ops.AttnDesc), ops.AttnDesc.workspace_bytes.offset]


def test_fp8_linear_copies_of_transformer_weights():
    """weights.add_fp8_linears (host side, CPU): e4m3 copies exist for the C % 128 == 0 blocks only, dequantise to within one e4m3 step of
    the prepared 2-byte weights (row scale = power of two, row maximum in the top binade), and keep the GEGLU row permutation."""
    import torch
    from gaussctrl_amd.sd.weights import add_fp8_linears
    g = torch.Generator().manual_seed(0)
    out = {}
    for name, C in (("a.transformer_blocks.0.", 640), ("b.transformer_blocks.0.", 320)):
        for lin, (n, k) in (("attn1.to_qkv", (3 * C, C)), ("attn2.to_q", (C, C)), ("ff.net.0.proj", (8 * C, C)), ("ff.net.2", (C, 4 * C))):
            out[name + lin + ".weight"] = (torch.randn(n, k, generator=g) * k ** -0.5 * torch.exp2(torch.randint(-6, 6, (n, 1), generator=g).float())).to(torch.bfloat16)
    add_fp8_linears(out, 5)
    assert out["_fp8_linears"] == 5
    assert not any(k.startswith("b.") and k.endswith(".w8") for k in out)
    for lin in ("attn1.to_qkv", "attn2.to_q", "ff.net.0.proj", "ff.net.2"):
        w = out["a.transformer_blocks.0." + lin + ".weight"].double()
        q, sc = out["a.transformer_blocks.0." + lin + ".w8"], out["a.transformer_blocks.0." + lin + ".w8_scale"]
        assert q.dtype == torch.uint8 and q.shape == w.shape and sc.shape == (w.shape[0],)
        deq = q.view(torch.float8_e4m3fn).double() * torch.exp2(sc.double() - 127)[:, None]
        amax = w.abs().amax(1, keepdim=True)
        assert bool(((deq - w).abs() <= 0.0626 * w.abs() + amax * 2.0 ** -9).all())          # half an e4m3 step (normal), subnormal floor
        stored_max = q.view(torch.float8_e4m3fn).float().abs().amax(1)
        assert bool((stored_max >= 224).all()) and bool((stored_max <= 448).all())


def test_fp8_gemm_planning_queries(built):
    """host-side planning of the fp8 GEMM (no GPU needed: gc_dn_gemm_workspace_bytes / gc_dn_gemm_chan_parts_layout are pure functions of
    the descriptor): the 16 x 16-map convolutions at the benchmark's batch are k-sliced and leave their GroupNorm partials through the
    reduce kernel (32-row slabs, 64-column blocks); full grids are not sliced and leave them through k_gemm8q's own epilogue (row-tile
    slabs); GEGLU / e4m3-output / statistics problems are never sliced; with plan_rows (batch-invariant mode) the slice count depends on the
    rows ONE frame contributes, not on the batch."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.ops import GemmDesc
    lib = ctypes.CDLL(built)
    lib.gc_dn_gemm_workspace_bytes.restype = ctypes.c_size_t

    def conv(B, hw, cin, cout, **kw):
        d = GemmDesc()
        d.dtype = 0; d.mode = 1; d.M, d.N, d.K = B * hw * hw, cout, 9 * cin
        d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.stride, d.pad_lo = B, hw, hw, cin, hw, hw, 1, 1
        d.rows_per_batch = hw * hw; d.fp8 = 1; d.a_scale = 127; d.out = 1; d.ldc = cout; d.lda = cin
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def splits(d):
        return lib.gc_dn_gemm_workspace_bytes(ctypes.byref(d)) // (4 * d.M * d.N)

    def layout(d, with_ws=True):
        if with_ws:
            d.workspace = 1; d.workspace_bytes = lib.gc_dn_gemm_workspace_bytes(ctypes.byref(d))
        d.gn_groups = 32
        rows, ns, ct = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
        assert lib.gc_dn_gemm_chan_parts_layout(ctypes.byref(d), ctypes.byref(rows), ctypes.byref(ns), ctypes.byref(ct)) == 0
        return rows.value, ns.value, ct.value

    assert splits(conv(6, 16, 1280, 1280)) == 2                 # 120 tiles of 90 k-steps -> 240 workgroups
    assert splits(conv(3, 16, 1280, 1280)) == 5                 # 60 tiles -> 300 workgroups of 18 k-steps
    assert splits(conv(6, 16, 2560, 1280)) == 2
    assert splits(conv(14, 16, 1280, 1280)) == 0                # 280 tiles: a full grid
    assert splits(conv(6, 32, 640, 640)) == 0 and splits(conv(6, 64, 384, 320)) == 0
    assert splits(conv(6, 16, 1280, 1280, geglu=1)) == 0 and splits(conv(6, 16, 1280, 1280, out_fp8=127)) == 0
    assert splits(conv(6, 16, 1280, 1280, out_group_stats=1)) == 0
    assert splits(conv(6, 16, 1280, 1280, kernel_variant=2 << ops.GC_GEMM_VAR_MT_SHIFT)) == 0          # a forced tile height (MT 2) does not slice
    assert layout(conv(6, 16, 1280, 1280)) == (32, 8, 64)       # reduce kernel: 32-row slabs, 64-column blocks
    assert layout(conv(6, 16, 1280, 1280), with_ws=False) == (128, 2, 128)   # no workspace -> unsliced, k_gemm8q's own partial epilogue
    assert layout(conv(14, 16, 1280, 1280)) == (192, 3, 128)    # MT 3 tiles of 192 rows straddle the 256-row batches
    assert layout(conv(6, 64, 384, 320)) == (128, 32, 160)      # N = 320 (Cin 320 padded to 384): 160-column tiles
    assert layout(conv(6, 8, 1280, 1280))[0] == 0               # 8 x 8 maps: fewer than 256 rows per batch -> no partials
    # batch-invariant planning: the same slices whatever shares the batch
    a, b = conv(6, 16, 1280, 1280, plan_rows=256), conv(14, 16, 1280, 1280, plan_rows=256)
    assert splits(a) == splits(b) == 10


def test_gemm_planning_matches_the_documented_design(built):
    """the 2-byte GEMM's host-side planning at the benchmark's shapes (CFG batch 6), as DESIGN.md 3.2 / 7.0 states it: 64 x 64 maps at C = 320 on
    192-row x 160-column tiles; 32 x 32 maps on 128 x 128 tiles; the long-K part-filled grids in k-slices whose reduce kernel leaves the GroupNorm
    partials in 32-row slabs; the 8 x 8 maps in 15 slices ("128 x 128 x 15 slices") without partials (fewer than 256 rows per batch); GEGLU
    never sliced.  Pure functions of the descriptor: no GPU needed."""
    from gaussctrl_amd.sd.ops import GemmDesc
    lib = ctypes.CDLL(built)
    lib.gc_dn_gemm_workspace_bytes.restype = ctypes.c_size_t

    def conv(B, hw, cin, cout):
        d = GemmDesc()
        d.dtype = 0; d.mode = 1; d.M, d.N, d.K = B * hw * hw, cout, 9 * cin
        d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.stride, d.pad_lo = B, hw, hw, cin, hw, hw, 1, 1
        d.rows_per_batch = hw * hw; d.out = 1; d.ldc = cout; d.lda = cin; d.zeros = 1
        return d

    def lin(M, N, K, rpb=0, geglu=0):
        d = GemmDesc()
        d.dtype = 0; d.mode = 0; d.M, d.N, d.K = M, N, K
        d.lda = K; d.out = 1; d.ldc = N; d.zeros = 1; d.rows_per_batch = rpb; d.geglu = geglu
        return d

    def plan(d):
        ws = lib.gc_dn_gemm_workspace_bytes(ctypes.byref(d))
        d.workspace = 1; d.workspace_bytes = ws; d.gn_groups = 32
        rows, ns, ct = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
        assert lib.gc_dn_gemm_chan_parts_layout(ctypes.byref(d), ctypes.byref(rows), ctypes.byref(ns), ctypes.byref(ct)) == 0
        return ws // (4 * d.M * d.N), (rows.value, ns.value, ct.value)

    assert plan(conv(6, 64, 320, 320)) == (0, (192, 23, 160))
    assert plan(conv(6, 32, 640, 640)) == (0, (128, 8, 128))
    assert plan(conv(6, 16, 1280, 1280)) == (4, (32, 8, 64))
    assert plan(conv(6, 16, 2560, 1280)) == (4, (32, 8, 64))
    assert plan(conv(6, 8, 1280, 1280)) == (15, (0, 0, 0))
    assert plan(lin(6144, 640, 640, 1024)) == (0, (128, 8, 128))              # proj_out of a 32 x 32 block
    assert plan(lin(1536, 1280, 5120, 256)) == (4, (32, 8, 64))               # FF down projection, 16 x 16 block
    assert plan(lin(384, 1280, 5120, 64))[0] == 10                            # ... 8 x 8 block
    assert plan(lin(6144, 5120, 640, geglu=1)) == (0, (0, 0, 0))


# (H, Cin, Cout, stride) of every 3 x 3 conv of one UNet + ControlNet forward at 64 x 64 latents (conv_in with Cin padded to 8), and
# (L, K, N, geglu) of its plain linears per level; the table holds, per CFG batch of a launch set (12: the short last set of a scene, 24: the
# default 4 chunks x 3 views, 40: 4 chunks of the plugin's chunk_size 5), (kernel, m-tiles, k-slices, ntw) as launched, the GroupNorm partials
# layout (rows per slab, slabs per batch, column tile; None: the stand-alone GroupNorm), and (kernel, m-tiles, k-slices, ntw) in the
# batch-invariant form (plan_rows = the rows of one frame).  Linears also carry the persistent workgroup count.
_LAUNCH_SET_CONVS = {
    (64, 320, 320, 1): {12: (("k8", 3, 1, 5), (192, 23, 160), ("k8_sliced", 2, 3, 5)), 24: (("k8", 4, 1, 5), (256, 16, 160), ("k8_sliced", 2, 3, 5)), 40: (("k8", 4, 1, 5), (256, 16, 160), ("k8_sliced", 2, 3, 5))},
    (64, 640, 320, 1): {12: (("k8", 3, 1, 5), (192, 23, 160), ("k8_sliced", 2, 4, 5)), 24: (("k8", 4, 1, 5), (256, 16, 160), ("k8_sliced", 2, 4, 5)), 40: (("k8", 4, 1, 5), (256, 16, 160), ("k8_sliced", 2, 4, 5))},
    (64, 960, 320, 1): {12: (("k8", 3, 1, 5), (192, 23, 160), ("k8_sliced", 2, 4, 5)), 24: (("k8", 4, 1, 5), (256, 16, 160), ("k8_sliced", 2, 4, 5)), 40: (("k8", 4, 1, 5), (256, 16, 160), ("k8_sliced", 2, 4, 5))},
    (64, 320, 320, 2): {12: (("k8", 2, 1, 5), (128, 8, 160), ("k8_sliced", 2, 3, 5)), 24: (("k8", 3, 1, 5), (192, 7, 160), ("k8_sliced", 2, 3, 5)), 40: (("k8", 3, 1, 5), (192, 7, 160), ("k8_sliced", 2, 3, 5))},
    (32, 320, 640, 1): {12: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 3, 4)), 24: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 3, 4)), 40: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 3, 4))},
    (32, 640, 640, 1): {12: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4)), 24: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4)), 40: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4))},
    (32, 1280, 640, 1): {12: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4)), 24: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4)), 40: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4))},
    (32, 1920, 640, 1): {12: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4)), 24: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4)), 40: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4))},
    (32, 960, 640, 1): {12: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4)), 24: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4)), 40: (("k8", 4, 1, 4), (256, 4, 128), ("k8_sliced", 2, 6, 4))},
    (32, 640, 640, 2): {12: (("k8_sliced", 3, 3, 4), (32, 8, 64), ("k8_sliced", 2, 7, 4)), 24: (("k8", 2, 1, 4), (128, 2, 128), ("k8_sliced", 2, 7, 4)), 40: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 7, 4))},
    (16, 640, 1280, 1): {12: (("k8", 2, 1, 4), (128, 2, 128), ("k8_sliced", 2, 7, 4)), 24: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 7, 4)), 40: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 7, 4))},
    (16, 1280, 1280, 1): {12: (("k8", 2, 1, 4), (128, 2, 128), ("k8_sliced", 2, 12, 4)), 24: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 12, 4)), 40: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 12, 4))},
    (16, 2560, 1280, 1): {12: (("k8", 2, 1, 4), (128, 2, 128), ("k8_sliced", 2, 12, 4)), 24: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 12, 4)), 40: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 12, 4))},
    (16, 1920, 1280, 1): {12: (("k8", 2, 1, 4), (128, 2, 128), ("k8_sliced", 2, 12, 4)), 24: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 12, 4)), 40: (("k8", 4, 1, 4), (256, 1, 128), ("k8_sliced", 2, 12, 4))},
    (16, 1280, 1280, 2): {12: (("k8_sliced", 2, 4, 4), None, ("k8_sliced", 2, 15, 4)), 24: (("k8_sliced", 4, 4, 4), None, ("k8_sliced", 2, 15, 4)), 40: (("k8", 2, 1, 4), None, ("k8_sliced", 2, 15, 4))},
    (8, 1280, 1280, 1): {12: (("k8_sliced", 2, 4, 4), None, ("k8_sliced", 2, 15, 4)), 24: (("k8_sliced", 4, 4, 4), None, ("k8_sliced", 2, 15, 4)), 40: (("k8", 2, 1, 4), None, ("k8_sliced", 2, 15, 4))},
    (8, 2560, 1280, 1): {12: (("k8_sliced", 2, 4, 4), None, ("k4", 0, 16, 4)), 24: (("k8_sliced", 4, 4, 4), None, ("k4", 0, 16, 4)), 40: (("k8", 2, 1, 4), None, ("k4", 0, 16, 4))},
    (64, 8, 320, 1): {12: (("k8", 3, 1, 5), (192, 23, 160), ("k4", 0, 1, 5)), 24: (("k8", 4, 1, 5), (256, 16, 160), ("k4", 0, 1, 5)), 40: (("k8", 4, 1, 5), (256, 16, 160), ("k4", 0, 1, 5))},
}
_LAUNCH_SET_LINEARS = {
    (4096, 320, 320, 0): {12: (("k8", 3, 1, 5), 0, (192, 23, 160), ("k8", 2, 1, 5)), 24: (("k8", 4, 1, 5), 0, (256, 16, 160), ("k8", 2, 1, 5)), 40: (("k8", 4, 1, 5), 0, (256, 16, 160), ("k8", 2, 1, 5))},
    (4096, 320, 2560, 1): {12: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4)), 24: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4)), 40: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4))},
    (4096, 1280, 320, 0): {12: (("k8", 3, 1, 5), 0, (192, 23, 160), ("k8", 2, 1, 5)), 24: (("k8", 4, 1, 5), 0, (256, 16, 160), ("k8", 2, 1, 5)), 40: (("k8", 4, 1, 5), 0, (256, 16, 160), ("k8", 2, 1, 5))},
    (1024, 640, 640, 0): {12: (("k8", 4, 1, 4), 0, (256, 4, 128), ("k8", 2, 1, 4)), 24: (("k8", 4, 1, 4), 0, (256, 4, 128), ("k8", 2, 1, 4)), 40: (("k8", 4, 1, 4), 0, (256, 4, 128), ("k8", 2, 1, 4))},
    (1024, 640, 5120, 1): {12: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4)), 24: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4)), 40: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4))},
    (1024, 2560, 640, 0): {12: (("k8", 4, 1, 4), 0, (256, 4, 128), ("k8_sliced", 2, 3, 4)), 24: (("k8", 4, 1, 4), 0, (256, 4, 128), ("k8_sliced", 2, 3, 4)), 40: (("k8", 4, 1, 4), 0, (256, 4, 128), ("k8_sliced", 2, 3, 4))},
    (256, 1280, 1280, 0): {12: (("k8", 2, 1, 4), 0, (128, 2, 128), ("k8", 1, 1, 4)), 24: (("k8", 4, 1, 4), 0, (256, 1, 128), ("k8", 2, 1, 4)), 40: (("k8", 4, 1, 4), 0, (256, 1, 128), ("k8", 2, 1, 4))},
    (256, 1280, 10240, 1): {12: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4)), 24: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4)), 40: (("k8", 4, 1, 4), 256, None, ("k8", 4, 1, 4))},
    (256, 5120, 1280, 0): {12: (("k8", 2, 1, 4), 0, (128, 2, 128), ("k8_sliced", 2, 6, 4)), 24: (("k8", 4, 1, 4), 0, (256, 1, 128), ("k8_sliced", 2, 6, 4)), 40: (("k8", 4, 1, 4), 0, (256, 1, 128), ("k8_sliced", 2, 6, 4))},
    (64, 1280, 1280, 0): {12: (("k8", 2, 1, 4), 0, None, ("k8", 2, 1, 4)), 24: (("k8", 1, 1, 4), 0, None, ("k8", 1, 1, 4)), 40: (("k8", 1, 1, 4), 0, None, ("k8", 1, 1, 4))},
    (64, 5120, 1280, 0): {12: (("k8_sliced", 2, 4, 4), 0, None, ("k8_sliced", 2, 6, 4)), 24: (("k8_sliced", 2, 2, 4), 0, None, ("k8_sliced", 2, 6, 4)), 40: (("k8", 2, 1, 4), 0, None, ("k8_sliced", 2, 6, 4))},
    (64, 1280, 10240, 1): {12: (("k8", 4, 1, 4), 0, None, ("k8", 2, 1, 4)), 24: (("k8", 4, 1, 4), 256, None, ("k8", 2, 1, 4)), 40: (("k8", 4, 1, 4), 256, None, ("k8", 2, 1, 4))},
}


@pytest.mark.parametrize("B", [12, 24, 40])
def test_gemm_planning_at_launch_set_batches(built, B):
    """gc_dn_gemm_selection at the CFG batches of a launch set (DESIGN.md 3.2 "Launch sets"), for the descriptors ops.conv3x3 / ops.linear build
    (workspace from gc_dn_gemm_workspace_bytes, channel partials asked for where the layout allows them).  The 8 x 8-map convs and the 16 -> 8
    stride-2 conv of a 24-frame set take the k-sliced 8-wave kernel on 256-row tiles (four whole images) x 4 slices (`img8`); at 12 frames the
    grid is small (128-row tiles), at 40 it fills a round unsliced.  Pure functions of the descriptor: no GPU needed."""
    from gaussctrl_amd.sd import ops
    lib = ctypes.CDLL(built)
    lib.gc_dn_gemm_workspace_bytes.restype = ctypes.c_size_t

    def finish(d, parts):
        ws = lib.gc_dn_gemm_workspace_bytes(ctypes.byref(d))
        if ws:
            d.workspace = 1; d.workspace_bytes = ws
        lay = None
        if parts and d.rows_per_batch >= 256:              # as ops._run_gemm: ask for partials where the layout exists (and <= 64 slabs)
            d.gn_groups = 32
            rows, ns, ct = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
            assert lib.gc_dn_gemm_chan_parts_layout(ctypes.byref(d), ctypes.byref(rows), ctypes.byref(ns), ctypes.byref(ct)) == 0
            if rows.value > 0 and ns.value <= 64:
                d.out_chan_parts = 1; lay = (rows.value, ns.value, ct.value)
            else:
                d.gn_groups = 0
        s = ops.gemm_selection(d)
        if lay is not None:           # partials of a k-sliced problem come from the reduce kernel (32-row slabs, 64-column blocks), else from the epilogue
            assert s["parts"] == (1 if s["splits"] > 1 else 2) and (lay[0] == 32) == (s["splits"] > 1), (s, lay)
            assert s["splits"] > 1 or lay[0] == 64 * s["m_tiles"], (s, lay)
        return s, lay

    def conv(H, cin, cout, stride, plan):
        d = ops.GemmDesc()
        Ho = H // stride
        d.dtype = 1; d.mode = 1; d.M, d.N, d.K = B * Ho * Ho, cout, 9 * cin
        d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.stride, d.pad_lo = B, H, H, cin, Ho, Ho, stride, 1
        d.rows_per_batch = Ho * Ho; d.out = 1; d.ldc = cout; d.lda = cin; d.zeros = 1
        d.plan_rows = Ho * Ho if plan else 0
        return finish(d, not plan)

    def lin(L, K, N, geglu, plan):
        d = ops.GemmDesc()
        d.dtype = 1; d.mode = 0; d.M, d.N, d.K = B * L, N, K
        d.lda = K; d.out = 1; d.ldc = N; d.zeros = 1; d.rows_per_batch = L; d.geglu = geglu
        d.plan_rows = L if plan else 0
        return finish(d, not plan and not geglu)

    key = lambda s: (s["kernel"], s["m_tiles"], s["splits"], s["ntw"])
    got, want = {}, {}
    for shape, row in _LAUNCH_SET_CONVS.items():
        (s, lay), (p, _) = conv(*shape, False), conv(*shape, True)
        got[("conv",) + shape] = (key(s), lay, key(p)); want[("conv",) + shape] = row[B]
    for shape, row in _LAUNCH_SET_LINEARS.items():
        (s, lay), (p, _) = lin(*shape, False), lin(*shape, True)
        got[("linear",) + shape] = (key(s), s["persist"], lay, key(p)); want[("linear",) + shape] = row[B]
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, bad
    if B == 24:      # the issue's anchor: the bench's 8 x 8-map convs, four whole images per 256-row tile x 4 slices
        for cin in (1280, 2560):
            assert got[("conv", 8, cin, 1280, 1)][0] == ("k8_sliced", 4, 4, 4)


def test_attention_selection_at_launch_set_batches(built):
    """gc_dn_attention_selection for the attention problems of a launch set (product form: self set + 4 sets from the cached reference bank; the
    text attention against 77 shared keys), with and without the set-split workspace (batch-invariant mode never offers it)."""
    from gaussctrl_amd.sd import ops
    lib = ctypes.CDLL(built)
    lib.gc_dn_attention_workspace_bytes.restype = ctypes.c_size_t

    def sel(B, L, D, nsets=5, Lk=None, ws=True, variant=0):
        d = ops.AttnDesc()
        d.dtype = 1; d.batch, d.heads, d.head_dim, d.Lq, d.Lk = B, 8, D, L, L if Lk is None else Lk
        d.frames_per_half = B // 2; d.nsets = nsets; d.q_prescaled = 1; d.kernel_variant = variant
        wsb = lib.gc_dn_attention_workspace_bytes(ctypes.byref(d))
        if ws and wsb:
            d.workspace = 1; d.workspace_bytes = wsb
        return ops.attention_selection(d)

    for B in (12, 24, 40):
        assert sel(B, 4096, 40) == "attn5" and sel(B, 4096, 40, nsets=4) == "attn5"
        assert sel(B, 4096, 40, variant=ops.GC_ATTN_VAR_K4) == "attn4" and sel(B, 4096, 40, variant=ops.GC_ATTN_VAR_D40_K3) == "attn3"
        assert sel(B, 4096, 40, variant=ops.GC_ATTN_VAR_ONLINE_ONLY) == "attn"
        assert sel(B, 1024, 80) == "attn3"
        assert sel(B, 256, 160) == "wide+combine" and sel(B, 256, 160, ws=False) == "attn"
        assert sel(B, 256, 160, variant=ops.GC_ATTN_VAR_D160_Q64) == ("attn+combine" if B == 12 else "attn")   # the 64-query form: set split while 4 x 8 x B < 512 workgroups
        assert sel(B, 64, 160) == "attn+combine" and sel(B, 64, 160, ws=False) == "attn"
        assert sel(B, 4096, 40, nsets=1, Lk=77) == "attn"                 # text keys: 2 key tiles, the pipelined kernels do not amortise
    assert sel(64, 64, 160) == "attn"                                     # 512 workgroups: a full grid, no set split
    assert sel(64, 256, 160, variant=ops.GC_ATTN_VAR_D160_Q64) == "attn"
    d = ops.AttnDesc()
    d.batch, d.heads, d.head_dim, d.Lq, d.Lk, d.nsets = 2, 8, 48, 64, 64, 1
    with pytest.raises(Exception):
        ops.attention_selection(d)


def _header_variant_enumerators():
    src = open(os.path.join(ROOT, "include", "gaussctrl_hip.h")).read()
    return sorted(set(re.findall(r"\b(GC_(?:GEMM|ATTN)_VAR_[A-Z0-9_]+) =", src)))


def test_variant_constants_match_the_header_and_do_not_overlap(tmp_path):
    """the GC_GEMM_VAR_* / GC_ATTN_VAR_* constants of gaussctrl_amd/sd/ops.py have the values the C compiler gives the header's enumerators, every
    enumerator has a Python counterpart and the reverse, and inside one kernel_variant field no two switches share a bit (bits 8..10 of the GEMM
    field once meant two things at once); every *_MASK field sits at its *_SHIFT."""
    import subprocess
    from gaussctrl_amd.sd import ops
    names = _header_variant_enumerators()
    assert len(names) >= 29, names            # 17 GEMM + 12 attention enumerators when this was written
    assert names == sorted(n for n in vars(ops) if re.match(r"GC_(GEMM|ATTN)_VAR_", n))
    src = tmp_path / "var.c"
    src.write_text('#include <stdio.h>\n#include "gaussctrl_hip.h"\nint main(void) {\n'
                   + "".join(f'    printf("{n} %d\\n", {n});\n' for n in names) + "    return 0;\n}\n")
    exe = tmp_path / "var"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())}
    assert got == {n: getattr(ops, n) for n in names}
    for kind in ("GC_GEMM_VAR_", "GC_ATTN_VAR_"):
        bits = {n: v for n, v in got.items() if n.startswith(kind) and not n.endswith("_SHIFT")}
        assert all(v > 0 for v in bits.values())
        clash = [(a, b) for a in bits for b in bits if a < b and bits[a] & bits[b]]
        assert not clash, clash
        for n, v in bits.items():
            if n.endswith("_MASK"):
                sh = got[n[:-5] + "_SHIFT"]
                assert v >> sh << sh == v and (v >> sh) & 1 and ((v >> sh) + 1) & (v >> sh) == 0, (n, v, sh)     # contiguous, lowest bit at the shift
            else:
                assert v & (v - 1) == 0, (n, v)


def test_options_from_env_keeps_every_documented_value():
    """options_from_env gives the integers it gave before the switches had names, for every GC_* variable of the README's table (literals:
    the values are frozen by bench.py, recorded profiles and the README); the epilogue timing ablations have a variable and bits of their own."""
    from gaussctrl_amd.sd import ops
    g = lambda **e: ops.options_from_env(e).gemm_variant
    a = lambda **e: ops.options_from_env(e).attn_variant
    assert g() == 0 and a() == 0 and ops.options_from_env({}) == ops.KernelOptions()
    assert [g(GC_GEMM_MT=v) for v in "234"] == [2, 3, 4]
    assert [g(GC_GEMM8=v) for v in "012"] == [0x10, 0, 0x20]
    assert [g(GC_GEMM_CONVSPLIT=v) for v in "012"] == [0x40, 0x80, 0]
    assert [g(GC_GEMM_DBG=v) for v in ("1", "2", "4", "8", "16", "31")] == [0x100, 0x200, 0x400, 0x800, 0x1000, 0x1f00]
    assert [g(GC_GEMM_SPLIT_MT=v) for v in "234"] == [2 << 24, 3 << 24, 4 << 24]
    assert [g(GC_GEMM_PW=v) for v in ("0", "1", "3", "7")] == [1 << 16, 2 << 16, 4 << 16, 8 << 16]
    assert g(GC_GEMM_MT="3", GC_GEMM8="2", GC_GEMM_DBG="5", GC_GEMM_PW="1") == 3 | 0x20 | 0x500 | (2 << 16)
    assert a(GC_ATTN_SAFE="1") == 1 and a(GC_ATTN_16="1") == 2 and [a(GC_ATTN_V=v) for v in ("1", "2", "4", "8", "16", "32")] == [4, 8, 16, 32, 64, 128]
    assert a(GC_ATTN_SAFE="1", GC_ATTN_16="1", GC_ATTN_V="4") == 19
    # the fused-statistics epilogue's timing ablations: bits 28..30 and nothing else; GC_GEMM_DBG no longer reaches them
    assert [g(GC_GEMM_EPI_ABL=v) for v in "124"] == [1 << 28, 2 << 28, 4 << 28]
    for v in "124":
        assert g(GC_GEMM_EPI_ABL=v) & ~ops.GC_GEMM_VAR_EPI_ABL_MASK == 0 and g(GC_GEMM_DBG=v) & ops.GC_GEMM_VAR_EPI_ABL_MASK == 0
    for v in ("32", "64", "128", "33", "-1"):              # (32 was passed by an old job script; nothing read it)
        with pytest.raises(ValueError):
            g(GC_GEMM_DBG=v)
    o = ops.options_from_env({"GC_BATCH_INVARIANT": "1", "GC_FUSED_HEAD": "0", "GC_FUSED_TAIL": "0", "GC_ABLATE": "gn,ln"})
    assert o.batch_invariant and not o.fused_head and not o.fused_tail and o.two_streams and o.ablate == frozenset({"gn", "ln"})


def test_undefined_variant_bits_are_refused(built):
    """kernel_variant bits no switch owns: gc_dn_gemm_selection / gc_dn_attention_selection return GC_EINVAL and name the bits (gc_dn_gemm and
    gc_dn_attention make the same two calls -- decode_variant, refuse_variant_bits -- among their argument checks, before anything is launched); the size and layout queries, which have no error
    channel, keep ignoring them; every defined bit passes."""
    from gaussctrl_amd.sd import ops
    lib = ctypes.CDLL(built)
    lib.gc_dn_gemm_workspace_bytes.restype = ctypes.c_size_t
    lib.gc_last_error_string.restype = ctypes.c_char_p
    d = ops.GemmDesc()
    d.dtype = 1; d.mode = 0; d.M, d.N, d.K = 6144, 640, 640
    d.lda = 640; d.out = 1; d.ldc = 640; d.zeros = 1; d.rows_per_batch = 1024
    sel = ops.GemmSelection()
    for bad in (0x8, 0x2000, 0x4000, 0x8000, 1 << 27, -(1 << 31)):
        d.kernel_variant = bad | ops.GC_GEMM_VAR_K4_ONLY
        assert lib.gc_dn_gemm_selection(ctypes.byref(d), ctypes.byref(sel)) == -1
        assert b"kernel_variant" in lib.gc_last_error_string() and ("0x%x" % (bad & 0xffffffff)).encode() in lib.gc_last_error_string()
        sizes = lib.gc_dn_gemm_workspace_bytes(ctypes.byref(d)), lib.gc_dn_gemm_row_stat_slots(ctypes.byref(d))
        d.kernel_variant = ops.GC_GEMM_VAR_K4_ONLY
        assert sizes == (lib.gc_dn_gemm_workspace_bytes(ctypes.byref(d)), lib.gc_dn_gemm_row_stat_slots(ctypes.byref(d))) and sizes[1] > 0
    a = ops.AttnDesc()
    a.dtype = 1; a.batch, a.heads, a.head_dim, a.Lq, a.Lk, a.nsets = 12, 8, 40, 4096, 4096, 5
    k = ctypes.c_int(0)
    for bad in (1 << 21, 1 << 24, -(1 << 31)):
        a.kernel_variant = bad | ops.GC_ATTN_VAR_K4
        assert lib.gc_dn_attention_selection(ctypes.byref(a), ctypes.byref(k)) == -1
        assert ("0x%x" % (bad & 0xffffffff)).encode() in lib.gc_last_error_string()
    all_gemm = 0
    for n, v in vars(ops).items():
        if n.startswith("GC_GEMM_VAR_") and not n.endswith("_SHIFT"):
            all_gemm |= v
    d.kernel_variant = all_gemm & ~(ops.GC_GEMM_VAR_MT_MASK ^ 4)       # every defined bit (MT field = 4)
    assert lib.gc_dn_gemm_selection(ctypes.byref(d), ctypes.byref(sel)) == 0
    a.kernel_variant = ops.GC_ATTN_VAR_ABL_MASK | ops.GC_ATTN_VAR_CSHIFT_MASK | 0xff
    assert lib.gc_dn_attention_selection(ctypes.byref(a), ctypes.byref(k)) == 0


def test_options_is_the_only_switch_state(built, monkeypatch):
    """ops.OPTIONS owns the switches: what configure() sets is what the compatibility view ops.KERNEL_VARIANT shows (bench.py reads it) and what
    the descriptors built by the launch path carry; KernelOptions keeps its fields (bench.py prints dataclasses.asdict(OPTIONS))."""
    import dataclasses
    from gaussctrl_amd.sd import ops
    assert list(dataclasses.asdict(ops.KernelOptions())) == ["gemm_variant", "attn_variant", "batch_invariant", "fused_head", "fused_tail", "two_streams", "gn_parts",
                                                            "tail_in_rows", "q_only", "ffout_merge", "text_fold", "cfg_share", "fp8_min_hw", "ablate"]
    assert ops.KernelOptions() == ops.KernelOptions(0, 0, False, True, True, True, True, True, True, True, True, True, 256, frozenset())
    keep = ops.OPTIONS
    X = ops.GC_GEMM_VAR_NO_PERSIST | 3
    try:
        got = ops.configure(gemm_variant=X, attn_variant=ops.GC_ATTN_VAR_K4, batch_invariant=True)
        assert got is ops.OPTIONS and ops.KERNEL_VARIANT == {"gemm": X, "attn": ops.GC_ATTN_VAR_K4}
        view = ops.KERNEL_VARIANT
        view["gemm"] = 0                                   # a view: writing to it changes nothing
        assert ops.KERNEL_VARIANT == {"gemm": X, "attn": ops.GC_ATTN_VAR_K4} and ops.OPTIONS.gemm_variant == X
        ops.BATCH_INVARIANT = False                        # the old global's name: an assignment lands in OPTIONS
        assert ops.OPTIONS.batch_invariant is False and ops.OPTIONS.gemm_variant == X
        monkeypatch.setattr(ops, "BATCH_INVARIANT", True)
        assert ops.OPTIONS.batch_invariant is True and ops.BATCH_INVARIANT is True

        class Stop(Exception):
            pass

        class Lib:                                         # the library as _run_gemm sees it, stopped at its first query
            def gc_dn_gemm_workspace_bytes(self, ref):
                raise Stop
        monkeypatch.setattr(ops.L, "lib", lambda: Lib())
        monkeypatch.setitem(ops._zero_page, "cpu", type("Z", (), {"data_ptr": lambda self: 64})())
        d = ops.GemmDesc()
        with pytest.raises(Stop):
            ops._run_gemm(d, "cpu")
        assert d.kernel_variant == X
    finally:
        ops.configure(keep)
    assert ops.KERNEL_VARIANT == {"gemm": keep.gemm_variant, "attn": keep.attn_variant}

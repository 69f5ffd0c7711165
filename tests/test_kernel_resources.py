"""CPU: private (scratch) memory and register spills of the shipped gfx950 kernels, read from the AMDGPU metadata of the code objects in the built
library ("no compiler-generated VMEM access in the k loop").

The LDS-DMA ring of k_gemm8 / k_gemm8q / k_gemm8p and the operand stream of k_thead / k_ttail are ordered by COUNTED s_waitcnt vmcnt(N): the DMA is
issued from inline asm, so the compiler's wait-count pass does not know those loads are in flight.  A scratch load the compiler puts into such a
loop is waited for with vmcnt(0), which drains the ring every k-tile; a scratch store counts in vmcnt and makes the next counted wait stricter
than written.  So these kernels use no private memory at all: .private_segment_fixed_size == 0 and .vgpr_spill_count == 0.
Only metadata keys are read (.name, .private_segment_fixed_size, .vgpr_spill_count), no instruction text."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = "/opt/rocm/lib/llvm/bin"

# Kernels deliberately left with private memory: regex on the demangled name -> (private bytes, spilled VGPRs) as built today.  More fails.
# All three are the FUSE = true ("everything" epilogue, wave_epilogue) instantiations of the largest wave tile (NTW 5 x MT 4 = 80 accumulators
# at the 256-register cap of a 512-thread workgroup): the spills sit in the epilogue, behind the k loop -- 80 accumulators + bias + LayerNorm
# column sums + the residuals of every m-tile + the GroupNorm channel sums do not fit.  The k loops of these kernels are scratch-free like the
# others (the cursor fix is in the shared template).  The benchmark launches none of them (its fused-statistics convs run the CS epilogue).
ALLOWED = {
    r"k_gemm8<dn::(BF16|F16), 1, 5, 4, true, false, false, 0>": (140, 40),
    r"k_gemm8<dn::(BF16|F16), 2, 5, 4, true, false, false, 0>": (132, 38),
    r"k_gemm8<dn::(BF16|F16), 3, 5, 4, true, false, false, 0>": (132, 38),
}
# the k_attn5 instantiation the benchmark launches (profiles/r06_bench_kernel_stats_bf16_final.txt), and its f16 twin
BENCH_ATTN5 = r"k_attn5<dn::(BF16|F16), true, 4, false, true>"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")):
        ge.build()
    return os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")


def kernel_resources(lib):
    """{demangled kernel name: (private_segment_fixed_size, vgpr_spill_count)} over every code object of the library."""
    spec = importlib.util.spec_from_file_location("packed_fp32_audit", os.path.join(ROOT, "scripts", "packed_fp32_audit.py"))
    audit = importlib.util.module_from_spec(spec); spec.loader.exec_module(audit)
    out = {}
    for co in audit.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co); f.flush()
            notes = subprocess.run([f"{BIN}/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
        # a kernel's keys are sorted and share one indentation: ... .name, .private_segment_fixed_size, ..., .vgpr_spill_count, ...
        lines = notes.splitlines()
        for i, line in enumerate(lines):
            m = re.match(r"^(\s+)\.private_segment_fixed_size:\s+(\d+)\s*$", line)
            if not m:
                continue
            ind = re.escape(m.group(1))
            name = next(n.group(1) for n in (re.match(rf"^{ind}\.name:\s+(\S+)\s*$", l) for l in reversed(lines[:i])) if n)
            spill = next(int(n.group(1)) for n in (re.match(rf"^{ind}\.vgpr_spill_count:\s+(\d+)\s*$", l) for l in lines[i:]) if n)
            out[name.strip("'\"")] = (int(m.group(2)), spill)
    names = sorted(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(dem) == len(names)
    return {d: out[n] for d, n in zip(dem, names)}


@pytest.fixture(scope="module")
def kernels(built):
    return kernel_resources(built)


def _gemm8_mode(name):
    m = re.search(r"\bk_gemm8<[^,]+, (\d+),", name)
    return int(m.group(1)) if m else None


def _allowed(name):
    return next((v for p, v in ALLOWED.items() if re.search(p, name)), None)


def test_every_code_object_was_read(kernels):
    assert len(kernels) > 300, len(kernels)
    for fam in ("k_gemm8<", "k_gemm8p<", "k_gemm8q<", "k_thead<", "k_ttail<", "k_attn5<"):
        assert sum(fam in k for k in kernels) >= 2, fam          # bf16 and f16
    for mode in (0, 1, 2, 3, 4):
        assert any(_gemm8_mode(k) == mode for k in kernels), mode


def test_hot_kernels_use_no_private_memory(kernels):
    """every k_gemm8 (MODE 0 .. 4: generic / fast / upsample-fused convs and linears), k_gemm8p, k_gemm8q, k_thead, k_ttail: no scratch, no
    spills -- except the allow-listed fused-epilogue instantiations, which are held at their recorded numbers"""
    bad = {}
    for k, v in kernels.items():
        if not (_gemm8_mode(k) is not None or re.search(r"\bk_gemm8[pq]<|\bk_thead<|\bk_ttail<", k)):
            continue
        lim = _allowed(k) or (0, 0)
        if v[0] > lim[0] or v[1] > lim[1]:
            bad[k] = (v, lim)
    assert not bad, "\n".join(f"{v} > {lim}  {k}" for k, (v, lim) in sorted(bad.items()))


def test_allow_list_is_current(kernels):
    """every allow-list entry names kernels that exist (bf16 and f16) and still need the allowance: an entry that became clean must go"""
    for p, lim in ALLOWED.items():
        hit = {k: v for k, v in kernels.items() if re.search(p, k)}
        assert len(hit) == 2, (p, sorted(hit))
        assert any(v != (0, 0) for v in hit.values()), p


def kernel_vgprs(lib, pattern):
    """{demangled kernel name: .vgpr_count} of the kernels whose demangled name matches `pattern` (metadata keys only, as above)"""
    spec = importlib.util.spec_from_file_location("packed_fp32_audit", os.path.join(ROOT, "scripts", "packed_fp32_audit.py"))
    audit = importlib.util.module_from_spec(spec); spec.loader.exec_module(audit)
    out = {}
    for co in audit.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co); f.flush()
            notes = subprocess.run([f"{BIN}/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
        lines = notes.splitlines()
        for i, line in enumerate(lines):
            m = re.match(r"^(\s+)\.vgpr_count:\s+(\d+)\s*$", line)
            if m:
                ind = re.escape(m.group(1))
                name = next(n.group(1) for n in (re.match(rf"^{ind}\.name:\s+(\S+)\s*$", l) for l in reversed(lines[:i])) if n)
                out[name.strip("'\"")] = int(m.group(2))
    names = sorted(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {d: out[n] for d, n in zip(dem, names) if re.search(pattern, d)}


def test_persistent_gemm_keeps_one_accumulator_set(built):
    """k_gemm8p runs k_gemm8's k loop (ring_loop in csrc/dn_gemm_kernels.h): ONE copy of the tail's second MFMA block, so the allocator keeps one
    set of the 64 accumulators -- 169 VGPRs (LNV 0) / 179 (LNV 2) as built today; with a copy in either arm of the tail's branch it kept two
    (232 / 242).  ring_loop's form depends on how the optimiser treats it before it is inlined (its trip count arrives by const reference for
    that reason): a compiler that rewrites it shows here, without a second build to compare with.  More fails."""
    v = kernel_vgprs(built, r"\bk_gemm8p<")
    assert len(v) == 4, sorted(v)
    for k, n in v.items():
        lim = 179 if re.search(r"k_gemm8p<dn::(BF16|F16), 4, 4, 2>", k) else 169
        assert n <= lim, (k, n, lim)


def test_bench_attention_kernel_uses_no_private_memory(kernels):
    hit = {k: v for k, v in kernels.items() if re.search(BENCH_ATTN5, k)}
    assert len(hit) == 2, sorted(hit)
    assert all(v == (0, 0) for v in hit.values()), hit


def test_densification_kernels_use_no_private_memory(kernels):
    """every k_refine_* and k_mcmc_* kernel (csrc/train_refine.hip, train_mcmc.hip on the shared csrc/train_rows.h): no scratch, no spilled
    VGPRs.  The header hands per-lane state (row values, child rows, masks) in and out by value; a helper that advanced a caller's array
    through a reference would show here first.  The count is asserted so that no kernel is silently missed."""
    hit = {k: v for k, v in kernels.items() if re.search(r"\bk_(refine|mcmc)_", k)}
    assert len(hit) == 22, sorted(hit)
    assert all(v == (0, 0) for v in hit.values()), {k: v for k, v in hit.items() if v != (0, 0)}


def test_compositing_kernels_use_no_private_memory(kernels):
    """the 18 tile compositors (csrc/raster_composite.hip, raster_composite_nd.hip on the shared csrc/raster_tile.h): k_rasterize_fwd x 2,
    k_rasterize_bwd x 4, k_rasterize_nd_fwd / _bwd x 6 channel widths each -- no scratch, no spilled VGPRs.  The header's pieces hand the pixel
    and pair state in and out by value, and the staged record is stored before the culling mask's branches; a piece that kept either in
    memory would show here first.  The counts are asserted so that no instantiation is silently missed."""
    want = {r"\bk_rasterize_fwd<": 2, r"\bk_rasterize_bwd<": 4, r"\bk_rasterize_nd_fwd<": 6, r"\bk_rasterize_nd_bwd<": 6}
    hit = {}
    for p, n in want.items():
        fam = {k: v for k, v in kernels.items() if re.search(p, k)}
        assert len(fam) == n, (p, sorted(fam))
        hit.update(fam)
    assert len(hit) == 18, sorted(hit)
    assert all(v == (0, 0) for v in hit.values()), {k: v for k, v in hit.items() if v != (0, 0)}


def test_attention_kernels_use_no_private_memory(kernels):
    """every kernel of csrc/dn_attn.hip -- k_attn x 14, k_attn3 x 16, k_attn4 x 24, k_attn_wide x 2, k_attn_combine x 2 -- and the four product
    instantiations of k_attn5: no scratch, no spilled VGPRs.  In k_attn3 / k_attn4 / k_attn5 a scratch access drains the K / V^T DMA ring on
    every tile, and a prologue helper that chose between the addresses of two pointer fields of the argument block kept the whole 224-byte
    block in private memory (csrc/dn_attn_common.h).  The instrumented (timing-ablation) instantiation of k_attn5 is held at its recorded
    numbers.  The counts are asserted so that no instantiation is silently missed."""
    want = {r"\bk_attn<": 14, r"\bk_attn3<": 16, r"\bk_attn4<": 24, r"\bk_attn_wide<": 2, r"\bk_attn_combine<": 2}
    hit = {}
    for p, n in want.items():
        fam = {k: v for k, v in kernels.items() if re.search(p, k)}
        assert len(fam) == n, (p, sorted(fam))
        hit.update(fam)
    assert len(hit) == 58, sorted(hit)
    k5 = {k: v for k, v in kernels.items() if re.search(r"\bk_attn5<", k)}
    assert len(k5) == 5, sorted(k5)
    abl = {k: v for k, v in k5.items() if re.search(r"k_attn5<dn::BF16, true, 4, true, false>", k)}
    assert len(abl) == 1, sorted(k5)
    hit.update({k: v for k, v in k5.items() if k not in abl})
    assert len(hit) == 62
    assert all(v == (0, 0) for v in hit.values()), {k: v for k, v in hit.items() if v != (0, 0)}
    (v,) = abl.values()
    assert v[0] <= 124 and v[1] <= 46, abl

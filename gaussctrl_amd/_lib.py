"""ctypes loader of libgaussctrl_hip.so (the C-ABI of include/gaussctrl_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol cannot be resolved
this module raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported
from here.)

Every entry point is bound with its argument and return types from ONE table, ABI below, and the ops modules reach the library
through ONE function, call(name, *args) with plain ints, floats, tensors and None.  The table is Python text, not read from the
headers; tests/test_binding_cpu.py holds it to include/*.h name by name and letter by letter.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GC_HIP_LIB") or os.path.join(_HERE, "libgaussctrl_hip.so")   # GC_HIP_LIB: kernel-experiment builds only

# header -> entry point (in the header's order) -> "<return>:<one letter per parameter>".
#   parameters  i int   q int64_t   f float   z size_t   p any pointer (device, host array, byref(descriptor), NULL)
#               s the trailing `void *stream`: call() appends the current stream itself
#   return      e status code, checked by call()   i plain int value   z size_t   c const char *   v void
ABI = {
    "gaussctrl_hip.h": {
        "gc_last_error_string": "c:", "gc_abi_version": "i:", "gc_project_gaussians_fwd": "e:qppfpppffffiiiifpppppps",
        "gc_project_gaussians_bwd": "e:qppfpppffffiipppppppps", "gc_sh_fwd": "e:qiippps", "gc_sh_bwd": "e:qiippps",
        "gc_raster_scan_workspace_bytes": "z:q", "gc_raster_scan_tiles": "e:qppppzs", "gc_raster_read_count": "e:pps",
        "gc_raster_map_intersects": "e:qqppppiipps", "gc_raster_pad_intersects": "e:qpipps", "gc_raster_sort_workspace_bytes": "z:qi",
        "gc_raster_sort_intersects": "e:qipppppzs", "gc_raster_tile_bins": "e:qipps", "gc_raster_depth_order_workspace_bytes": "z:q",
        "gc_raster_depth_order": "e:qpppppppzs", "gc_raster_bin_workspace_bytes": "z:q", "gc_raster_bin_tiles": "e:qqpppppiippppzs",
        "gc_raster_bin_tiles_dev": "e:qqpppppppiippppzs", "gc_raster_bin_tiles_boxes": "e:qqppppppiippppzs",
        "gc_rasterize_fwd": "e:iiiipppppppppppps", "gc_rasterize_bwd": "e:iiiiqppppppppppppppps",
        "gc_rasterize_bwd_clamped": "e:iiiiqpppppppppppppppps", "gc_rasterize_nd_fwd": "e:iiiiipppppppppps",
        "gc_rasterize_nd_bwd": "e:iiiiqippppppppppppppps", "gc_project_sh_fwd": "e:qppppppiipppffffiiiifppppppps",
        "gc_project_sh_fwd_boxes": "e:qppppppiipppffffiiiifpppppppps", "gc_project_sh_bwd": "e:qpppppiipppffffiipppppppppppps",
        "gc_project_sh_bwd_accumulate": "e:qpppppiipppffffiipppppppppppps", "gc_raster_finalize": "e:qpppps", "gc_raster_finalize_into": "e:qppppps",
        "gc_l1_ssim_workspace_bytes": "z:iii", "gc_l1_ssim_fwd_bwd": "e:ppiiiffipppzs", "gc_adam_step": "e:ppppqffffis",
        "gc_project_sh_fwd_views": "e:qippppppiipiiiifppppppppps", "gc_project_sh_bwd_views": "e:qiipppppiipiipppppppppppps",
        "gc_raster_scan_tiles_views": "e:qipppppzqs", "gc_raster_depth_order_views_workspace_bytes": "z:qi",
        "gc_raster_depth_order_views": "e:qippppppppzs", "gc_raster_bin_views_workspace_bytes": "z:qi",
        "gc_raster_bin_tiles_views": "e:qiqppppppiippppzs", "gc_raster_order_boxes_views_workspace_bytes": "z:qi",
        "gc_raster_order_boxes_views": "e:qippppppppzs", "gc_raster_bin_sorted_views": "e:qiqppppppiipppzs",
        "gc_rasterize_fwd_views": "e:iqqiiiiiipppppppppppps", "gc_rasterize_bwd_views": "e:iqqiiiiiipppppppppppppppps",
        "gc_l1_ssim_views_workspace_bytes": "z:iiii", "gc_l1_ssim_fwd_bwd_views": "e:ippiiiffipppzs",
        "gc_rasterize_bwd_depth_views": "e:iqqiiiiiipppppppppppppppppppps", "gc_project_sh_bwd_depth_views": "e:qiipppppiipiippppppppppppps",
        "gc_depth_l1_views_workspace_bytes": "z:iii", "gc_depth_l1_fwd_bwd_views": "e:ippiifpppzs", "gc_dn_gemm_workspace_bytes": "z:p",
        "gc_dn_gemm_row_stat_slots": "i:p", "gc_dn_gemm_chan_parts_layout": "e:pppp", "gc_dn_gemm_selection": "e:pp", "gc_dn_gemm": "e:ps",
        "gc_dn_attention_workspace_bytes": "z:p", "gc_dn_attention_selection": "e:pp", "gc_dn_attention": "e:ps", "gc_dn_transformer_tail": "e:ps",
        "gc_dn_transformer_tail_layout": "v:pppp", "gc_dn_transformer_head": "e:ps", "gc_dn_groupnorm_workspace_bytes": "z:qqi",
        "gc_dn_groupnorm": "e:ippqqiippfips", "gc_dn_groupnorm_coef": "e:ipqqiippfpps", "gc_dn_groupnorm_apply": "e:ippqqiippfips",
        "gc_dn_groupnorm_apply_fp8": "e:ippqqiiippfipis", "gc_dn_group_stats": "e:ipqqiips", "gc_dn_layernorm": "e:ippqippfs",
        "gc_dn_layernorm_fp8": "e:ippqippfis", "gc_dn_concat_add": "e:ipippipqqpis", "gc_dn_groupnorm_apply_parts": "e:ippqqiippfipqiiis",
        "gc_dn_groupnorm_apply_parts_fp8": "e:ippqqiiippfipqiiiis", "gc_dn_groupnorm_coef_parts": "e:qqiippfpqiiips",
        "gc_dn_concat_parts_layout": "e:qiippp", "gc_dn_concat_add_parts": "e:ipippipqqips", "gc_dn_axpby": "e:ipfpfipqs",
        "gc_dn_cast_f32": "e:ipipqs", "gc_dn_softmax_rows": "e:ipqqqfs", "gc_dn_depth_to_disparity": "e:ipqpps", "gc_dn_mask_composite": "e:pipppqs",
        "gc_dn_cfg_ddim_step": "e:ipiqqfiffppis",
    },
    "gaussctrl_absgrad.h": {
        "gc_rasterize_bwd_abs_views": "e:iqqiiiiiippppppppppppppppppppps",
    },
    "gaussctrl_antialias.h": {
        "gc_project_sh_fwd_aa_views": "e:qippppppiipiiiifpppppppppps", "gc_project_sh_bwd_aa_views": "e:qiipppppiipiipppppppppppppps",
    },
    "gaussctrl_bilagrid.h": {
        "gcx_bilagrid_slice_fwd_views": "e:iiiiiiipppps", "gcx_bilagrid_slice_bwd_views": "e:iiiiiiipppppps",
        "gcx_bilagrid_tv_workspace_bytes": "z:iiii", "gcx_bilagrid_tv_fwd_bwd": "e:iiiipfpppzs",
    },
    "gaussctrl_mcmc.h": {
        "gc_mcmc_dead_workspace_bytes": "z:q", "gc_mcmc_dead": "e:qpfppppzs", "gc_mcmc_relocate": "e:qqippfpppps",
        "gc_mcmc_inject_noise": "e:qpppppfs",
    },
    "gaussctrl_pose.h": {
        "gcx_pose_bwd_views_workspace_bytes": "z:qi", "gcx_pose_bwd_views": "e:qiipppppiipppppppps",
    },
    "gaussctrl_refine.h": {
        "gc_refine_accumulate_views": "e:qippfppps", "gc_refine_plan_workspace_bytes": "z:q", "gc_refine_plan": "e:qpppppiifffiffififppppzs",
        "gc_refine_apply": "e:qiiqqqppppppppps", "gc_refine_reset_opacity": "e:qfppps",
    },
    "gaussctrl_trace.h": {
        "gc_trace_mask_views": "e:iqqiiiiipppppppps", "gc_trace_select": "e:qppffpps", "gc_adam_step_rows": "e:ppppqipffffis",
    },
}

SIGNATURES = {name: sig for names in ABI.values() for name, sig in names.items()}
# views of the table, kept under their older names: the counted entry points (prefix gc_), and the extension sets (prefix gcx_, headers of
# their own) that tests/test_bilagrid_abi_cpu.py and tests/test_pose_abi_cpu.py check header by header
SYMBOLS = [s for s in SIGNATURES if s.startswith("gc_")]
EXT_SYMBOLS = list(ABI["gaussctrl_bilagrid.h"])
POSE_SYMBOLS = list(ABI["gaussctrl_pose.h"])
EXT_SETS = {"gaussctrl_bilagrid.h": EXT_SYMBOLS, "gaussctrl_pose.h": POSE_SYMBOLS}

# Extension headers in subdirectories of include/ (same alphabet, prefix gcx_): bound and called like every entry of ABI, kept in a table of
# their own so that the views above stay what they were.  tests/test_distort_cpu.py holds it to include/ext/*.h.
EXT_ABI = {
    "ext/gaussctrl_distort.h": {
        "gcx_distort_fwd_views": "e:iqqiiiiippppppiffpps", "gcx_distort_bwd_views": "e:iqqiiiiippppppiffpppppppps",
    },
}
EXT_SIGNATURES = {name: sig for names in EXT_ABI.values() for name, sig in names.items()}
_BOUND = {**SIGNATURES, **EXT_SIGNATURES}

ARG_TYPES = {"i": C.c_int, "q": C.c_int64, "f": C.c_float, "z": C.c_size_t, "p": C.c_void_p, "s": C.c_void_p}
RETURN_TYPES = {"e": C.c_int, "i": C.c_int, "z": C.c_size_t, "c": C.c_char_p, "v": None}


def _plan(sig):
    """what call() needs of a signature: return kind, arguments the caller passes, whether the stream is appended, pointer positions"""
    kind, letters = sig.split(":")
    stream = letters.endswith("s")
    return kind, len(letters) - stream, stream, tuple(i for i, c in enumerate(letters) if c == "p")


_PLANS = {name: _plan(sig) for name, sig in _BOUND.items()}
_HAS_DATA_PTR = {}          # type of a pointer argument -> it is a tensor (has data_ptr), not None / an int / a host ctypes object

_lib = None


class GaussCtrlHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GaussCtrlHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
        l = C.CDLL(LIB_PATH)
        for s in _BOUND:
            if not hasattr(l, s):
                raise GaussCtrlHipError(f"libgaussctrl_hip.so does not export {s}")
        for s, sig in _BOUND.items():
            kind, letters = sig.split(":")
            fn = getattr(l, s)
            fn.restype = RETURN_TYPES[kind]
            fn.argtypes = [ARG_TYPES[c] for c in letters]
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().gc_last_error_string().decode("utf-8", "replace")
        raise GaussCtrlHipError(f"{what} failed (code {rc}): {msg}")


def call(name, *args):
    """The one way the ops modules enter the library: `args` are the header's arguments without the stream -- plain ints and floats,
    tensors (or anything else with data_ptr) / None / host ctypes objects for pointers.  The function is looked up on the handle at every
    call (tests and the benchmark put recording proxies at `_lib`), the current stream is looked up at every call and appended where the
    table says so; a non-zero status raises GaussCtrlHipError, every other return kind is handed back."""
    kind, n, stream, pointers = _PLANS[name]
    if len(args) != n:
        raise TypeError(f"{name} takes {n} arguments{' and the stream' if stream else ''}, got {len(args)}")
    fn = getattr(lib(), name)
    for i in pointers:
        a = args[i]
        has = _HAS_DATA_PTR.get(a.__class__)
        if has is None:
            has = _HAS_DATA_PTR[a.__class__] = hasattr(a.__class__, "data_ptr")
        if has:
            if args.__class__ is tuple:
                args = list(args)
            args[i] = a.data_ptr()
    rc = fn(*args, stream_handle()) if stream else fn(*args)
    if rc and kind == "e":
        check(rc, name)
    return rc


def need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise GaussCtrlHipError("gaussctrl_amd ops need GPU tensors (HIP path only; no CPU fallback)")


def ptr(t):
    """device pointer of a torch tensor (or NULL for None) as c_void_p."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


def host_floats(values):
    """small host float array (camera matrices) -> ctypes float array."""
    vals = [float(v) for v in values]
    return (C.c_float * len(vals))(*vals)


_raw_stream = None


def stream_handle():
    """raw hipStream_t of torch's current stream on the current device, as an int.  The host enqueues ~13 000 launches per 3-view chunk:
    through torch.cuda.current_stream() this lookup alone was 84 of the 275 ms of host time per chunk (scripts/cpu_bound_check.py); the raw
    lookup is ~0.3 us instead of ~8 us."""
    global _raw_stream
    if _raw_stream is None:
        import torch
        raw, device = getattr(torch._C, "_cuda_getCurrentRawStream", None), torch.cuda.current_device
        _raw_stream = (lambda: raw(device())) if raw is not None else (lambda: torch.cuda.current_stream().cuda_stream)
    return _raw_stream()


def stream_ptr():
    return C.c_void_p(stream_handle())


i64 = C.c_int64
i32 = C.c_int
f32 = C.c_float

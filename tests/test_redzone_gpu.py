"""The existing small-shape GPU tests, run again with every buffer inside a red-zone arena (tests/_redzone.py).

Each case calls an existing test function at one of its own parametrisations inside guard(...): `torch` of the product modules that allocate,
and of the test modules whose code runs, is the arena's proxy, so outputs, workspaces and the inputs the tests build with torch factories are
carved with a poisoned zone behind each.  Every oracle comparison and every bar of the wrapped test applies unchanged, and no tolerance is
added: whatever is computed from an over-read float is NaN and fails the wrapped test's own comparison, and whatever is stored outside a buffer
fails the zone check.  Inputs a wrapped test still moves with .to(device) / .cuda(), and the gradients autograd allocates, are torch's own: there
only outputs and workspaces are guarded (the share of such pointers is in the margins log, "red zone: share of device pointers outside")."""
import importlib
import inspect
import os
import sys
import types

import pytest
import torch

from _redzone import guard

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
_TESTS = os.path.dirname(os.path.abspath(__file__))
SMALL0 = (5000, 200, 136, 180.0, 0.03)             # test_raster_nd_gpu.SMALL[0]


def _c(module_, test_, **kw):
    return (module_, test_, kw)


def _both(module_, test_, key="dt", **kw):
    return [(module_, test_, dict(kw, **{key: d})) for d in (BF, HF)]


R, V, ND, DP, AA = "test_raster_gpu", "test_raster_views_gpu", "test_raster_nd_gpu", "test_raster_depth_gpu", "test_raster_antialias_gpu"
RF, MC, DK, TT, TS = "test_refine_gpu", "test_mcmc_gpu", "test_denoise_kernels_gpu", "test_ttail_gpu", "test_train_step_gpu"

CASES = [
    # raster operator surface
    _c(R, "test_rasterize_ops_fwd_bwd", N=3, W=40, H=24, fx=50.0, sm=0.2),
    _c(R, "test_rasterize_ops_fwd_bwd", N=5000, W=200, H=136, fx=180.0, sm=0.03),
    _c(R, "test_sh_fwd_bwd"),
    _c(R, "test_project_gaussians_bit_exact", N=1, W=64, H=64, fx=100.0),
    _c(R, "test_project_gaussians_bit_exact", N=5000, W=200, H=136, fx=180.0),
    # binning: 28, 63 and 117 tiles (every staged-pass shape), each with the capacity subcases int(M * 1.3) + 7, M exactly and M // 2
    _c(R, "test_bin_and_sort_bit_exact", N=3000, W=100, H=60, fx=90.0),
    _c(R, "test_bin_and_sort_bit_exact", N=4000, W=130, H=100, fx=110.0),
    _c(R, "test_bin_and_sort_bit_exact", N=5000, W=200, H=136, fx=180.0),
    # fused render
    _c(R, "test_fused_render_view", N=7, W=33, H=17, fx=40.0, sm=0.3, training=False),
    _c(R, "test_fused_render_view", N=5000, W=200, H=136, fx=180.0, sm=0.03, training=False),
    _c(R, "test_tight_tile_boxes_same_images_and_gradients"),
    _c(R, "test_empty_and_all_culled"),
    # views (N = 299: the scalar tails of the 16-byte staging; C = 11 crosses the 8-views-per-launch split)
    *[_c(V, "test_every_sh_width_and_colour_mode_single_view_vs_views", deg=d) for d in (0, 1, 2, 3)],
    _c(V, "test_sorted_boxes_chain_bit_identical_to_the_pair_chain", N=7, W=33, H=17, fx=40.0, sm=0.3, C=2, behind=False),
    _c(V, "test_sorted_boxes_chain_bit_identical_to_the_pair_chain", N=4097, W=64, H=64, fx=70.0, sm=0.05, C=1, behind=True),
    _c(V, "test_sorted_boxes_chain_all_culled_and_capacity"),
    _c(V, "test_render_views_sync_free_capacity_and_overflow"),
    _c(V, "test_render_views_bit_identical_to_single_view", N=20000, W=200, H=136, fx=180.0, sm=0.03, C=11),
    _c("test_render_view_vs_views_gpu", "test_render_view_is_render_views_of_one_camera", depth_grad=True, absgrad=True, antialiased=True, into=True),
    _c("test_render_view_vs_views_gpu", "test_render_view_is_render_views_of_one_camera", depth_grad=False, absgrad=False, antialiased=False,
       into=False),
    # N-channel, depth, antialias, absgrad
    *[_c(ND, "test_forward_vs_fp64_oracle", scene=SMALL0, C=c) for c in (1, 5, 33)],
    *[_c(ND, "test_backward_vs_fp64_autograd", scene=SMALL0, C=c) for c in (1, 33)],
    _c(ND, "test_image_size_not_a_multiple_of_16", W=37, H=29),
    _c(DP, "test_depth_grad_single_view", name="b"),
    _c(DP, "test_depth_grad_views", C=3),
    _c(AA, "test_antialiased_single_view", name="b"),
    _c(AA, "test_antialiased_views_gradients", C=9),
    _c("test_absgrad_gpu", "test_absgrad_views"),
    # projection / SH kernels alone, camera inside the cloud (N = 299: the staging tails; C = 9 crosses the 8-views-per-launch split)
    _c("test_project_vjp_gpu", "test_fused_single_view", name="tiny", deg=3, n_use=3),
    _c("test_project_vjp_gpu", "test_views_backward", C=9),
    # compositing backward alone on crafted tile lists (tiny: the staging tails; deep: one to three backward batches)
    *[_c("test_composite_vjp_gpu", "test_bwd_clamped", name=n, cset="a") for n in ("tiny", "deep")],
    *[_c("test_composite_vjp_gpu", "test_bwd_views", name=n, shared=False) for n in ("tiny", "deep")],
    # training step
    _c("test_plugin_gpu", "test_l1_ssim_loss_and_fused_adam"),
    _c(V, "test_l1_ssim_loss_views_matches_per_image"),
    _c(DP, "test_depth_l1_loss"),
    _c("test_dist_gpu", "test_sharded_adam_slice_update_is_the_fused_adam_kernel"),
    # training step against float64: below the window, one SSIM pixel, tiles + 1 at C = 4; the batched loss; Adam's chunk tails
    *[_c(TS, "test_l1_ssim_vs_float64", H=h, W=w, C=c) for h, w, c in ((1, 1, 1), (11, 11, 3), (17, 33, 4))],
    _c(TS, "test_l1_ssim_views_vs_float64_per_image"),
    *[_c(TS, "test_adam_vs_float64", n=n) for n in (5, 1025)],
    # densification
    *[_c(RF, "test_accumulate", N=n, C=c) for n in (1, 255, 257) for c in (1, 3)],
    _c(RF, "test_plan_apply_mixed", N=257, ns=2),
    _c(RF, "test_plan_apply_mixed", N=257, ns=3),
    _c(RF, "test_plan_apply_edge_populations"),
    _c(RF, "test_reset_opacity", N=257),
    _c(MC, "test_dead", N=1),
    _c(MC, "test_dead", N=257),
    _c(MC, "test_relocate", N=257, inplace=True),
    _c(MC, "test_relocate", N=257, inplace=False),
    *[_c(MC, "test_relocate_sh_widths_and_missing_moments", rest_k=k, moments=m) for k, m in ((0, "all"), (3, "some"), (15, "none"), (3, "none"),
                                                                                              (15, "some"))],
    _c(MC, "test_inject_noise", N=257),
    # denoise kernels, both activation types
    *[c for M, N, K in ((14, 1280, 320), (154, 320, 768), (1000, 640, 2560)) for c in _both(DK, "test_linear", M=M, N=N, K=K)],
    *_both(DK, "test_linear_geglu_rowvec_transposed"),
    *[c for B, H, W, Cin, Cout, stride, ups in ((2, 9, 7, 96, 96, 2, False), (2, 8, 8, 64, 64, 1, True), (2, 32, 32, 8, 320, 1, False))
      for c in _both(DK, "test_conv3x3", B=B, H=H, W=W, Cin=Cin, Cout=Cout, stride=stride, ups=ups)],
    *[c for B, HW, C, G in ((1, 4, 1920, 32), (2, 36, 960, 32)) for c in _both(DK, "test_groupnorm", B=B, HW=HW, C=C, G=G)],
    *[c for kind, B, H, Cin, Cout in (("conv", 2, 32, 320, 640), ("linear", 2, 64, 320, 320), ("concat", 2, 16, 1280, 640))
      for c in _both(DK, "test_groupnorm_from_producer_partials", kind=kind, B=B, H=H, Cin=Cin, Cout=Cout)],
    *[c for M, C in ((5, 64), (77, 640)) for c in _both(DK, "test_layernorm", M=M, C=C)],
    *[c for f, L, heads, D, coeff in ((5, 70, 2, 8, 0.6), (7, 100, 8, 80, 0.6), (6, 4, 8, 160, 0.6), (5, 136, 2, 80, 0.6))
      for c in _both(DK, "test_cross_view_attention", f=f, L=L, heads=heads, D=D, coeff=coeff)],
    *_both(DK, "test_text_attention_and_rescale_branch"),
    *_both(DK, "test_elementwise_and_ddim"),
    *_both(DK, "test_linear_fp8", M=256, N=320, K=384),
    *_both(DK, "test_layernorm_fp8", M=64, C=320),
    *_both(DK, "test_conv3x3_fp8", B=2, H=16, W=16, Cin=128, Cout=128, stride=1),
    *_both(DK, "test_linear_fp8_qkv_transposed_v", B=1, L=100, C=640),
    *_both(DK, "test_groupnorm_apply_fp8", B=2, HW=256, C=320),
    *_both(TT, "test_tail_matches_torch_and_the_per_op_path", key="dtype", B=2, HW=256, f=1, Lt=77, gate_shift=0.0),
    *_both(TT, "test_tail_matches_torch_and_the_per_op_path", key="dtype", B=4, HW=128, f=2, Lt=50, gate_shift=0.0),
    *_both(TT, "test_head_matches_torch_and_the_per_op_path", key="dtype", B=2, HW=256),
    *_both("test_conv_cursor_gpu", "test_head_smallest_launch"),
    # the fused head / tail against the float64 mirror: text attention one key into the second 32-key block, the CFG-shared prefix, the head
    *[c for n in ("T3-ordinary-Lt33", "chain-halves2-B3-Lt33", "H4-HW128") for c in _both("test_ttail_pin_gpu", "test_case", key="dtype", name=n)],
    _c("test_plugin_gpu", "test_mask_composite_with_real_mask", H=96, W=130, C=3),
]


def _fmt(v):
    return str(v).replace("torch.", "") if not isinstance(v, tuple) else "x".join(str(x) for x in v)


def case_id(case):
    module, name, kw = case
    return "-".join([f"{module[5:]}.{name[5:]}"] + [_fmt(v) for v in kw.values()])


def product_modules():
    from gaussctrl_amd import gsplat_ops, mcmc, refine, scene_rows, train_ops, xview_attn
    from gaussctrl_amd.sd import ops
    return [gsplat_ops, train_ops, refine, mcmc, scene_rows, ops, xview_attn]


def helper_modules_of(mod):
    """the test module and every module of this directory whose functions it uses (its helpers: test_raster_gpu._t, ...), as far as they
    have a module global `torch`"""
    seen, todo = {}, [mod]
    while todo:
        m = todo.pop()
        if m.__name__ in seen or os.path.dirname(os.path.abspath(getattr(m, "__file__", None) or "/")) != _TESTS:
            continue
        seen[m.__name__] = m
        for v in vars(m).values():
            owner = v if isinstance(v, types.ModuleType) else sys.modules.get(getattr(v, "__module__", None) or "") if callable(v) else None
            if owner is not None:
                todo.append(owner)
    return [m for m in seen.values() if m.__dict__.get("torch") is torch and m.__name__ not in ("_redzone", __name__)]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_guarded(case, request):
    module, name, kw = case
    mod = importlib.import_module(module)
    fn = getattr(mod, name)
    kw = dict(kw)
    for p in inspect.signature(fn).parameters:
        if p not in kw:
            kw[p] = request.getfixturevalue(p)              # oracle_c, monkeypatch: passed through
    with guard(*product_modules(), *helper_modules_of(mod)):
        fn(**kw)
    _ran.add(case_id(case))


_ran = set()
# entry points of _lib.SYMBOLS that no guarded case above reaches: the next gap.  A new entry point joins either a case or this list.
NOT_REACHED = ["gc_abi_version", "gc_last_error_string",                       # (no device buffers)
               "gc_dn_attention_selection", "gc_dn_gemm_selection", "gc_dn_gemm_row_stat_slots", "gc_dn_transformer_tail_layout",      # (host-side queries)
               "gc_dn_depth_to_disparity", "gc_dn_group_stats", "gc_dn_groupnorm_apply", "gc_dn_groupnorm_apply_parts_fp8",
               "gc_raster_pad_intersects", "gc_raster_scan_tiles_views"]


# entry points that only the guards of another test module reach (its own arena sizes): when that module is not part of the run (this file
# run alone or next to a few others) they count as reached; in a run of the whole suite the list above holds as it stands
ELSEWHERE = {"test_edit_trace_gpu": ["gc_adam_step_rows", "gc_trace_mask_views", "gc_trace_select"]}


def test_entry_points_no_guarded_case_reaches():
    """which entry points the guarded cases of this process looked up, against the list above (only when every case ran and passed here)"""
    import _redzone
    from gaussctrl_amd import _lib
    if len(_ran) < len(CASES):
        return
    elsewhere = {s for module, names in ELSEWHERE.items() if module not in sys.modules for s in names}
    missing = sorted(set(_lib.SYMBOLS) - _redzone.reached - elsewhere)
    print("not reached:", missing)
    assert missing == sorted(NOT_REACHED), (sorted(set(missing) - set(NOT_REACHED)), sorted(set(NOT_REACHED) - set(missing)))


def test_guard_sees_a_device_store_past_the_end():
    """the check itself on the device (tests/test_redzone_cpu.py has the rest): a store of one float past a 299-float buffer, made with a
    torch view inside the arena (no kernel of the library misbehaves, nothing leaves memory the test owns), fails the guard; without it the
    same body passes"""
    victim = types.ModuleType("redzone_victim")
    victim.torch = torch
    exec("def make(n):\n    return torch.empty(n, dtype=torch.float32, device='cuda:0')\n", victim.__dict__)
    for past in (0, 1):
        try:
            with guard(victim, nbytes=8 << 20) as g:
                x = victim.make(299)
                assert g.arena.contains(x.data_ptr()) and bool(torch.isnan(x).all())
                torch.as_strided(x, (299 + past,), (1,))[298 + past] = 0.0
            failed = None
        except AssertionError as e:
            failed = str(e)
        assert victim.torch is torch
        if past:
            assert failed and "(299,) torch.float32: 4 bytes from offset 0" in failed, failed
        else:
            assert failed is None, failed

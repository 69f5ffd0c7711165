"""CPU: the edit-region tracing part of the C ABI (include/gaussctrl_trace.h) and its host layer, as far as they go without a GPU: the
header's three names and their export, the argument checks of each entry point (GC_EINVAL before anything is launched: the dummy host
buffers are never touched), the edit_region switch of GaussCtrlPipelineConfig and the combinations "traced" refuses, follow_cull on CPU
tensors, and the private-memory metadata of the three new kernels."""
import ctypes
import os
import re
import types

import pytest
import torch

from _abi_header import names as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gc_adam_step_rows", "gc_trace_mask_views", "gc_trace_select"]
EINVAL = -1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")):
        ge.build()
    return os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")


def test_header_declares_the_three_entry_points(built):
    from gaussctrl_amd import _lib
    assert _declared("gaussctrl_trace.h") == NAMES
    assert len(_declared("gaussctrl_hip.h")) == 83
    lib = ctypes.CDLL(built)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.SYMBOLS, n
    assert len(_lib.SYMBOLS) == len(set(_lib.SYMBOLS)) == 98


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()                      # host memory: a check that let one of these calls through would not go unnoticed
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    i32, i64, f32 = L.i32, L.i64, L.f32

    def trace(C=1, N=4, M=8, H=16, W=16, tx=1, ty=1, masks=p, w_in=p, w_all=p):
        return lib.gc_trace_mask_views(i32(C), i64(N), i64(M), i32(1), i32(H), i32(W), i32(tx), i32(ty), p, p, p, p, p, masks, w_in, w_all, null)

    assert trace(C=0) == EINVAL and trace(C=65536) == EINVAL and trace(N=-1) == EINVAL and trace(M=-1) == EINVAL
    assert trace(tx=2) == EINVAL and trace(ty=0) == EINVAL and trace(H=0) == EINVAL and trace(H=17) == EINVAL
    assert b"tile bounds" in lib.gc_last_error_string()
    assert trace(masks=null) == EINVAL and trace(w_in=null) == EINVAL and trace(w_all=null) == EINVAL
    assert b"gc_trace_mask_views" in lib.gc_last_error_string()
    assert trace(N=0, masks=null, w_in=null, w_all=null) == 0          # an empty scene: nothing to add, nothing launched

    def select(N=4, w_in=p, w_all=p, thr=0.5, mw=0.0, sel=p, count=p):
        return lib.gc_trace_select(i64(N), w_in, w_all, f32(thr), f32(mw), sel, count, null)

    assert select(N=-1) == EINVAL and select(count=null) == EINVAL
    assert select(w_in=null) == EINVAL and select(w_all=null) == EINVAL and select(sel=null) == EINVAL
    assert select(thr=float("nan")) == EINVAL and select(mw=float("nan")) == EINVAL
    assert b"gc_trace_select" in lib.gc_last_error_string()

    def adam(param=p, grad=p, m=p, v=p, rows=4, rf=3, sel=p, step=1):
        return lib.gc_adam_step_rows(param, grad, m, v, i64(rows), i32(rf), sel, f32(1e-3), f32(0.9), f32(0.999), f32(1e-15), i32(step), null)

    assert adam(param=null) == EINVAL and adam(grad=null) == EINVAL and adam(m=null) == EINVAL and adam(v=null) == EINVAL
    assert adam(sel=null) == EINVAL and adam(rows=-1) == EINVAL and adam(rf=0) == EINVAL and adam(step=0) == EINVAL
    assert adam(rows=1 << 26, rf=45) == EINVAL and adam(rows=1 << 31, rf=1) == EINVAL            # 2^31 elements and more
    assert b"gc_adam_step_rows" in lib.gc_last_error_string()
    assert adam(rows=0) == 0
    assert all(v == 0.0 for v in buf)


def test_config_switch_and_refusals():
    from gaussctrl_amd import edit_region as er
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipeline, GaussCtrlPipelineConfig
    from gaussctrl_amd.ns_compat import HAVE_NERFSTUDIO
    cfg = GaussCtrlPipelineConfig()
    assert cfg.edit_region == "image" and cfg.trace_ratio_thresh == 0.5 and cfg.trace_min_weight == 0.0
    assert GaussCtrlPipelineConfig(edit_region="traced").edit_region == "traced"
    with pytest.raises(ValueError, match="edit_region"):
        GaussCtrlPipelineConfig(edit_region="gaussians")
    # the refusals, on the rule itself ...
    ok = dict(config=GaussCtrlPipelineConfig(edit_region="traced", langsam_obj="bear"), model=types.SimpleNamespace(config=GaussCtrlModelConfig()),
              world_size=1, have_masks=True, have_nerfstudio=False)
    er.refuse_unsupported(**ok)
    for change, word in ((dict(have_masks=False), "masks"), (dict(have_nerfstudio=True), "nerfstudio"), (dict(world_size=2), "one GPU"),
                         (dict(model=types.SimpleNamespace(config=GaussCtrlModelConfig(refine_on_device=True))), "refine_on_device"),
                         (dict(model=types.SimpleNamespace(config=GaussCtrlModelConfig(densify_strategy="mcmc"))), "mcmc"),
                         (dict(config=GaussCtrlPipelineConfig(edit_region="traced", langsam_obj="bear", train_mode="sharded")), "sharded")):
        with pytest.raises(ValueError, match=word):
            er.refuse_unsupported(**dict(ok, **change))
    # ... and where the pipeline applies it: in its constructor, before any weight is made or loaded (no datamanager is ever asked)
    model = types.SimpleNamespace(config=GaussCtrlModelConfig())
    mask_fn = lambda rgb, obj: rgb[..., 0] > 0.5
    cases = [(GaussCtrlPipelineConfig(edit_region="traced"), dict(mask_fn=mask_fn), model),                                   # no langsam_obj
             (GaussCtrlPipelineConfig(edit_region="traced", langsam_obj="bear"), dict(), model)]                             # no mask_fn
    if not HAVE_NERFSTUDIO:
        good = lambda **kw: GaussCtrlPipelineConfig(edit_region="traced", langsam_obj="bear", **kw)
        cases += [(good(), dict(mask_fn=mask_fn), types.SimpleNamespace(config=GaussCtrlModelConfig(refine_on_device=True))),
                  (good(), dict(mask_fn=mask_fn), types.SimpleNamespace(config=GaussCtrlModelConfig(densify_strategy="mcmc"))),
                  (good(), dict(mask_fn=mask_fn, world_size=2), model),
                  (good(train_mode="sharded"), dict(mask_fn=mask_fn), model)]
    for cfg, kw, mdl in cases:
        with pytest.raises(ValueError, match="edit_region 'traced'"):
            GaussCtrlPipeline(cfg, "cpu", datamanager=object(), model=mdl, **kw)
    # a value assigned after construction is checked where it is read
    pipe = object.__new__(GaussCtrlPipeline)
    pipe.__dict__.update(config=types.SimpleNamespace(edit_region="Traced"), _model=model, world_size=1, mask_fn=mask_fn)
    with pytest.raises(ValueError, match="edit_region"):
        pipe._edit_region_traced()
    pipe.__dict__["config"] = types.SimpleNamespace(edit_region="image")
    assert pipe._edit_region_traced() is False
    pipe.apply_edit_select({})                                         # "image": the optimizers are not touched


def test_follow_cull_on_cpu_tensors():
    from gaussctrl_amd import edit_region as er
    sel = torch.tensor([1, 0, 0, 1, 1, 0, 1], dtype=torch.uint8)
    keep = torch.tensor([True, True, False, False, True, True, True])
    out = er.follow_cull(sel, keep)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.tolist() == [1, 0, 1, 0, 1]
    assert er.follow_cull(sel, torch.ones(7, dtype=torch.bool)).tolist() == sel.tolist()
    assert er.follow_cull(sel, torch.zeros(7, dtype=torch.bool)).shape == (0,)
    assert er.follow_cull(sel, keep.to(torch.uint8)).tolist() == [1, 0, 1, 0, 1]      # a 0 / 1 byte mask is a mask, not an index list
    with pytest.raises(ValueError):
        er.follow_cull(sel, keep[:-1])


def test_cull_callback_prunes_the_selection_with_the_rows():
    """gc_trainer.CullCallback on a six-tensor stub model on the CPU: model.edit_select loses the rows the parameters lose"""
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.gc_trainer import CullCallback
    from gaussctrl_amd.scene_rows import NAMES as LEAVES
    N = 6
    m = torch.nn.Module()
    shapes = {"means": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N, 1), "features_dc": (N, 3), "features_rest": (N, 15, 3)}
    g = torch.Generator().manual_seed(0)
    for n in LEAVES:
        setattr(m, n, torch.nn.Parameter(torch.randn(shapes[n], generator=g)))
    with torch.no_grad():
        m.scales[:] = -3.0                                                                # small scales: only the opacity rule culls
        m.opacities[:] = torch.tensor([3.0, -9.0, 3.0, 3.0, -9.0, 3.0])[:, None]
    m.config = GaussCtrlModelConfig()
    m.get_param_groups = lambda: {"xyz": [m.means], "features_dc": [m.features_dc], "features_rest": [m.features_rest],
                                  "opacity": [m.opacities], "scaling": [m.scales], "rotation": [m.quats]}
    m.edit_select = torch.tensor([1, 1, 0, 0, 0, 1], dtype=torch.uint8)
    CullCallback(m, {}).run(m.config.stop_split_at + m.config.refine_every - m.config.stop_split_at % m.config.refine_every)
    assert m.means.shape[0] == 4 and m.edit_select.tolist() == [1, 0, 0, 1]


def test_new_kernels_use_no_private_memory(built):
    from test_kernel_resources import kernel_resources
    res = kernel_resources(built)
    for name in ("k_trace_mask", "k_trace_select", "k_adam_rows"):
        hit = {k: v for k, v in res.items() if re.search(rf"\b{name}\(", k)}
        assert len(hit) == 1, (name, sorted(hit))
        assert list(hit.values()) == [(0, 0)], hit

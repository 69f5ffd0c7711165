"""CPU: the float64 absgrad reference (tests/_absgrad_ref.py) is sound -- its signed sum is the oracle's autograd xys gradient, its absolute
sum dominates it and is zero on culled Gaussians -- and the absgrad entry point is declared (include/gaussctrl_absgrad.h), listed, exported
and bound with matching argument counts; the config field and the RenderAux switch exist and default to off."""
import numpy as np
import pytest

import _abi_header as A
from _absgrad_ref import absgrad_reference
from test_raster_depth_gpu import BG, _cotangents, _oracle_scene, _scene

NEW = "gc_rasterize_bwd_abs_views"


@pytest.mark.parametrize("name", ["a", "b"])
def test_reference_signed_sum_is_the_oracle_gradient(name):
    """sum_p dL_p/dX = dL/dX: the per-pixel decomposition loses nothing (1e-12 relative, float64 against float64), |sum| <= sum of |.|
    elementwise, and a Gaussian the view culls (radius 0) is in no tile list, so both sums are exactly 0 there"""
    P, c2w, K = _scene(name)
    r = absgrad_reference(P, c2w, K, BG, _cotangents(K["H"], K["W"], 7))
    want = _oracle_scene(name)["full"]["xys"]
    assert np.abs(want).max() > 0
    assert np.abs(r["signed"] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(r["abs"] >= np.abs(r["signed"]))
    # ... and without the depth term of every L_p: the oracle's gradient of the two-term loss
    want2 = _oracle_scene(name)["nodepth"]["xys"]
    assert np.abs(r["signed_nodepth"] - want2).max() <= 1e-12 * np.abs(want2).max()
    assert np.all(r["abs_nodepth"] >= np.abs(r["signed_nodepth"])) and np.abs(r["abs_nodepth"] - r["abs"]).max() > 0
    culled = r["radii"] == 0
    assert np.all(r["abs"][culled] == 0.0)
    if name == "a":
        assert culled.any() and (~culled).any()
        # the reason the feature exists: most of the per-pixel gradient cancels in the signed sum
        vis = np.linalg.norm(r["signed"], axis=1) > 0
        assert np.median(np.linalg.norm(r["abs"][vis], axis=1) / np.linalg.norm(r["signed"][vis], axis=1)) > 2.0


def test_absgrad_symbol_declared_listed_and_exported():
    import ctypes
    from gaussctrl_amd import _lib
    assert A.names("gaussctrl_absgrad.h") == [NEW]
    assert NEW in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NEW)
    main = A.names("gaussctrl_hip.h")
    assert len(main) == 83 and NEW not in main               # the main header is as it was


def test_absgrad_bindings_pass_the_declared_number_of_arguments():
    """the prototype is gc_rasterize_bwd_depth_views' plus v_xy_abs before stream, and the call of gsplat_ops (_composite_bwd, which serves
    render_view and render_views) passes that many arguments"""
    (proto,) = A.prototypes("gaussctrl_absgrad.h")
    (base,) = [p for p in A.prototypes("gaussctrl_hip.h") if p.name == "gc_rasterize_bwd_depth_views"]
    assert proto.name == NEW and proto.ret == base.ret == "int"
    assert proto.params == base.params[:-1] + [("float *", "v_xy_abs"), ("void *", "stream")]
    n = len(proto.params)
    assert n == 31
    calls = A.sites("gaussctrl_amd/gsplat_ops.py", "gaussctrl_absgrad.h")
    assert calls == {NEW: [n]}, calls


def test_absgrad_switches_default_to_off():
    import dataclasses
    from gaussctrl_amd import gsplat_ops
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    f = {x.name: x for x in dataclasses.fields(GaussCtrlModelConfig)}
    assert f["use_absgrad"].type in (bool, "bool") and f["use_absgrad"].default is False
    assert "use_absgrad" in GaussCtrlModelConfig.__annotations__             # declared on this class: there with and without nerfstudio
    assert GaussCtrlModelConfig().use_absgrad is False and GaussCtrlModelConfig(use_absgrad=True).use_absgrad is True
    assert gsplat_ops.RenderAux.absgrad is False and gsplat_ops.RenderAux().absgrad is False
    assert gsplat_ops.RenderAux().xys_absgrad is None
    assert isinstance(GaussCtrlModel.xys_absgrad, property)


def test_refine_accumulate_refuses_a_missing_absgrad_buffer():
    """config.use_absgrad with a backward that left xys_grad but no xys_absgrad: an error, never the signed gradient in its place"""
    import types
    import torch
    from gaussctrl_amd import gsplat_ops, refine
    from gaussctrl_amd._lib import GaussCtrlHipError
    aux = gsplat_ops.RenderAux()
    aux.xys_grad = torch.zeros(4, 2)
    model = types.SimpleNamespace(config=types.SimpleNamespace(use_absgrad=True), _aux=aux, radii=torch.zeros(4, dtype=torch.int32), last_size=(8, 8))
    with pytest.raises(GaussCtrlHipError, match="xys_absgrad"):
        refine.RefineState().accumulate(model)

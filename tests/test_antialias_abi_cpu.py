"""CPU: the antialiased rasterize_mode's entry points are declared (include/gaussctrl_antialias.h), listed, exported and bound with matching
argument counts; the config field, the RenderAux switch and the render command's flag exist with the classic default."""
import pytest

import _abi_header as A

NEW = ("gc_project_sh_fwd_aa_views", "gc_project_sh_bwd_aa_views")


def test_antialias_symbols_declared_listed_and_exported():
    import ctypes
    from gaussctrl_amd import _lib
    assert set(A.names("gaussctrl_antialias.h")) == set(NEW)
    for name in NEW:
        assert name in _lib.SYMBOLS, name
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    main = set(A.names("gaussctrl_hip.h"))
    assert len(main) == 83 and not main & set(NEW)          # the main header is as it was


def test_antialias_bindings_pass_the_declared_number_of_arguments():
    """every call("gc_project_sh_*_aa_views", ...) of gsplat_ops passes, with the stream call() appends, as many arguments as the header's
    prototype has parameters; the binding table has that arity too (_abi_header.sites)"""
    declared = A.arities("gaussctrl_antialias.h")
    assert declared == {"gc_project_sh_fwd_aa_views": 27, "gc_project_sh_bwd_aa_views": 28}
    calls = A.sites("gaussctrl_amd/gsplat_ops.py", "gaussctrl_antialias.h")
    sites = {"gc_project_sh_fwd_aa_views": 2, "gc_project_sh_bwd_aa_views": 1}      # the forwards of render_view and render_views; _project_bwd
    for name in NEW:
        assert len(calls[name]) == sites[name] and all(n == declared[name] for n in calls[name]), (name, calls[name])


def test_rasterize_mode_config_field():
    import dataclasses
    from gaussctrl_amd import gsplat_ops
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    f = {x.name: x for x in dataclasses.fields(GaussCtrlModelConfig)}
    assert f["rasterize_mode"].type in (str, "str") and f["rasterize_mode"].default == "classic"
    assert "rasterize_mode" in GaussCtrlModelConfig.__annotations__          # declared on this class: there with and without nerfstudio
    assert GaussCtrlModelConfig().rasterize_mode == "classic"
    assert GaussCtrlModelConfig(rasterize_mode="antialiased").rasterize_mode == "antialiased"
    with pytest.raises(ValueError, match="rasterize_mode"):
        GaussCtrlModelConfig(rasterize_mode="mip")
    assert gsplat_ops.RenderAux.antialiased is False and gsplat_ops.RenderAux().antialiased is False
    assert gsplat_ops.RenderAux().compensation is None


def test_render_command_takes_the_mode():
    import inspect
    from gaussctrl_amd import gc_render
    base = ["dataset", "--load-gaussians", "scene.npz", "--cameras", "cams.json", "--output-path", "out"]
    ap = gc_render.make_parser()
    assert ap.parse_args(base).rasterize_mode == "classic"
    assert ap.parse_args(base + ["--rasterize-mode", "antialiased"]).rasterize_mode == "antialiased"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--rasterize-mode", "mip"])
    assert inspect.signature(gc_render.load_model).parameters["rasterize_mode"].default == "classic"

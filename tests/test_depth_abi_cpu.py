"""CPU: the depth-supervision entry points are declared and loaded, and the config switches exist with their defaults."""
import _abi_header as A

NEW = ("gc_rasterize_bwd_depth_views", "gc_project_sh_bwd_depth_views", "gc_depth_l1_views_workspace_bytes", "gc_depth_l1_fwd_bwd_views")


def test_depth_symbols_declared_and_listed():
    from gaussctrl_amd import _lib
    declared = set(A.names("gaussctrl_hip.h"))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
    assert len(declared) == 83


def test_depth_config_fields_and_defaults():
    import dataclasses
    from gaussctrl_amd import gsplat_ops, train_ops
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipelineConfig
    m = {f.name: f for f in dataclasses.fields(GaussCtrlModelConfig)}
    assert m["output_depth_during_training"].type in (bool, "bool") and GaussCtrlModelConfig().output_depth_during_training is False
    p = {f.name: f for f in dataclasses.fields(GaussCtrlPipelineConfig)}
    assert p["depth_loss_mult"].type in (float, "float") and GaussCtrlPipelineConfig().depth_loss_mult == 0.0
    assert gsplat_ops.RenderAux.depth_grad is False and gsplat_ops.RenderAux().depth_grad is False
    assert callable(train_ops.depth_l1_loss) and callable(train_ops.depth_l1_loss_views)

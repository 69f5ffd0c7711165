"""CPU: the bilateral-grid extension set of the C ABI (include/gaussctrl_bilagrid.h) and its host layer, as far as they go without a GPU:
the header's four gcx_ names, their export and the loader's EXT_SYMBOLS beside an unchanged SYMBOLS; the argument checks of each entry
point (GC_EINVAL before anything is launched: the dummy host buffers are never touched) and the empty call; the private-memory metadata of
the new kernels; the config fields, their validation and the refusals; and that nothing changes with the switch off."""
import ctypes
import os
import re
import types

import pytest
import torch

from _abi_header import names as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gcx_bilagrid_slice_bwd_views", "gcx_bilagrid_slice_fwd_views", "gcx_bilagrid_tv_fwd_bwd", "gcx_bilagrid_tv_workspace_bytes"]
EINVAL = -1
LEAVES = ["features_dc", "features_rest", "means", "opacities", "quats", "scales"]
GROUPS = ["features_dc", "features_rest", "opacity", "rotation", "scaling", "xyz"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")):
        ge.build()
    return os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")


def test_header_declares_the_four_extension_entry_points(built):
    from gaussctrl_amd import _lib
    assert _declared("gaussctrl_bilagrid.h", "gcx") == NAMES
    assert _declared("gaussctrl_bilagrid.h", "gc") == []                  # nothing the counted set's regex would pick up ...
    assert not re.search(r"\bgc_[a-z0-9_]+\s*\(", open(os.path.join(ROOT, "include", "gaussctrl_bilagrid.h")).read())     # ... comments included
    assert sorted(_lib.EXT_SYMBOLS) == NAMES and not set(_lib.EXT_SYMBOLS) & set(_lib.SYMBOLS)
    assert len(_lib.SYMBOLS) == len(set(_lib.SYMBOLS)) == 98
    assert len(_declared("gaussctrl_hip.h", "gc")) == 83
    lib = ctypes.CDLL(built)
    for n in NAMES:
        assert hasattr(lib, n), n
    l = _lib.lib()
    assert l.gcx_bilagrid_tv_workspace_bytes.restype is ctypes.c_size_t and l.gcx_bilagrid_tv_fwd_bwd.restype is ctypes.c_int
    assert l.gcx_bilagrid_slice_fwd_views.restype is ctypes.c_int and l.gcx_bilagrid_slice_bwd_views.restype is ctypes.c_int


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()                      # host memory: a check that let one of these calls through would not go unnoticed
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    i32, f32 = L.i32, L.f32
    ids = (ctypes.c_int32 * 2)(1, 0)

    def fwd(C=2, H=4, W=4, V=2, GW=4, GH=4, Lz=4, grids=p, rgb=p, idx=ids, out=p):
        return lib.gcx_bilagrid_slice_fwd_views(i32(C), i32(H), i32(W), i32(V), i32(GW), i32(GH), i32(Lz), grids, rgb, idx, out, null)

    def bwd(C=2, H=4, W=4, V=2, GW=4, GH=4, Lz=4, grids=p, rgb=p, idx=ids, v_out=p, v_grids=p, v_rgb=p):
        return lib.gcx_bilagrid_slice_bwd_views(i32(C), i32(H), i32(W), i32(V), i32(GW), i32(GH), i32(Lz), grids, rgb, idx, v_out, v_grids, v_rgb, null)

    for call, name in ((fwd, b"gcx_bilagrid_slice_fwd_views"), (bwd, b"gcx_bilagrid_slice_bwd_views")):
        assert call(C=0) == EINVAL and call(C=-1) == EINVAL and call(H=0) == EINVAL and call(W=0) == EINVAL and call(V=0) == EINVAL
        assert call(GW=1) == EINVAL and call(GH=1) == EINVAL and call(Lz=1) == EINVAL
        assert b"grid dimension" in lib.gc_last_error_string()
        assert call(idx=(ctypes.c_int32 * 2)(0, 2)) == EINVAL and call(idx=(ctypes.c_int32 * 2)(-1, 0)) == EINVAL and call(V=1) == EINVAL
        assert b"view_idx" in lib.gc_last_error_string() and name in lib.gc_last_error_string()
        assert call(C=1, H=32768, W=32768) == EINVAL                      # 3 * 2^30 image elements
        assert call(GW=1024, GH=1024, Lz=1024) == EINVAL                  # 12 * 2^30 grid elements
        assert b"2^31" in lib.gc_last_error_string()
        assert call(C=1, H=16 * 65535 + 1, W=1, idx=(ctypes.c_int32 * 1)(0)) == EINVAL         # more tile rows than a launch has
        assert b"65535" in lib.gc_last_error_string()
        assert call(grids=null) == EINVAL and call(rgb=null) == EINVAL and call(idx=null) == EINVAL
    assert fwd(out=null) == EINVAL
    assert bwd(v_out=null) == EINVAL and bwd(v_grids=null) == EINVAL and bwd(v_rgb=null) == EINVAL

    def tv(V=2, GW=4, GH=4, Lz=4, grids=p, weight=1.0, out=p, v_grids=p, ws=p, nbytes=1 << 20):
        return lib.gcx_bilagrid_tv_fwd_bwd(i32(V), i32(GW), i32(GH), i32(Lz), grids, f32(weight), out, v_grids, ws, ctypes.c_size_t(nbytes), null)

    need = lib.gcx_bilagrid_tv_workspace_bytes(i32(2), i32(4), i32(4), i32(4))
    assert need >= 8 * -(-2 * 12 * 4 * 4 * 4 // 256) and need % 8 == 0
    assert lib.gcx_bilagrid_tv_workspace_bytes(i32(40), i32(16), i32(16), i32(8)) >= 8 * (40 * 12 * 8 * 16 * 16 // 256)
    assert tv(V=-1) == EINVAL and tv(GW=1) == EINVAL and tv(GH=1) == EINVAL and tv(Lz=1) == EINVAL
    assert tv(GW=1024, GH=1024, Lz=1024) == EINVAL
    assert tv(grids=null) == EINVAL and tv(out=null) == EINVAL and tv(v_grids=null) == EINVAL and tv(ws=null) == EINVAL
    assert tv(nbytes=need - 1) == EINVAL and tv(nbytes=0) == EINVAL
    assert tv(weight=float("nan")) == EINVAL
    assert b"gcx_bilagrid_tv_fwd_bwd" in lib.gc_last_error_string()
    # the empty call: no grid, nothing to sum, nothing launched, no pointer looked at
    assert tv(V=0) == 0 and tv(V=0, grids=null, out=null, v_grids=null, ws=null, nbytes=0) == 0
    assert all(v == 0.0 for v in buf)


def test_new_kernels_use_no_private_memory(built):
    from test_kernel_resources import kernel_resources
    res = kernel_resources(built)
    hit = {k: v for k, v in res.items() if re.search(r"\bk_bilagrid_", k)}
    for name in (r"k_bilagrid_slice_fwd<true>", r"k_bilagrid_slice_fwd<false>", r"k_bilagrid_slice_bwd<0>", r"k_bilagrid_slice_bwd<1>",
                 r"k_bilagrid_slice_bwd<2>", r"k_bilagrid_tv\(", r"k_bilagrid_tv_sum\("):
        assert sum(bool(re.search(rf"\b{name}", k)) for k in hit) == 1, (name, sorted(hit))
    assert len(hit) == 7, sorted(hit)
    assert all(v == (0, 0) for v in hit.values()), hit
    # the counted families of tests/test_kernel_resources.py do not pick them up
    assert not any(re.search(r"\bk_(refine|mcmc)_|\bk_rasterize_|\bk_gemm8|\bk_thead<|\bk_ttail<|\bk_attn5<", k) for k in hit)


def test_config_defaults_and_validation():
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    c = GaussCtrlModelConfig()
    assert c.use_bilateral_grid is False and tuple(c.bilateral_grid_shape) == (16, 16, 8) and c.bilagrid_tv_mult == 10.0 and c.bilagrid_lr == 2e-3
    c = GaussCtrlModelConfig(use_bilateral_grid=True, bilateral_grid_shape=(7, 5, 4), bilagrid_tv_mult=0.0, bilagrid_lr=1e-2)
    assert c.use_bilateral_grid is True and tuple(c.bilateral_grid_shape) == (7, 5, 4)
    for bad in ((16, 16), (16, 16, 1), (16, 0, 8), (16.0, 16, 8), "16x16x8", None, (16, 16, 8, 2)):
        with pytest.raises(ValueError, match="bilateral_grid_shape"):
            GaussCtrlModelConfig(bilateral_grid_shape=bad)
    for bad in (-1.0, float("nan"), float("inf"), "10"):
        with pytest.raises(ValueError, match="bilagrid_tv_mult"):
            GaussCtrlModelConfig(bilagrid_tv_mult=bad)
    for bad in (0.0, -1e-3, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="bilagrid_lr"):
            GaussCtrlModelConfig(bilagrid_lr=bad)
    with pytest.raises(ValueError, match="use_bilateral_grid"):
        GaussCtrlModelConfig(use_bilateral_grid="yes")


def _params(n=5):
    from gaussctrl_amd import synthetic as syn
    return syn.make_gaussians(n, seed=0)


def test_switch_off_changes_nothing():
    from gaussctrl_amd.gc_config import optimizer_table
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.ns_compat import HAVE_NERFSTUDIO
    if HAVE_NERFSTUDIO:
        pytest.skip("the stand-alone model")
    m = GaussCtrlModel(GaussCtrlModelConfig(), params=_params(), device="cpu", num_train_data=3)      # num_train_data alone adds nothing
    assert sorted(m.get_param_groups()) == GROUPS and sorted(m.state_dict()) == LEAVES
    assert sorted(n for n, _ in m.named_parameters()) == LEAVES and not hasattr(m, "bilateral_grid")
    assert "bilateral_grid" not in optimizer_table()                                # the reference's table stays the reference's


def test_switch_on_owns_the_grids_and_their_group():
    from gaussctrl_amd.bilagrid import IDENTITY
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.ns_compat import HAVE_NERFSTUDIO
    if HAVE_NERFSTUDIO:
        pytest.skip("the stand-alone model")
    cfg = GaussCtrlModelConfig(use_bilateral_grid=True, bilateral_grid_shape=(7, 5, 4))
    m = GaussCtrlModel(cfg, params=_params(), device="cpu", num_train_data=3)
    assert isinstance(m.bilateral_grid, torch.nn.Parameter) and m.bilateral_grid.shape == (3, 12, 4, 5, 7)
    assert torch.equal(m.bilateral_grid[2, :, 1, 4, 6], torch.tensor(IDENTITY)) and torch.equal(m.bilateral_grid[0, :, 0, 0, 0], torch.tensor(IDENTITY))
    assert sorted(m.state_dict()) == sorted(LEAVES + ["bilateral_grid"])
    groups = m.get_param_groups()
    assert sorted(groups) == sorted(GROUPS + ["bilateral_grid"]) and groups["bilateral_grid"][0] is m.bilateral_grid
    # refusals: num_train_data missing or not positive
    for kw in ({}, {"num_train_data": 0}, {"num_train_data": -2}, {"num_train_data": None}, {"num_train_data": 2.0}):
        with pytest.raises(ValueError, match="num_train_data"):
            GaussCtrlModel(cfg, params=_params(), device="cpu", **kw)
    # an image_idx outside [0, V), refused before any kernel is asked
    out = {"rgb": torch.zeros(8, 8, 3)}
    for idx in (3, -1):
        with pytest.raises(ValueError, match="image_idx"):
            m.get_loss_dict(out, {"image": torch.zeros(8, 8, 3), "image_idx": idx})


def test_refuses_more_than_one_gpu_and_mismatched_views():
    from gaussctrl_amd import bilagrid
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipeline, GaussCtrlPipelineConfig
    on, off = GaussCtrlModelConfig(use_bilateral_grid=True), GaussCtrlModelConfig()
    bilagrid.refuse_unsupported(on, 1)
    bilagrid.refuse_unsupported(off, 8)
    for mode in ("parity", "throughput", "sharded"):
        me = types.SimpleNamespace(world_size=2, model=types.SimpleNamespace(config=on), config=types.SimpleNamespace(train_mode=mode))
        with pytest.raises(ValueError, match="use_bilateral_grid"):
            GaussCtrlPipeline.train_forward_backward(me, 0)
    # ... and in the pipeline's constructor, before any weight is made or loaded (no datamanager is ever asked)
    with pytest.raises(ValueError, match="use_bilateral_grid"):
        GaussCtrlPipeline(GaussCtrlPipelineConfig(), "cpu", world_size=2, datamanager=object(), model=types.SimpleNamespace(config=on))
    model = types.SimpleNamespace(config=on, bilateral_grid=torch.zeros(3, 12, 8, 16, 16))
    with pytest.raises(ValueError, match="3 grids"):
        GaussCtrlPipeline(GaussCtrlPipelineConfig(), "cpu", datamanager=types.SimpleNamespace(train_data=[{}] * 4), model=model)


def test_host_layer_on_cpu_tensors():
    from gaussctrl_amd import bilagrid
    from gaussctrl_amd._lib import GaussCtrlHipError
    g = bilagrid.identity_grids(2, 4, 3, 2, "cpu")
    assert g.shape == (2, 12, 2, 3, 4) and g.is_contiguous() and g.dtype == torch.float32
    assert torch.equal(g[:, :, 1, 2, 3], torch.tensor(bilagrid.IDENTITY).expand(2, 12))
    assert bilagrid.identity_grids(0, 4, 3, 2, "cpu").shape == (0, 12, 2, 3, 4)
    with pytest.raises(ValueError):
        bilagrid.identity_grids(2, 1, 3, 2, "cpu")
    with pytest.raises(GaussCtrlHipError):
        bilagrid.bilagrid_apply(g, torch.zeros(1, 4, 4, 3), [0])
    with pytest.raises(GaussCtrlHipError):
        bilagrid.bilagrid_tv_loss(g)
    with pytest.raises(ValueError, match="outside"):
        bilagrid.bilagrid_apply(g, torch.zeros(1, 4, 4, 3), [2])
    assert bilagrid.check_view(torch.tensor(1), 2) == 1


def _switched_on(n=50, V=4):
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    return GaussCtrlModel(GaussCtrlModelConfig(use_bilateral_grid=True, bilagrid_lr=5e-3), params=_params(n), device="cpu", num_train_data=V)


def test_trainer_schedules_every_group_of_a_switched_on_model():
    """the stand-alone trainer assigns a learning rate to every optimizer before it steps: the grid's group is outside the reference's
    table and gets config.bilagrid_lr at every step, the six leaf groups get what they got"""
    from gaussctrl_amd.gc_config import build_optimizers, optimizer_table, scheduled_lr
    from gaussctrl_amd.gc_trainer import GaussCtrlTrainer
    from gaussctrl_amd.ns_compat import HAVE_NERFSTUDIO
    if HAVE_NERFSTUDIO:
        pytest.skip("the stand-alone trainer")
    m = _switched_on()
    opts = build_optimizers(m)
    assert set(opts) == set(GROUPS) | {"bilateral_grid"}
    for table in (None, optimizer_table()):
        me = types.SimpleNamespace(config=types.SimpleNamespace(optimizers=table), pipeline=types.SimpleNamespace(model=m))
        for step in (30000, 30499):
            for g, opt in opts.items():
                for pg in opt.param_groups:
                    pg["lr"] = GaussCtrlTrainer.lr_at(me, g, step)
            assert opts["bilateral_grid"].param_groups[0]["lr"] == 5e-3 and opts["bilateral_grid"].param_groups[0]["eps"] == 1e-15
            assert all(opts[g].param_groups[0]["lr"] == scheduled_lr(g, step) for g in GROUPS)


def test_cull_leaves_the_grids_and_their_moments_alone():
    """gc_trainer.CullCallback prunes the six per-Gaussian tensors with the row mask; the grids (no rows) and their Adam state keep
    their bits"""
    from gaussctrl_amd.gc_trainer import CullCallback
    from gaussctrl_amd.ns_compat import HAVE_NERFSTUDIO
    if HAVE_NERFSTUDIO:
        pytest.skip("the stand-alone callbacks")
    m = _switched_on(50, 4)
    with torch.no_grad():
        m.scales[:] = -3.0
        m.opacities[:] = 3.0
        m.opacities[[3, 11, 12, 40, 49]] = -9.0
        m.bilateral_grid.add_(torch.randn(m.bilateral_grid.shape, generator=torch.Generator().manual_seed(0)) * 0.1)
    grid = m.bilateral_grid
    state = {"step": 7, "exp_avg": torch.randn(grid.shape), "exp_avg_sq": torch.rand(grid.shape)}
    opts = {"bilateral_grid": types.SimpleNamespace(state={grid: dict(state)}),
            "opacity": types.SimpleNamespace(state={m.opacities: {"step": 7, "exp_avg": torch.randn(50, 1), "exp_avg_sq": torch.rand(50, 1)}})}
    before = grid.detach().clone()
    CullCallback(m, opts).run(30000)
    assert m.means.shape[0] == 45 and m.opacities.shape == (45, 1) and opts["opacity"].state[m.opacities]["exp_avg"].shape == (45, 1)
    assert m.bilateral_grid is grid and torch.equal(grid.detach(), before) and grid.shape == (4, 12, 8, 16, 16)
    st = opts["bilateral_grid"].state[grid]
    assert st["step"] == 7 and torch.equal(st["exp_avg"], state["exp_avg"]) and torch.equal(st["exp_avg_sq"], state["exp_avg_sq"])

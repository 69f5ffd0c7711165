"""CPU: the MCMC densification entry points are declared (include/gaussctrl_mcmc.h), exported and bound with matching argument counts; the
config fields exist with their defaults and densify_strategy is validated; mcmc.schedule against hand cases; the stand-alone model's callbacks
and loss keys under both strategies; "mcmc" refuses world_size > 1."""
import types

import pytest

import _abi_header as A

NEW = ("gc_mcmc_dead_workspace_bytes", "gc_mcmc_dead", "gc_mcmc_relocate", "gc_mcmc_inject_noise")


def test_mcmc_symbols_declared_listed_and_exported():
    import ctypes
    from gaussctrl_amd import _lib
    assert set(A.names("gaussctrl_mcmc.h")) == set(NEW)
    for name in NEW:
        assert name in _lib.SYMBOLS, name
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


def test_mcmc_bindings_pass_the_declared_number_of_arguments():
    """every call("gc_mcmc_*", ...) of the host layer passes, with the stream call() appends, as many arguments as the header's prototype has
    parameters; the binding table has that arity too (_abi_header.sites)"""
    declared = A.arities("gaussctrl_mcmc.h")
    assert declared == {"gc_mcmc_dead_workspace_bytes": 1, "gc_mcmc_dead": 9, "gc_mcmc_relocate": 11, "gc_mcmc_inject_noise": 8}
    sites = A.sites("gaussctrl_amd/mcmc.py", "gaussctrl_mcmc.h")
    for name, passed in sites.items():
        assert all(n == declared[name] for n in passed), (name, passed)
    assert set(sites) == set(NEW)


def test_mcmc_workspace_size_and_refusals_without_a_device():
    """the argument checks come before any launch or pointer use: they can be exercised without a GPU"""
    import ctypes as C
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    assert lib.gc_mcmc_dead_workspace_bytes(L.i64(0)) >= 4
    assert lib.gc_mcmc_dead_workspace_bytes(L.i64(257)) == 8 and lib.gc_mcmc_dead_workspace_bytes(L.i64(70001)) == 4 * 274
    one = C.c_void_p(64)
    six = (C.c_void_p * 6)(*[64] * 6)
    # N = 0 / n = 0: success, nothing launched
    assert lib.gc_mcmc_dead(L.i64(0), None, L.f32(0.005), None, None, None, None, C.c_size_t(0), None) == 0
    assert lib.gc_mcmc_relocate(L.i64(0), L.i64(5), L.i32(45), None, None, L.f32(0.005), None, None, None, None, None) == 0
    assert lib.gc_mcmc_relocate(L.i64(100), L.i64(0), L.i32(45), None, None, L.f32(0.005), None, None, None, None, None) == 0
    assert lib.gc_mcmc_inject_noise(L.i64(0), None, None, None, None, None, L.f32(1.0), None) == 0
    # 2^31 elements or more, a wrong features_rest width, a min_opacity outside [0, 1): GC_EINVAL
    big = (1 << 31) // 45 + 1
    assert lib.gc_mcmc_relocate(L.i64(big), L.i64(1), L.i32(45), one, one, L.f32(0.005), one, six, None, None, None) == -1
    assert b"2^31" in lib.gc_last_error_string()
    assert lib.gc_mcmc_relocate(L.i64(big - 10), L.i64(20), L.i32(0), one, None, L.f32(0.005), one, six, None, None, None) == -1     # N + n rows
    assert lib.gc_mcmc_dead(L.i64(1 << 31), one, L.f32(0.005), one, one, one, one, C.c_size_t(1 << 40), None) == -1
    assert lib.gc_mcmc_inject_noise(L.i64(1 << 29), one, one, one, one, one, L.f32(1.0), None) == -1
    assert lib.gc_mcmc_relocate(L.i64(10), L.i64(1), L.i32(7), one, one, L.f32(0.005), one, six, None, None, None) == -1
    assert b"features_rest" in lib.gc_last_error_string()
    assert lib.gc_mcmc_dead(L.i64(10), one, L.f32(-0.1), one, one, one, one, C.c_size_t(64), None) == -1
    assert lib.gc_mcmc_dead(L.i64(1000), one, L.f32(0.005), one, one, one, one, C.c_size_t(4), None) != 0                         # workspace too small


def test_mcmc_config_fields_and_validation():
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    c = GaussCtrlModelConfig()
    want = dict(densify_strategy="default", mcmc_cap_max=1_000_000, mcmc_noise_lr=5e5, mcmc_min_opacity=0.005, mcmc_refine_start_iter=500,
                mcmc_refine_stop_iter=25_000, mcmc_refine_every=100, mcmc_opacity_reg=0.01, mcmc_scale_reg=0.01)
    assert {k: getattr(c, k) for k in want} == want
    assert all(type(getattr(c, k)) is type(v) for k, v in want.items())
    assert GaussCtrlModelConfig(densify_strategy="mcmc").densify_strategy == "mcmc"
    for bad in ("MCMC", "", "absgrad", None):
        with pytest.raises(ValueError):
            GaussCtrlModelConfig(densify_strategy=bad)
    assert c.refine_on_device is False and c.rasterize_mode == "classic" and c.use_absgrad is False          # the other switches keep their defaults


def test_mcmc_schedule_hand_cases():
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.mcmc import schedule
    c = GaussCtrlModelConfig()
    assert [schedule(c, s) for s in (500, 600, 650, 25000, 24900)] == [False, True, False, False, True]
    assert not schedule(c, 0) and not schedule(c, 30000) and schedule(c, 1000)
    # a shrunk schedule, as the GPU callback test uses it
    c2 = types.SimpleNamespace(mcmc_refine_start_iter=4, mcmc_refine_stop_iter=30, mcmc_refine_every=5)
    assert [s for s in range(40) if schedule(c2, s)] == [5, 10, 15, 20, 25]


def _cpu_model(**cfg):
    import torch
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    g = torch.Generator().manual_seed(0)
    P = {"means": torch.randn(7, 3, generator=g), "scales": torch.randn(7, 3, generator=g) - 3, "quats": torch.randn(7, 4, generator=g),
         "opacities": torch.randn(7, 1, generator=g), "features_dc": torch.randn(7, 3, generator=g), "features_rest": torch.zeros(7, 15, 3)}
    return GaussCtrlModel(GaussCtrlModelConfig(**cfg), params=P, device="cpu")


def test_mcmc_callbacks_of_the_stand_alone_model():
    from gaussctrl_amd.gc_trainer import CullCallback, McmcCallback, RefineCallback, StepCallback
    attrs = types.SimpleNamespace(optimizers={"xyz": None}, grad_scaler=None, pipeline=None)
    kinds = lambda **cfg: [type(c) for c in _cpu_model(**cfg).get_training_callbacks(attrs)]
    assert kinds(densify_strategy="mcmc") == [StepCallback, McmcCallback]
    assert kinds(densify_strategy="mcmc", refine_on_device=True) == [StepCallback, McmcCallback]
    assert kinds() == [StepCallback, CullCallback]
    assert kinds(refine_on_device=True) == [StepCallback, RefineCallback]
    cb = _cpu_model(densify_strategy="mcmc").get_training_callbacks(attrs)[1]
    assert (cb.n_relocated, cb.n_added) == (0, 0) and cb.optimizers is attrs.optimizers and cb.where == ("after_train_iteration",)


def test_mcmc_loss_keys_and_values(monkeypatch):
    """the key logic alone: the image loss is replaced by a constant, the two regularisers are plain torch and run on the CPU"""
    import torch
    from gaussctrl_amd import train_ops
    monkeypatch.setattr(train_ops, "l1_ssim_loss", lambda rgb, gt, lam: torch.tensor(0.25))
    batch, out = {"image": torch.zeros(2, 2, 3)}, {"rgb": torch.zeros(2, 2, 3)}
    m = _cpu_model()
    assert list(m.get_loss_dict(out, batch)) == ["main_loss"]
    m = _cpu_model(densify_strategy="mcmc", mcmc_opacity_reg=0.5, mcmc_scale_reg=2.0)
    loss = m.get_loss_dict(out, batch)
    assert list(loss) == ["main_loss", "opacity_reg", "scale_reg"] and float(loss["main_loss"]) == 0.25
    assert torch.allclose(loss["opacity_reg"], 0.5 * torch.sigmoid(m.opacities).mean()) and loss["opacity_reg"].requires_grad
    assert torch.allclose(loss["scale_reg"], 2.0 * torch.exp(m.scales).mean()) and loss["scale_reg"].requires_grad


def test_mcmc_refuses_more_than_one_gpu():
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipeline
    me = types.SimpleNamespace(world_size=2, model=types.SimpleNamespace(config=GaussCtrlModelConfig(densify_strategy="mcmc")),
                               config=types.SimpleNamespace(train_mode="parity"))
    with pytest.raises(ValueError, match="mcmc"):
        GaussCtrlPipeline.train_forward_backward(me, 0)


def test_mcmc_host_layer_refuses_cpu_tensors():
    from gaussctrl_amd import mcmc
    from gaussctrl_amd._lib import GaussCtrlHipError
    m = _cpu_model(densify_strategy="mcmc")
    for call in (lambda: mcmc.relocate(m, {}), lambda: mcmc.add_new(m, {}), lambda: mcmc.inject_noise(m, 1e-4)):
        with pytest.raises(GaussCtrlHipError):
            call()

"""CPU: camera pose refinement as far as it goes without a GPU -- the bars of tests/_pose_ref.py against the reference's own float32 error,
the compose function (zero row, SO(3) exponential on both sides of the small-angle switch, Jacobian), the config fields and their
validation, the refusals, the parameter, its group and state_dict round trip, the regulariser and the metrics."""
import types

import numpy as np
import pytest
import torch

import _inside_scene as S
import _pose_ref as R
from _margins import within


def test_bars_are_four_times_the_reference_distance():
    """BARS = 4 x the worst float32-vs-float64 distance of pose_ref itself (bar / 8 <= measured <= bar / 3, the convention of
    test_project_vjp_cpu.py); row 2 of v_P is exactly 0 in every case (asserted inside)"""
    dist = R.reference_distances()
    for k, bar in R.BARS.items():
        print(f"{k}: float32 reference distance {dist[k]:.3e}, bar {bar:.3e}")
        assert bar / 8 <= dist[k] <= bar / 3, (k, dist[k], bar)


def test_blocks_that_no_cotangent_reaches_are_exactly_zero_in_the_reference():
    for name in ("in3", "tiny"):
        for aa in (False, True):
            assert not R.pose_ref(name, 0, aa, "b", False)["v_P"].any()          # conics do not read P
            assert not R.pose_ref(name, 0, aa, "d", True)["v_P"].any()           # nor does the depth
            assert not R.pose_ref(name, 0, aa, "c", False)["v_V"].any()          # the pixel centre does not read V
            assert R.pose_ref(name, 0, aa, "b", False)["v_V"].any() and R.pose_ref(name, 0, aa, "c", False)["v_P"].any()


def test_sensitivity_of_the_conic_only_cases():
    """What the bar would catch.  Dropping the T = J W term from v_V moves all 12 conic-only cases (the 12 views of the four scenes) by
    0.56 .. 1.03 of |v_V|; a straight-through frustum clamp moves all 12 by 0.028 .. 0.19 -- both four orders of magnitude beyond the bar.
    The restated covariance that isolates the T term agrees with the oracle's conics to 2e-15."""
    n_t = n_st = total = 0
    for name in S.SCENES:
        for v in range(len(S.scene(name)[1])):
            ref = R.pose_ref(name, v, False, "b", False)
            term, restated = R.conic_T_term(name, v)
            assert restated < 1e-12
            dropped = ref["v_V"].copy()
            dropped[:, :3] -= term
            n_t += R.block_error(dropped, ref["v_V"]) > 0.5
            n_st += R.block_error(R.pose_ref(name, v, False, "b", False, straight_through=True)["v_V"], ref["v_V"]) > 0.02
            total += 1
    assert (n_t, n_st, total) == (12, 12, 12)


# ---------------------------------------------------------------------------------------- compose
def _c2w(seed=3):
    from gaussctrl_amd import synthetic as syn
    return syn.make_cameras(1, seed=seed)[0]


def test_zero_row_gives_the_unadjusted_cam_dict_bit_for_bit():
    from gaussctrl_amd import camera_opt
    from gaussctrl_amd.camera import camera_to_gsplat
    for seed in (1, 2, 3):
        c2w = _c2w(seed)
        adj = camera_opt.adjusted_c2w(c2w, torch.zeros(6))
        assert adj.dtype == np.float32 and adj.tobytes() == np.asarray(c2w, np.float32)[:3].tobytes()
        a, b = camera_to_gsplat(adj, 80.0, 79.2, 49.3, 29.9, 96, 64), camera_to_gsplat(c2w, 80.0, 79.2, 49.3, 29.9, 96, 64)
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].tobytes() == b[k].tobytes(), k
            else:
                assert a[k] == b[k], k
    moved = camera_opt.adjusted_c2w(_c2w(), torch.tensor([0.01, 0.0, 0.0, 0.0, 0.02, 0.0]))
    assert not np.array_equal(moved, np.asarray(_c2w(), np.float32)[:3])


def _skew(w):
    z = torch.zeros((), dtype=torch.float64)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1e-4, 0.0099, 0.0101, 0.02, 0.5, 3.0])
def test_so3_exp_matches_matrix_exp_on_both_sides_of_the_switch(angle):
    """the switch sits at |omega|^2 = 1e-4, i.e. an angle of 0.01: 0.0099 takes the series, 0.0101 Rodrigues' formula.  Held to
    torch.matrix_exp at 1e-12 -- except at 0.02, where matrix_exp's own low-degree Taylor form is 2.1e-12 away from the truth (measured
    against the 12-term series of the two Rodrigues coefficients; so3_exp is 1.1e-16 from it) -- and to that series at 1e-15 up to 0.5 rad."""
    import math
    from gaussctrl_amd import camera_opt
    d = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
    w = d / d.norm() * angle
    assert (float((w * w).sum()) < camera_opt.SMALL_ANGLE2) == (angle < 0.01)
    E = camera_opt.so3_exp(w)
    if angle != 0.02:
        err = float((E - torch.matrix_exp(_skew(w))).abs().max())
        within(f"so3_exp at angle {angle}: max abs error against matrix_exp", err, 1e-12)
    t2, K = float((w * w).sum()), _skew(w)
    A = sum((-1) ** k * t2 ** k / math.factorial(2 * k + 1) for k in range(12))
    B = sum((-1) ** k * t2 ** k / math.factorial(2 * k + 2) for k in range(12))
    truth = torch.eye(3, dtype=torch.float64) + A * K + B * (K @ K)
    if angle <= 0.5:            # (at 3 rad the alternating series itself cancels to 4e-14)
        within(f"so3_exp at angle {angle}: max abs error against the long series", float((E - truth).abs().max()), 1e-15)
    assert float((E @ E.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
    if angle == 0.0:
        assert torch.equal(E, torch.eye(3, dtype=torch.float64))


def _plain_viewmat(c2w, row):
    """the plain formula: c2w @ [matrix_exp(skew(omega)) | tau], then the glue's flip and inverse"""
    c = torch.tensor(np.asarray(c2w, np.float64)[:3])
    R_, t = c[:, :3] @ torch.matrix_exp(_skew(row[3:])), c[:, :3] @ row[:3] + c[:, 3]
    Rg = R_ @ torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64))
    return torch.cat([Rg.T, -(Rg.T @ t)[:, None]], 1)


@pytest.mark.parametrize("scale", [0.0, 1e-3, 0.3])
def test_jacobian_matches_autograd_of_the_plain_formula(scale):
    from gaussctrl_amd import camera_opt
    c2w = _c2w(5)
    row = torch.tensor([0.4, -0.2, 0.7, 0.5, 0.1, -0.6], dtype=torch.float64) * scale
    J = camera_opt.jacobian(c2w, row)
    assert J.shape == (3, 4, 6) and J.dtype == torch.float64
    ref = torch.autograd.functional.jacobian(lambda x: _plain_viewmat(c2w, x), row)
    within(f"compose Jacobian at scale {scale}: max abs error against autograd of the plain formula", float((J - ref).abs().max()), 1e-10)
    # and the composed pose is the product's own glue of it
    from gaussctrl_amd.camera import camera_to_gsplat
    vm = camera_opt.viewmat_of(camera_opt.compose(c2w, row)).numpy()
    glue = np.asarray(camera_to_gsplat(camera_opt.adjusted_c2w(c2w, row), 1.0, 1.0, 0.0, 0.0, 2, 2)["viewmat4"], np.float64)[:3]
    assert np.abs(vm - glue).max() < 1e-6
    # right-multiplication: the translation moves along the camera's own axes
    moved = camera_opt.compose(c2w, torch.tensor([0.1, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)).numpy()
    assert np.allclose(moved[:, 3] - np.asarray(c2w, np.float64)[:3, 3], 0.1 * np.asarray(c2w, np.float64)[:3, 0], atol=1e-12)


def test_link_chains_viewmat_grad_to_the_row():
    """the autograd link on CPU tensors: with aux.viewmat_grad = G the row receives sum(G * J); the means' gradient passes unchanged"""
    from gaussctrl_amd import camera_opt
    c2w = _c2w(7)
    row = torch.tensor([0.01, -0.02, 0.005, 0.02, 0.01, -0.015], requires_grad=True)
    means = torch.randn(5, 3, generator=torch.Generator().manual_seed(0), requires_grad=True)
    aux = types.SimpleNamespace(viewmat_grad=None)
    out = camera_opt.link(means, row, aux, c2w)
    assert torch.equal(out, means)
    G = torch.randn(1, 3, 4, generator=torch.Generator().manual_seed(1))
    aux.viewmat_grad = G                       # what the render's backward leaves before the link's backward runs
    (out * 2.0).sum().backward()
    assert torch.equal(means.grad, torch.full((5, 3), 2.0))
    want = torch.einsum("rc,rcj->j", G[0].double(), camera_opt.jacobian(c2w, row.detach()))
    assert row.grad.dtype == torch.float32 and float((row.grad.double() - want).abs().max()) < 1e-6 * float(want.abs().max())
    # float64 autograd of a linear functional of the view matrix gives the same thing
    r64 = row.detach().double().requires_grad_(True)
    (camera_opt.viewmat_of(camera_opt.compose(c2w, r64)) * G[0].double()).sum().backward()
    assert float((r64.grad - want).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------- config, parameter, refusals
GROUPS = ["features_dc", "features_rest", "opacity", "rotation", "scaling", "xyz"]
LEAVES = ["features_dc", "features_rest", "means", "opacities", "quats", "scales"]


def _params(n=5):
    from gaussctrl_amd import synthetic as syn
    return syn.make_gaussians(n, seed=0)


def test_config_defaults_and_validation():
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    c = GaussCtrlModelConfig()
    assert c.camera_optimizer_mode == "off" and c.camera_opt_lr is None
    assert c.camera_opt_trans_l2_penalty == 1e-2 and c.camera_opt_rot_l2_penalty == 1e-3
    c = GaussCtrlModelConfig(camera_optimizer_mode="SO3xR3", camera_opt_lr=1e-3, camera_opt_trans_l2_penalty=0.0, camera_opt_rot_l2_penalty=0)
    assert c.camera_optimizer_mode == "SO3xR3"
    for bad in ("SO3", "so3xr3", "on", None, True, 1):
        with pytest.raises(ValueError, match="camera_optimizer_mode"):
            GaussCtrlModelConfig(camera_optimizer_mode=bad)
    for bad in (0.0, -1e-3, float("nan"), float("inf"), "1e-3", True):
        with pytest.raises(ValueError, match="camera_opt_lr"):
            GaussCtrlModelConfig(camera_opt_lr=bad)
    for name in ("camera_opt_trans_l2_penalty", "camera_opt_rot_l2_penalty"):
        for bad in (-1.0, float("nan"), float("inf"), "1", None):
            with pytest.raises(ValueError, match=name):
                GaussCtrlModelConfig(**{name: bad})


def _standalone():
    from gaussctrl_amd.ns_compat import HAVE_NERFSTUDIO
    if HAVE_NERFSTUDIO:
        pytest.skip("the stand-alone model")


def test_switch_off_changes_nothing():
    _standalone()
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    m = GaussCtrlModel(GaussCtrlModelConfig(), params=_params(), device="cpu", num_train_data=3)
    assert sorted(m.get_param_groups()) == GROUPS and sorted(m.state_dict()) == LEAVES and not hasattr(m, "pose_adjustment")
    m.train()
    out = {"rgb": torch.zeros(8, 8, 3)}
    assert "camera_opt_translation" not in m.get_metrics_dict(out, {"image": torch.zeros(8, 8, 3)})


def _switched_on(V=4, **kw):
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    return GaussCtrlModel(GaussCtrlModelConfig(camera_optimizer_mode="SO3xR3", **kw), params=_params(), device="cpu", num_train_data=V)


def test_switch_on_owns_the_rows_their_group_and_state():
    _standalone()
    from gaussctrl_amd.gc_config import build_optimizers, optimizer_table, scheduled_lr
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.gc_trainer import GaussCtrlTrainer
    m = _switched_on()
    assert isinstance(m.pose_adjustment, torch.nn.Parameter) and m.pose_adjustment.shape == (4, 6) and m.pose_adjustment.dtype == torch.float32
    assert not m.pose_adjustment.detach().any()
    groups = m.get_param_groups()
    assert sorted(groups) == sorted(GROUPS + ["camera_opt"]) and groups["camera_opt"][0] is m.pose_adjustment
    assert sorted(m.state_dict()) == sorted(LEAVES + ["pose_adjustment"])
    # state_dict round trip
    with torch.no_grad():
        m.pose_adjustment.copy_(torch.arange(24.0).reshape(4, 6) * 1e-3)
    m2 = _switched_on()
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2.pose_adjustment, m.pose_adjustment)
    # num_train_data missing or not positive
    cfg = GaussCtrlModelConfig(camera_optimizer_mode="SO3xR3")
    for kw in ({}, {"num_train_data": 0}, {"num_train_data": None}, {"num_train_data": 2.0}, {"num_train_data": True}):
        with pytest.raises(ValueError, match="num_train_data"):
            GaussCtrlModel(cfg, params=_params(), device="cpu", **kw)
    # the optimizer: the table's schedule by default, config.camera_opt_lr (constant, eps 1e-15) when a number
    opts = build_optimizers(m)
    assert set(opts) == set(GROUPS) | {"camera_opt"}
    assert opts["camera_opt"].param_groups[0]["lr"] == scheduled_lr("camera_opt", 30000) and opts["camera_opt"].param_groups[0]["params"][0] is m.pose_adjustment
    m3 = _switched_on(camera_opt_lr=3e-3)
    opts3 = build_optimizers(m3)
    assert opts3["camera_opt"].param_groups[0]["lr"] == 3e-3 and opts3["camera_opt"].param_groups[0]["eps"] == 1e-15
    for model, want in ((m, scheduled_lr("camera_opt", 30250)), (m3, 3e-3)):
        me = types.SimpleNamespace(config=types.SimpleNamespace(optimizers=optimizer_table()), pipeline=types.SimpleNamespace(model=model))
        assert GaussCtrlTrainer.lr_at(me, "camera_opt", 30250) == want
        assert GaussCtrlTrainer.lr_at(me, "xyz", 30250) == scheduled_lr("xyz", 30250)


def test_view_index_is_checked():
    from gaussctrl_amd import camera_opt
    cam = lambda md: types.SimpleNamespace(metadata=md)
    assert camera_opt.check_view(cam({"cam_idx": 2}), 3) == 2 and camera_opt.check_view(cam({"cam_idx": torch.tensor(0)}), 3) == 0
    for md in (None, {}, {"cam_idx": None}, {"cam_idx": 3}, {"cam_idx": -1}):
        with pytest.raises(ValueError, match="cam_idx"):
            camera_opt.check_view(cam(md), 3)


def test_training_get_outputs_refuses_before_any_kernel():
    """a camera without (or with a wrong) cam_idx, a crop box and grad_into are refused in training mode before anything is launched (the
    model sits on the CPU: reaching a kernel would raise another error)"""
    _standalone()
    from gaussctrl_amd.ns_compat import Cameras
    m = _switched_on()
    m.train()
    c2w = torch.tensor(_c2w())
    for md in (None, {"cam_idx": 4}):
        with pytest.raises(ValueError, match="cam_idx"):
            m.get_outputs(Cameras(c2w, 40.0, 40.0, 16.0, 16.0, 32, 32, metadata=md))
    ok = Cameras(c2w, 40.0, 40.0, 16.0, 16.0, 32, 32, metadata={"cam_idx": 1})
    m.crop_box = object()
    with pytest.raises(ValueError, match="crop box"):
        m.get_outputs(ok)
    m.crop_box = None
    m.grad_into = {}
    with pytest.raises(ValueError, match="grad_into"):
        m.get_outputs(ok)


def test_refusals():
    from gaussctrl_amd import camera_opt
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipeline, GaussCtrlPipelineConfig
    on, off = GaussCtrlModelConfig(camera_optimizer_mode="SO3xR3"), GaussCtrlModelConfig()
    camera_opt.refuse_unsupported(on, 1, "single")
    camera_opt.refuse_unsupported(on, 1, "parity")
    camera_opt.refuse_unsupported(off, 8, "sharded", True, True)
    with pytest.raises(ValueError, match="nerfstudio"):
        camera_opt.refuse_unsupported(on, 1, "single", True)
    with pytest.raises(ValueError, match="one GPU"):
        camera_opt.refuse_unsupported(on, 2, "parity")
    for mode in ("throughput", "sharded"):
        with pytest.raises(ValueError, match="grad_into"):
            camera_opt.refuse_unsupported(on, 1, mode)
    with pytest.raises(ValueError, match="crop box"):
        camera_opt.refuse_unsupported(on, 1, "single", crop_in_training=True)
    from gaussctrl_amd.ns_compat import HAVE_NERFSTUDIO
    if HAVE_NERFSTUDIO:
        return
    for mode in ("parity", "throughput", "sharded"):
        me = types.SimpleNamespace(world_size=2, model=types.SimpleNamespace(config=on), config=types.SimpleNamespace(train_mode=mode))
        with pytest.raises(ValueError, match="camera_optimizer_mode"):
            GaussCtrlPipeline.train_forward_backward(me, 0)
    with pytest.raises(ValueError, match="camera_optimizer_mode"):
        GaussCtrlPipeline(GaussCtrlPipelineConfig(), "cpu", world_size=2, datamanager=object(), model=types.SimpleNamespace(config=on))
    model = types.SimpleNamespace(config=on, pose_adjustment=torch.zeros(3, 6))
    with pytest.raises(ValueError, match="3 pose rows"):
        GaussCtrlPipeline(GaussCtrlPipelineConfig(), "cpu", datamanager=types.SimpleNamespace(train_data=[{}] * 4), model=model)


def test_regulariser_and_metrics():
    _standalone()
    from gaussctrl_amd import camera_opt
    m = _switched_on(camera_opt_trans_l2_penalty=0.5, camera_opt_rot_l2_penalty=0.25)
    with torch.no_grad():
        m.pose_adjustment[0] = torch.tensor([3.0, 0.0, 4.0, 0.0, 0.0, 0.0])
        m.pose_adjustment[1] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.6, 0.8])
    reg = camera_opt.regularizer(m.pose_adjustment, 0.5, 0.25)
    assert float(reg.detach()) == pytest.approx(0.5 * 5.0 / 4 + 0.25 * 1.0 / 4, rel=1e-6)
    reg.backward()
    g = m.pose_adjustment.grad
    assert torch.isfinite(g).all() and not g[2:].any()                       # zero rows: a zero subgradient, not NaN
    assert torch.allclose(g[0], torch.tensor([0.6, 0.0, 0.8, 0.0, 0.0, 0.0]) * 0.5 / 4) and torch.allclose(g[1, 3:], torch.tensor([0.0, 0.6, 0.8]) * 0.25 / 4)
    out, batch = {"rgb": torch.zeros(8, 8, 3)}, {"image": torch.zeros(8, 8, 3)}
    met = m.get_metrics_dict(out, batch)
    assert float(met["camera_opt_translation"]) == pytest.approx(5.0 / 4) and float(met["camera_opt_rotation"]) == pytest.approx(1.0 / 4)
    # an all-zero parameter: value 0, gradient 0
    z = torch.zeros(3, 6, requires_grad=True)
    r = camera_opt.regularizer(z, 1.0, 1.0)
    r.backward()
    assert float(r) == 0.0 and not z.grad.any()

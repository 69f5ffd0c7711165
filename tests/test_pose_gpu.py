"""The camera gradient of the renderer on the GPU (include/gaussctrl_pose.h, RenderAux.pose_grad, camera_optimizer_mode "SO3xR3").

Entry point alone: gcx_pose_bwd_views on the scenes of tests/_inside_scene.py (camera inside the cloud) behind the product's own projection
forward, against float64 autograd of tests/_pose_ref.pose_ref per view and block at _pose_ref.BARS; bit-reproducible; N = 1, N = 0, every
Gaussian behind the camera; one run inside a red-zone arena.  Whole render: RenderAux.viewmat_grad of render_view / render_views against
float64 autograd of the oracle's whole render with the view matrix a leaf.  Recovery: four poses off by about 0.02 rad and 0.02 units are
pulled back by Adam on pose_adjustment alone, through the model's own training path.

Sensitivity of the entry-point bars (tests/test_pose_cpu.py::test_sensitivity_of_the_conic_only_cases asserts the counts on the float64
reference): dropping the T = J W term moves v_V of all 12 conic-only cases (12 views over the four scenes; 11 of them run here) by 0.56 ..
1.03 of its norm, a straight-through frustum clamp moves all 12 by 0.028 .. 0.19; the bar is 4.2e-6."""
import numpy as np
import pytest
import torch

import _inside_scene as S
import _pose_ref as R
from _margins import within
from _redzone import Arena
from test_project_vjp_gpu import _cams, _cot, _forward_views, _leaves, _t
from test_raster_gpu import _grad_close, _img_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F32 = dict(dtype=torch.float32, device=DEV)
_FWD = {}


def _front(name, aa):
    """(leaves, cams, forward state) of a scene: the product's projection forward, once per (scene, aa)"""
    if (name, aa) not in _FWD:
        tp, cams = _leaves(name), _cams(name)
        _FWD[(name, aa)] = (tp, cams, _forward_views(tp, cams, 3, 3, S.scene(name)[2], aa))
    return _FWD[(name, aa)]


def _pose(tp, cams, o, cot, aa, depth):
    """gcx_pose_bwd_views through ops.pose_bwd_views -> numpy [C, 2, 3, 4]"""
    from gaussctrl_amd import gsplat_ops as ops
    out = ops.pose_bwd_views(tp["means"], tp["scales"], tp["quats"], tp["opacities"], cams, o["radii"], o["conics"], cot["xys"], cot["conics"],
                             cot["opac"] if aa else None, cot["depths"] if depth else None, aa)
    return out.cpu().numpy()


@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
@pytest.mark.parametrize("name", ["in3", "tiny", "views9"])
def test_entry_point_vs_float64(name, aa):
    """every view and block under sets a (with and without v_depths), b, c, d against the float64 reference at BARS; exact zeros where the
    reference is exactly zero (v_P under conic-only and depth-only cotangents, v_V under xys-only ones, row 2 of v_P by layout); the same call
    twice gives the same bits.  tiny: N = 299 = one 256-lane round of the workgroup plus a 43-lane tail; views9: C = 9 crosses the
    8-views-per-launch split."""
    tp, cams, o = _front(name, aa)
    C, N = len(cams), tp["means"].shape[0]
    for v in range(C):                                     # the kept sets agree (a radius one off does not matter; a cull would)
        assert np.array_equal(o["radii"][v].cpu().numpy() > 0, R.pose_ref(name, v, aa, "b", False)["radii"] > 0), (name, v)
    for cset, depth in R.CASES:
        cot = _cot(name, cset, depth, C, N)
        got = _pose(tp, cams, o, cot, aa, cot["depths"] is not None)
        assert np.array_equal(got.view(np.int32), _pose(tp, cams, o, cot, aa, cot["depths"] is not None).view(np.int32)), "not bit-reproducible"
        vV, vP = R.split_out(got)
        for v in range(C):
            ref = R.pose_ref(name, v, aa, cset, depth)
            for k, g in (("v_V", vV[v]), ("v_P", vP[v])):
                e = R.block_error(g, ref[k])
                print(f"{name} aa={aa} set {cset} depth={depth} view {v} {k}: {e:.3e} (bar {R.BARS[k]:.1e})")
                within(f"{name} aa={aa} set {cset} depth={depth} view {v}: {k} relative Frobenius error", e, R.BARS[k])
        if cset in ("b", "d"):
            assert not got[:, 1].any()
        if cset == "c":
            assert not got[:, 0].any()


def test_zero_depth_cotangent_is_the_null_pointer():
    """v_depths = zeros gives the bits of v_depths = NULL"""
    tp, cams, o = _front("tiny", False)
    cot = _cot("tiny", "a", False, 1, 299)
    a = _pose(tp, cams, o, cot, False, False)
    cot["depths"] = torch.zeros(1, 299, **F32)
    assert np.array_equal(a.view(np.int32), _pose(tp, cams, o, cot, False, True).view(np.int32))


@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
def test_one_gaussian_none_and_all_behind(aa):
    from gaussctrl_amd import _lib as L, gsplat_ops as ops
    P, c2ws, K = S.scene("in3")
    cams = _cams("in3")
    keep = int(np.argmax(R.pose_ref("in3", 0, aa, "a", True)["radii"] > 0))          # a Gaussian the view keeps
    tp = {k: v[keep:keep + 1].contiguous() for k, v in _leaves("in3").items()}
    o = _forward_views(tp, cams, 3, 3, K, aa)
    assert int(o["radii"][0, 0]) > 0
    cot = {k: (None if v is None else v[:, keep:keep + 1].contiguous()) for k, v in _cot("in3", "a", True, 1, 3000).items()}
    got = _pose(tp, cams, o, cot, aa, True)
    # N = 1: the sum is the one Gaussian's own term -- the float64 reference of the one-row scene, restated through the full scene's cache
    # is not available per row, so hold it to the product's own N = 3000 run with every other cotangent zeroed
    tpf, _, of = _front("in3", aa)
    z = {k: (None if v is None else torch.zeros_like(v)) for k, v in _cot("in3", "a", True, 1, 3000).items()}
    for k in z:
        if z[k] is not None:
            z[k][:, keep] = _cot("in3", "a", True, 1, 3000)[k][:, keep]
    full = _pose(tpf, cams, of, z, aa, True)
    assert np.isfinite(got).all() and got.any() and np.array_equal(got.view(np.int32), full.view(np.int32))
    # N = 0: zeros, nothing else touched
    out = torch.full((2, 2, 3, 4), NAN, **F32)
    lib = L.lib()
    two = cams + cams
    L.check(lib.gcx_pose_bwd_views(L.i64(0), L.i32(2), L.i32(int(aa)), None, None, None, None, ops._cams_host(two), L.i32(K["H"]), L.i32(K["W"]), None,
                                   None, None, None, None, None, None, L.ptr(out), L.stream_ptr()), "gcx_pose_bwd_views")
    assert not out.cpu().numpy().any()
    # the camera turned about its own y axis by half a turn: every Gaussian it kept is now behind it; nothing contributes
    c2w = np.asarray(c2ws[0], np.float32).copy()
    c2w[:3, 0] *= -1; c2w[:3, 2] *= -1
    from gaussctrl_amd.camera import camera_to_gsplat
    back = [camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], K["W"], K["H"])]
    tpf = _leaves("in3")
    front_kept = of["radii"][0] > 0
    tpb = {k: v[front_kept].contiguous() for k, v in tpf.items()}
    ob = _forward_views(tpb, back, 3, 3, K, aa)
    assert int((ob["radii"] > 0).sum()) == 0 and int(front_kept.sum()) > 500
    n = int(front_kept.sum())
    cotb = {k: (None if v is None else v[:, :n].contiguous()) for k, v in _cot("in3", "a", True, 1, 3000).items()}
    gotb = _pose(tpb, back, ob, cotb, aa, True)
    assert not gotb.any()


def test_guarded_run_touches_nothing_outside_its_buffers():
    """every buffer of one call (views9, antialiased, with v_depths: two launches plus the sum) carved from a red-zone arena, the workspace
    exactly as large as the query says: the poisoned zones behind `out`, the workspace and every input come back untouched, and the result
    is the unguarded call's, bit for bit"""
    from gaussctrl_amd import _lib as L, gsplat_ops as ops
    tp, cams, o = _front("views9", True)
    C, N = 9, 3000
    K = S.scene("views9")[2]
    cot = _cot("views9", "a", True, C, N)
    want = _pose(tp, cams, o, cot, True, True)
    arena = Arena(16 << 20, DEV)

    def carve(t):
        b = arena.carve(t.shape, t.dtype)
        b.copy_(t)
        return b
    lib = L.lib()
    nbytes = int(lib.gcx_pose_bwd_views_workspace_bytes(L.i64(N), L.i32(C)))
    assert nbytes == C * 3 * 24 * 4
    ins = [carve(tp[k]) for k in ("means", "scales", "quats", "opacities")]
    per_view = [carve(t) for t in (o["radii"], o["conics"], cot["xys"], cot["conics"], cot["opac"], cot["depths"])]
    ws = arena.carve((nbytes,), torch.uint8)
    out = arena.carve((C, 2, 3, 4), torch.float32)
    assert arena.check() == []
    L.check(lib.gcx_pose_bwd_views(L.i64(N), L.i32(C), L.i32(1), *(L.ptr(t) for t in ins), ops._cams_host(cams), L.i32(K["H"]), L.i32(K["W"]),
                                   *(L.ptr(t) for t in per_view), L.ptr(ws), L.ptr(out), L.stream_ptr()), "gcx_pose_bwd_views")
    bad = arena.check()
    assert bad == [], bad
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------------------- whole render
WR = dict(N=2000, W=64, H=48, fx=60.0, seed=3, scale_mean=0.05)
BG = np.array([0.1, 0.2, 0.3], np.float32)


def _wr_scene():
    from gaussctrl_amd import synthetic as syn
    from gaussctrl_amd.camera import camera_to_gsplat
    if "wr" not in _FWD:
        P = syn.make_gaussians(WR["N"], seed=WR["seed"], scale_mean=WR["scale_mean"])
        c2ws = syn.make_cameras(3, seed=WR["seed"] + 1)
        K = dict(fx=WR["fx"], fy=WR["fx"] * 0.99, cx=WR["W"] / 2 + 1.3, cy=WR["H"] / 2 - 2.1, W=WR["W"], H=WR["H"])
        cams = [camera_to_gsplat(c, K["fx"], K["fy"], K["cx"], K["cy"], K["W"], K["H"]) for c in c2ws]
        v_rgb = np.random.default_rng(5).normal(size=(3, K["H"], K["W"], 3)).astype(np.float32)
        refs = []
        for c, cam, v in zip(c2ws, cams, v_rgb):             # float64 autograd of the oracle's whole render, the view matrix a leaf
            V = torch.tensor(np.asarray(cam["viewmat4"], np.float64)[:3]).requires_grad_(True)
            rgb, loss, p = R.whole_render_ref(P, V, np.asarray(c, np.float32)[:3, 3], K, BG, v_rgb=v)
            loss.backward()
            refs.append(dict(rgb=rgb.detach().numpy(), viewmat=V.grad.numpy(), leaves={k: t.grad.numpy() for k, t in p.items()}))
        _FWD["wr"] = (P, c2ws, K, cams, v_rgb, refs)
    return _FWD["wr"]


def _render(P, cams, v_rgb, pose_grad, batched):
    from gaussctrl_amd import gsplat_ops as ops
    tp = {k: _t(v).requires_grad_(True) for k, v in P.items()}
    aux = ops.RenderAux()
    aux.pose_grad = pose_grad
    args = [tp[k] for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")]
    if batched:
        rgb, _, _ = ops.render_views(*args, cams, _t(BG), False, 3, aux)
        (rgb * _t(v_rgb)).sum().backward()
    else:
        rgb, _, _ = ops.render_view(*args, cams[0], _t(BG), False, 3, aux)
        (rgb * _t(v_rgb[0])).sum().backward()
    proj = {k: getattr(aux, k).cpu().numpy() for k in ("xys", "radii")}
    return rgb.detach().cpu().numpy(), {k: t.grad.cpu().numpy() for k, t in tp.items()}, aux, proj


@pytest.mark.parametrize("batched", [False, True], ids=["render_view", "render_views"])
def test_whole_render_viewmat_grad(batched):
    """RenderAux.viewmat_grad within 1e-3 of its largest entry of the float64 oracle (the project's bar for gradients behind the float atomics
    of the compositing backward); with the flag on, image and leaf gradients stay within the existing bars of the run with it off, and the
    projection outputs keep their bits"""
    P, c2ws, K, cams, v_rgb, refs = _wr_scene()
    C = 3 if batched else 1
    rgb1, g1, aux1, proj1 = _render(P, cams, v_rgb, True, batched)
    rgb0, g0, aux0, proj0 = _render(P, cams, v_rgb, False, batched)
    assert aux0.viewmat_grad is None and aux1.viewmat_grad is not None
    vg = aux1.viewmat_grad
    assert vg.is_cuda and vg.dtype == torch.float32 and tuple(vg.shape) == (C, 3, 4)
    vg = vg.cpu().numpy().astype(np.float64)
    for v in range(C):
        ref = refs[v]["viewmat"]
        e = float(np.abs(vg[v] - ref).max() / np.abs(ref).max())
        print(f"view {v}: viewmat_grad max abs error / max entry {e:.3e}")
        within(f"whole render view {v}: viewmat_grad error / largest entry", e, 1e-3)
        _img_close((rgb1[v] if batched else rgb1), refs[v]["rgb"])
    # flag on against flag off: the same launches computed image and leaf gradients (compositing sums with float atomics: no bits demanded)
    _img_close(rgb1, rgb0)
    scale = max(np.abs(g).max() for g in g0.values())
    for k in g0:
        _grad_close(g1[k], g0[k], scale)
    for k in ("xys", "radii"):
        assert np.array_equal(proj1[k].view(np.int32), proj0[k].view(np.int32)), k
    assert np.array_equal(aux1.xys.cpu().numpy().view(np.int32), aux0.xys.cpu().numpy().view(np.int32))
    ref_sum = {k: sum(refs[v]["leaves"][k] for v in range(C)) for k in g1}
    for k in g1:
        _grad_close(g1[k], ref_sum[k], max(np.abs(g).max() for g in ref_sum.values()))


def test_conics_keep_their_bits_with_the_flag():
    """the projection state the backward saved (conics included) is bit-identical with pose_grad on and off"""
    from gaussctrl_amd import gsplat_ops as ops
    P, c2ws, K, cams, v_rgb, refs = _wr_scene()
    saved = []
    for flag in (False, True):
        tp = {k: _t(v).requires_grad_(True) for k, v in P.items()}
        aux = ops.RenderAux()
        aux.pose_grad = flag
        rgb, _, _ = ops.render_views(*[tp[k] for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")], cams, _t(BG), False, 3, aux)
        radii, conics, xys = rgb.grad_fn.saved_tensors[6:9]
        saved.append([t.cpu().numpy().view(np.int32) for t in (radii, conics, xys)])
    for a, b in zip(*saved):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------- recovery
def test_pose_recovery_through_the_training_path():
    """Targets: 4 views rendered from the true poses.  Start: every pose off by its seeded row (0.02 rad, 0.02 units).  The Gaussians are
    frozen; torch.optim.Adam steps pose_adjustment alone through GaussCtrlModel.get_outputs / get_loss_dict in training mode, one view per
    step in turn, 120 steps at 3e-3.  The float64 oracle's own run of this schedule (_pose_ref.oracle_recovery, measured on a CPU) ends at
    0.092 of the starting mean pose error (0.0400 -> 0.00368), well below the 0.25 it was sized for, and its loss at 0.064 of the start.
    Demanded of the device: mean pose error <= 0.5 of the start (the factor 2 is for a float32 Adam trajectory on atomically summed
    gradients) and the photometric loss, averaged over the last round of the views, below half of the first round's.  A sign or transpose
    error in the chain diverges and fails both."""
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.ns_compat import Cameras, HAVE_NERFSTUDIO
    if HAVE_NERFSTUDIO:
        pytest.skip("the stand-alone model")
    r = R.RECOVERY
    assert r["oracle_final_over_start"] <= 0.25
    P, c2ws, K, rows0 = R.recovery_scene()
    starts = R.start_poses(c2ws, rows0)
    cfg = GaussCtrlModelConfig(background_color="black", camera_optimizer_mode="SO3xR3", camera_opt_trans_l2_penalty=0.0, camera_opt_rot_l2_penalty=0.0)
    model = GaussCtrlModel(cfg, params=P, device=DEV, num_train_data=r["views"])
    cam = lambda c, i: Cameras(torch.tensor(np.asarray(c, np.float32)[:3]), K["fx"], K["fy"], K["cx"], K["cy"], K["W"], K["H"], metadata={"cam_idx": i})
    targets = [model.get_outputs_for_camera(cam(c, i))["rgb"].clone() for i, c in enumerate(c2ws)]
    before = {n: getattr(model, n).detach().clone() for n in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")}
    model.train()
    opt = torch.optim.Adam([model.pose_adjustment], lr=r["lr"], eps=1e-15)
    e0 = R.mean_pose_error(starts, model.pose_adjustment, c2ws)
    losses = []
    for step in range(r["steps"]):
        v = step % r["views"]
        model.zero_grad(set_to_none=True)
        out = model.get_outputs(cam(starts[v], v))
        loss_dict = model.get_loss_dict(out, {"image": targets[v], "image_idx": v})
        assert float(loss_dict["camera_opt_regularizer"].detach()) == 0.0
        loss = sum(loss_dict.values())
        loss.backward()
        g = model.pose_adjustment.grad
        assert g is not None and torch.isfinite(g).all() and bool(g[v].any()) and not bool(g[[i for i in range(r["views"]) if i != v]].any())
        opt.step()
        losses.append(float(loss))
    e1 = R.mean_pose_error(starts, model.pose_adjustment, c2ws)
    first, last = float(np.mean(losses[:r["views"]])), float(np.mean(losses[-r["views"]:]))
    print(f"mean pose error {e0:.5f} -> {e1:.5f} ({e1 / e0:.3f}); loss {first:.5f} -> {last:.5f} ({last / first:.3f})")
    assert abs(e0 - 0.04) < 1e-3
    within("pose recovery: final / initial mean pose error", e1 / e0, 0.5)
    within("pose recovery: final / initial photometric loss", last / first, 0.5, strict=True)
    for n, t in before.items():                              # frozen: nothing stepped the Gaussians
        assert torch.equal(getattr(model, n).detach(), t), n
    # evaluation never sees the adjustment: the true-pose render is still the target, bit for bit
    assert torch.equal(model.get_outputs_for_camera(cam(c2ws[0], 0))["rgb"], targets[0])

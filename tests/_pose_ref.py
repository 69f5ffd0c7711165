"""Float64 autograd references of the CAMERA gradient of the renderer (plain helper, like _inside_scene.py, whose scenes and cotangents it uses).

pose_ref is front_ref of _inside_scene.py restated with the two camera matrices as leaves: viewmat[:3] (V) and fullproj (P) of the oracle's
float32 camera glue -- the matrices the kernels are handed -- through oracle.raster_torch.project_gaussians (xys, depths, conics) and, with aa,
the per-view opacity sigmoid(logit) * rho of _inside_scene._rho.  The SH view directions are not differentiated: they pass no gradient to the
pose (include/gaussctrl_pose.h).  It returns, per view, raw v_V [3, 4], raw v_P [4, 4] and the chained [3, 4] gradient
v_V + (projmat4^T v_P)[:3] (fullproj = projmat4 @ viewmat4), in float32 or float64.

Metric: per view and block (v_V, v_P), |got - ref|_F / |ref|_F.  A block whose reference is exactly 0 must be exactly 0 on the other side
(v_P under conic-only or depth-only cotangents, v_V under xys-only cotangents, row 2 of v_P always).

BARS: 4 x the worst distance between the float32 and the float64 pose_ref over the four scenes of _inside_scene, every view, the cotangent
sets a - d with the depth cotangent (BAR_CASES), aa off and on (the device's operation order differs from torch's, hence the 4).  Measured
(tests/test_pose_cpu.py asserts bar / 8 <= measured <= bar / 3 for each):

    v_V 1.04e-6 (views9 view 1, aa, set a)      v_P 1.87e-6 (in7, sets a and c; 1.81e-6 on a second machine, whose BLAS sums in another order)

The GPU tests also run set a WITHOUT the depth cotangent (CASES), which the bars were not measured on: there v_V loses the depth term's share
of its norm and the float32 reference itself is 1.92e-6 away (tiny, aa) -- still inside the bar.

whole_render_ref is oracle.raster_torch.get_outputs (training form) restated from the oracle's own pieces with the view matrix as a leaf;
recovery_scene and oracle_recovery size the pose-recovery test of tests/test_pose_gpu.py."""
import numpy as np
import torch

import _inside_scene as S

BARS = {"v_V": 4.2e-6, "v_P": 7.2e-6}
# (cotangent set, with the depth cotangent): what the entry point is run under
CASES = (("a", False), ("a", True), ("b", False), ("c", False), ("d", True))
BAR_CASES = (("a", True), ("b", False), ("c", False), ("d", True))          # what BARS was measured over
_CACHE = {}


def _leaves(P, dtype):
    p = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in S.with_degree(P, 3).items()}
    scales = torch.exp(p["scales"])
    quats = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
    return p, scales, quats


def pose_ref(name, view, aa, cset, depth, dtype=torch.float64, straight_through=False):
    """{"v_V": [3, 4], "v_P": [4, 4], "chained": [3, 4]} (float64 numpy arrays, computed in dtype) of one view of a scene of _inside_scene
    under the cotangent set; cached"""
    key = ("pose", name, view, aa, cset, depth, dtype, straight_through)
    if key in _CACHE:
        return _CACHE[key]
    import contextlib
    from gaussctrl_amd.camera import camera_to_gsplat
    from oracle import raster_c, raster_torch as rt
    P, c2ws, K = S.scene(name)
    cot = {k: c[view] for k, c in S.cotangents(name, cset, depth).items()}
    p, scales, quats = _leaves(P, dtype)
    W, H = K["W"], K["H"]
    V4, F4 = raster_c.camera_glue(c2ws[view], K["fx"], K["fy"], W, H)
    V = torch.tensor(V4[:3], dtype=dtype).requires_grad_(True)
    F = torch.tensor(F4, dtype=dtype).requires_grad_(True)
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    with (S._straight_through_clamp(rt) if straight_through else contextlib.nullcontext()):
        xys, depths, radii, conics, _, _ = rt.project_gaussians(p["means"], scales, 1.0, quats, V, F, K["fx"], K["fy"], K["cx"], K["cy"], H, W, tb)
    o = dict(xys=xys, depths=depths, conics=conics)
    if aa:
        o["opac"] = torch.sigmoid(p["opacities"])[:, 0] * S._rho(rt, p["means"], scales, quats, V, K, radii)
    loss = sum((o[k] * torch.tensor(np.asarray(v), dtype=dtype)).sum() for k, v in cot.items() if k in o)
    gV, gF = torch.autograd.grad(loss, [V, F], allow_unused=True) if torch.is_tensor(loss) and loss.requires_grad else (None, None)
    gV = np.zeros((3, 4)) if gV is None else gV.numpy().astype(np.float64)
    gF = np.zeros((4, 4)) if gF is None else gF.numpy().astype(np.float64)
    proj = np.asarray(camera_to_gsplat(c2ws[view], K["fx"], K["fy"], K["cx"], K["cy"], W, H)["projmat4"], np.float64)
    _CACHE[key] = {"v_V": gV, "v_P": gF, "chained": gV + (proj.T @ gF)[:3], "radii": radii.numpy()}
    return _CACHE[key]


def split_out(out):
    """the entry point's out [C][2][3][4] (array) -> (v_V [C, 3, 4], v_P [C, 4, 4] with the zero row 2 put back), float64"""
    out = np.asarray(out, np.float64).reshape(-1, 2, 3, 4)
    vP = np.zeros((out.shape[0], 4, 4))
    vP[:, [0, 1, 3]] = out[:, 1]
    return out[:, 0].copy(), vP


def block_error(got, ref):
    """|got - ref|_F / |ref|_F; a reference that is exactly 0 demands exact zeros (returns 0.0)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    if not ref.any():
        assert not got.any(), "a block whose reference is exactly 0 is not exactly 0"
        return 0.0
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def reference_distances():
    """worst block_error of the float32 pose_ref against the float64 one, per block: what BARS is four times of"""
    if "dist" not in _CACHE:
        worst = {"v_V": 0.0, "v_P": 0.0}
        for name in S.SCENES:
            for view in range(len(S.scene(name)[1])):
                for aa in (False, True):
                    for cset, depth in BAR_CASES:
                        r32, r64 = (pose_ref(name, view, aa, cset, depth, dt) for dt in (torch.float32, torch.float64))
                        assert not r64["v_P"][2].any() and not r32["v_P"][2].any()
                        for k in worst:
                            worst[k] = max(worst[k], block_error(r32[k], r64[k]))
        _CACHE["dist"] = worst
    return _CACHE["dist"]


def conic_T_term(name, view, dtype=torch.float64):
    """The share of v_V, under the conic-only cotangents (set b), that arrives through T = J W alone: the 2 x 2 covariance of
    rt.project_gaussians restated (as _inside_scene._rho restates it) with the W of T a leaf of its own.  Returns (the [3, 3] term, the
    worst |restated conic - rt's conic| over the kept rows: the restatement's own check)."""
    from oracle import raster_c, raster_torch as rt
    P, c2ws, K = S.scene(name)
    p, scales, quats = _leaves(P, dtype)
    W, H = K["W"], K["H"]
    V4, F4 = raster_c.camera_glue(c2ws[view], K["fx"], K["fy"], W, H)
    V = torch.tensor(V4[:3], dtype=dtype)
    WT = V[:, :3].clone().requires_grad_(True)
    t = p["means"] @ V[:, :3].T + V[:, 3]
    keep = t[:, 2] > 0.01
    tz = torch.where(keep, t[:, 2], torch.ones_like(t[:, 2]))
    M = rt.quat_to_rotmat(quats) * scales[:, None, :]
    Sigma = M @ M.transpose(1, 2)
    txc = tz * torch.clamp(t[:, 0] / tz, -1.3 * (0.5 * W / K["fx"]), 1.3 * (0.5 * W / K["fx"]))
    tyc = tz * torch.clamp(t[:, 1] / tz, -1.3 * (0.5 * H / K["fy"]), 1.3 * (0.5 * H / K["fy"]))
    rz = 1.0 / tz
    zero = torch.zeros_like(rz)
    J = torch.stack([K["fx"] * rz, zero, -K["fx"] * txc * rz * rz, zero, K["fy"] * rz, -K["fy"] * tyc * rz * rz], -1).reshape(-1, 2, 3)
    Tm = J @ WT
    cov = Tm @ Sigma @ Tm.transpose(1, 2)
    a, b, d = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * d - b * b
    conics = torch.stack([d / det, -b / det, a / det], -1)
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    _, _, radii, ref_conics, _, _ = rt.project_gaussians(p["means"], scales, 1.0, quats, V, torch.tensor(F4, dtype=dtype), K["fx"], K["fy"],
                                                        K["cx"], K["cy"], H, W, tb)
    kept = radii > 0
    cot = torch.tensor(S.cotangents(name, "b")["conics"][view], dtype=dtype)
    (g,) = torch.autograd.grad((conics[kept] * cot[kept]).sum(), [WT])
    return g.numpy().astype(np.float64), float((conics[kept] - ref_conics[kept]).detach().abs().max())


# ---------------------------------------------------------------------------------------- whole render, the view matrix a leaf
def whole_render_ref(P, viewmat, c2w_origin, K, background, v_rgb=None, target=None, sh_degree_to_use=3, dtype=torch.float64, leaf_grads=True):
    """oracle.raster_torch.get_outputs, training form, restated from its own pieces with viewmat [3, 4] (a tensor, possibly part of a
    graph) in place of the camera glue: fullproj = projmat4 @ viewmat4.  The view directions use c2w_origin, a constant.  The loss is
    sum(rgb * v_rgb), or oracle.sd15_torch.splat_loss(rgb, target).  Returns (rgb, loss, params with requires_grad)."""
    import math
    from oracle import raster_torch as rt
    p = {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(leaf_grads) for k, v in P.items()}
    W, H = K["W"], K["H"]
    V4 = torch.cat([viewmat.to(dtype), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=dtype)], 0)
    proj = rt.projection_matrix(0.001, 1000, 2 * math.atan(W / (2 * K["fx"])), 2 * math.atan(H / (2 * K["fy"])), dtype=torch.float32).to(dtype)
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    colors = torch.cat([p["features_dc"][:, None, :], p["features_rest"]], 1)
    quats = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
    xys, depths, radii, conics, nth, _ = rt.project_gaussians(p["means"], torch.exp(p["scales"]), 1.0, quats, V4[:3], proj @ V4, K["fx"], K["fy"],
                                                              K["cx"], K["cy"], H, W, tb)
    viewdirs = p["means"].detach() - torch.tensor(np.asarray(c2w_origin), dtype=dtype)
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    rgbs = torch.clamp(rt.spherical_harmonics(sh_degree_to_use, viewdirs, colors) + 0.5, min=0.0)
    opac = torch.sigmoid(p["opacities"])[:, 0]
    _, ids, bins = rt.bin_and_sort(xys, depths, radii, nth, tb)
    rgb, _, _, _ = rt.rasterize(xys, conics, rgbs, opac, ids, bins, H, W, tb, torch.tensor(np.asarray(background), dtype=dtype))
    rgb = torch.clamp(rgb, max=1.0)
    if target is not None:
        from oracle import sd15_torch as sd
        loss = sd.splat_loss(rgb, torch.as_tensor(target).to(dtype))
    else:
        loss = (rgb * torch.tensor(np.asarray(v_rgb), dtype=dtype)).sum()
    return rgb, loss, p


def glue_viewmat(c2w):
    """[3, 4] float64 tensor of the float32 view matrix the product's camera glue builds for c2w"""
    from gaussctrl_amd.camera import camera_to_gsplat
    return torch.tensor(np.asarray(camera_to_gsplat(c2w, 1.0, 1.0, 0.0, 0.0, 2, 2)["viewmat4"], np.float64)[:3])


# ---------------------------------------------------------------------------------------- pose recovery
# Sized once on the CPU with the float64 oracle (oracle_recovery below, run by hand; tests/test_pose_cpu.py does not repeat it -- it takes
# minutes): the oracle's own run ends at the mean pose error recorded in RECOVERY["oracle_final_over_start"].
RECOVERY = dict(N=400, W=48, H=32, fx=40.0, scale_mean=0.12, views=4, seed=21, steps=120, lr=3e-3, rot=0.02, trans=0.02,
                oracle_final_over_start=0.092)         # measured: mean pose error 0.0400 -> 0.00368, loss 0.0260 -> 0.00166 (60 steps at 2e-3: 0.40)


def recovery_scene():
    """(parameters, true camera-to-worlds [4, 3, 4], intrinsics, the seeded start rows [4, 6] of about 0.02 rad and 0.02 units)"""
    from gaussctrl_amd import synthetic as syn
    r = RECOVERY
    P = syn.make_gaussians(r["N"], seed=r["seed"], scale_mean=r["scale_mean"])
    c2ws = syn.make_cameras(r["views"], seed=r["seed"] + 1)
    K = dict(fx=r["fx"], fy=r["fx"] * 0.99, cx=r["W"] / 2 + 1.3, cy=r["H"] / 2 - 2.1, W=r["W"], H=r["H"])
    g = np.random.default_rng(r["seed"] + 2)
    d = g.normal(size=(r["views"], 2, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rows = np.concatenate([d[:, 0] * r["trans"], d[:, 1] * r["rot"]], 1)
    return P, c2ws, K, rows


def start_poses(c2ws, rows):
    """the poses training starts from: each true pose off by its row, float32 [V, 3, 4] (so that the row -rows[v], to first order, recovers it)"""
    from gaussctrl_amd import camera_opt
    return np.stack([camera_opt.adjusted_c2w(c, torch.tensor(r)) for c, r in zip(c2ws, rows)])


def pose_error(c2w_start, row, c2w_true):
    """(rotation angle in rad, translation distance) between compose(c2w_start, row) and the true pose"""
    from gaussctrl_amd import camera_opt
    c = camera_opt.compose(c2w_start, torch.as_tensor(row).detach().cpu()).detach().numpy()
    t = np.asarray(c2w_true, np.float64)[:3]
    cosang = (np.trace(c[:, :3].T @ t[:, :3]) - 1.0) / 2.0
    return float(np.arccos(np.clip(cosang, -1.0, 1.0))), float(np.linalg.norm(c[:, 3] - t[:, 3]))


def mean_pose_error(starts, rows, c2ws):
    """mean over the views of (angle + distance): both start near 0.02"""
    return float(np.mean([sum(pose_error(s, r, t)) for s, r, t in zip(starts, rows, c2ws)]))


def oracle_recovery(verbose=False):
    """the recovery run on the float64 oracle: Adam (torch.optim) on the rows alone, one view per step in turn, loss = splat_loss against the
    target rendered from the true pose.  Returns (mean pose error at the start, at the end, first loss, last loss over the final round)."""
    from gaussctrl_amd import camera_opt
    r = RECOVERY
    P, c2ws, K, rows0 = recovery_scene()
    starts = start_poses(c2ws, rows0)
    bg = np.zeros(3)
    with torch.no_grad():
        targets = [whole_render_ref(P, glue_viewmat(c), c[:3, 3], K, bg, v_rgb=0.0, leaf_grads=False)[0] for c in c2ws]
    rows = torch.zeros(r["views"], 6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([rows], lr=r["lr"], eps=1e-15)
    e0 = mean_pose_error(starts, rows, c2ws)
    losses = []
    for step in range(r["steps"]):
        v = step % r["views"]
        opt.zero_grad()
        c2w = camera_opt.compose(starts[v], rows[v])
        # the product rounds the composed pose to float32 before the glue; the oracle differentiates through the unrounded one
        _, loss, _ = whole_render_ref(P, camera_opt.viewmat_of(c2w), c2w[:, 3].detach().numpy(), K, bg, target=targets[v], leaf_grads=False)
        loss.backward()
        opt.step()
        losses.append(float(loss))
        if verbose:
            print(step, v, float(loss), mean_pose_error(starts, rows, c2ws))
    return e0, mean_pose_error(starts, rows, c2ws), float(np.mean(losses[:r["views"]])), float(np.mean(losses[-r["views"]:]))

"""The projection / SH kernels of raster_project.hip alone, with the camera inside the cloud, against a float64 reference per row.

Every training gradient of means, scales, quaternions, opacities and SH passes through project_one_bwd / geom_vjp / colour_vjp.  The other
test files hold their backward against a reference only through a whole render behind float atomics, at 1e-3 of each tensor's max, on
scenes where no Gaussian is behind, near or around the camera.  Here the entry points are called on their own, with seeded cotangents on
their outputs, on the scenes of tests/_inside_scene.py (census, bars and their derivation: tests/test_project_vjp_cpu.py), and every
gradient row is held to BARS by the row metric e_row = |got - ref|_2 / (|ref_row|_2 + floor_row) against float64 autograd of front_ref.

Cotangent sets (seeded normal): a = every output, b = conics only, c = xys only, d = depths only (where the entry point takes one).
Every buffer an entry point writes starts NaN-filled and is finite afterwards.

The last two tests render the same scenes whole (render_view / render_views against oracle_c.render at the unchanged bars of
test_raster_gpu): the first renders with tile lists from Gaussians hundreds of pixels wide and a third of the scene behind the camera.
"""
import numpy as np
import pytest
import torch

import _inside_scene as S
from _margins import within
from _redzone import on_device
from test_raster_antialias_gpu import RHO_BAR
from test_raster_gpu import _grad_close, _img_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = np.array([0.1, 0.2, 0.3], np.float32)
NAN = float("nan")
F32 = dict(dtype=torch.float32, device=DEV)
I32 = dict(dtype=torch.int32, device=DEV)


def _t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _cams(name, views=None):
    from gaussctrl_amd.camera import camera_to_gsplat
    _, c2ws, K = S.scene(name)
    return [camera_to_gsplat(c2ws[v], K["fx"], K["fy"], K["cx"], K["cy"], K["W"], K["H"]) for v in (range(len(c2ws)) if views is None else views)]


def _leaves(name, deg=3):
    """the six parameter tensors as the raw entry points take them (opacity logits flat)"""
    tp = {k: _t(v) for k, v in S.with_degree(S.scene(name)[0], deg).items()}
    tp["opacities"] = tp["opacities"].reshape(-1)
    return tp


def _params(tp):
    from gaussctrl_amd import _lib as L
    return [L.ptr(tp[k]) for k in ("means", "scales", "quats", "opacities")]


def _nan_grads(tp):
    return {k: torch.full(tuple(tp[k].shape), NAN, **F32) for k in S.KEYS}


def _seeded_grads(tp, seed):
    g = np.random.default_rng(seed)
    return {k: _t(g.normal(size=tuple(tp[k].shape)).astype(np.float32)) for k in S.KEYS}


def _cot(name, cset, depth, C, N):
    """device cotangents [C][N][..] of the set; what the set leaves out is zero"""
    c = S.cotangents(name, cset, depth)
    out = {k: _t(c[k][:C]) if k in c else torch.zeros((C, N) + sh, **F32) for k, sh in (("xys", (2,)), ("conics", (3,)), ("rgbs", (3,)), ("opac", ()))}
    out["depths"] = _t(c["depths"][:C]) if "depths" in c else None
    return out


def _forward_views(tp, cams, deg, n_use, K, aa=False):
    """gc_project_sh_fwd_views / gc_project_sh_fwd_aa_views into NaN-filled (integers: -1) buffers [C][N][..]"""
    from gaussctrl_amd import _lib as L, gsplat_ops as ops
    lib = L.lib()
    N, C = tp["means"].shape[0], len(cams)
    o = dict(xys=torch.full((C, N, 2), NAN, **F32), depths=torch.full((C, N), NAN, **F32), radii=torch.full((C, N), -1, **I32),
             conics=torch.full((C, N, 3), NAN, **F32), nth=torch.full((C, N), -1, **I32), rgbs=torch.full((C, N, 3), NAN, **F32),
             opac=torch.full((C, N) if aa else (N,), NAN, **F32), boxes=torch.full((C, N), -1, **I32))
    tx, ty = (K["W"] + 15) // 16, (K["H"] + 15) // 16
    head = (L.i64(N), L.i32(C), *_params(tp), L.ptr(tp["features_dc"]), L.ptr(tp["features_rest"]), L.i32(deg), L.i32(n_use), ops._cams_host(cams),
            L.i32(K["H"]), L.i32(K["W"]), L.i32(tx), L.i32(ty), L.f32(0.01), L.ptr(o["xys"]), L.ptr(o["depths"]), L.ptr(o["radii"]), L.ptr(o["conics"]),
            L.ptr(o["nth"]), L.ptr(o["rgbs"]), L.ptr(o["opac"]))
    if aa:
        o["comp"] = torch.full((C, N), NAN, **F32)
        L.check(lib.gc_project_sh_fwd_aa_views(*head, L.ptr(o["comp"]), L.ptr(o["boxes"]), None, L.stream_ptr()), "gc_project_sh_fwd_aa_views")
    else:
        L.check(lib.gc_project_sh_fwd_views(*head, L.ptr(o["boxes"]), None, L.stream_ptr()), "gc_project_sh_fwd_views")
    return o


def _check_forward(label, o, v, ref_out, K, aa=False):
    """view v of the forward state against front_ref's outputs, per row at FWD_BARS; the compensation at the antialias file's RHO_BAR"""
    radii = o["radii"][v].cpu().numpy()
    off = radii != ref_out["radii"]                     # (a radius one off does not touch the float outputs)
    assert int(off.sum()) <= 1 and np.all(np.abs(radii - ref_out["radii"]) <= 1) and np.all(radii[off] > 0) and np.all(ref_out["radii"][off] > 0), label
    got = {k: o[k][v].cpu().numpy() for k in ("xys", "depths", "conics", "rgbs")}
    if not aa:
        got["opac"] = o["opac"].cpu().numpy()
    for k, e in S.forward_errors(got, ref_out, K, aa).items():
        within(f"{label}: forward {k} worst row error", e, S.FWD_BARS[k])
    if aa:
        comp, opac = o["comp"][v].cpu().numpy().astype(np.float64), o["opac"][v].cpu().numpy().astype(np.float64)
        assert np.isfinite(comp).all() and np.isfinite(opac).all() and np.all(comp[ref_out["radii"] == 0] == 0)
        within(f"{label}: compensation vs float64 rho", np.abs(comp - ref_out["rho"]).max(), RHO_BAR)
        within(f"{label}: effective opacity vs float64 sigmoid * rho", np.abs(opac - ref_out["opac"]).max(), RHO_BAR + S.FWD_BARS["opac"])


def _rest_beyond_is_zero(vrest, n_use):
    used = (n_use + 1) ** 2 - 1 if n_use >= 0 else 0
    assert bool((vrest[:, used:] == 0).all()), "features_rest gradient beyond sh_degree_to_use"


# ---------------------------------------------------------------------------------------- gsplat operator surface
@pytest.mark.parametrize("name", ["in3", "in7", "tiny"])
def test_project_gaussians_bit_exact_from_inside(oracle_c, name):
    """test_raster_gpu.test_project_gaussians_bit_exact's claim with the camera inside the cloud: Gaussians behind it, a few centimetres in
    front of it, clamped by the frustum limit in either direction, radii of hundreds of pixels"""
    from gaussctrl_amd import gsplat_ops as ops
    P, _, K = S.scene(name)
    cam, = _cams(name)
    W, H = K["W"], K["H"]
    scales = np.exp(P["scales"]).astype(np.float32)
    qn = (P["quats"] / np.linalg.norm(P["quats"], axis=-1, keepdims=True)).astype(np.float32)
    tb = cam["tile_bounds"]
    V4 = cam["viewmat4"]; full = np.asarray(cam["fullproj"], np.float32).reshape(4, 4)
    ref = oracle_c.project_gaussians(P["means"], scales, 1.0, qn, V4[:3], full, K["fx"], K["fy"], K["cx"], K["cy"], H, W, tb)
    got = ops.project_gaussians(_t(P["means"]), _t(scales), 1.0, _t(qn), V4[:3], full, K["fx"], K["fy"], K["cx"], K["cy"], H, W, tb)
    assert int((ref[2] > 0).sum()) == S.census(name)[0]["visible"]
    for n, r, g in zip(["xys", "depths", "radii", "conics", "num_tiles_hit", "cov3d"], ref, got):
        g = g.cpu().numpy()
        assert np.array_equal(r.view(np.int32) if r.dtype == np.float32 else r, g.view(np.int32) if g.dtype == np.float32 else g), f"{n} not bit-exact"


@pytest.mark.parametrize("name", ["in3", "in7", "tiny"])
def test_project_gaussians_backward_vs_float64(name):
    """ops.project_gaussians' autograd backward (gc_project_gaussians_bwd) behind torch's exp and q / |q| on the device, sets a to d; and the
    entry point itself once with v_depth = NULL into NaN-filled buffers: the bits of the same call with a zero depth cotangent"""
    from gaussctrl_amd import _lib as L, gsplat_ops as ops
    P, _, K = S.scene(name)
    cam, = _cams(name)
    W, H, N = K["W"], K["H"], P["means"].shape[0]
    V4 = cam["viewmat4"]; full = np.asarray(cam["fullproj"], np.float32).reshape(4, 4)
    m, ls, q = (_t(P[k]).requires_grad_(True) for k in ("means", "scales", "quats"))
    scales, qn = torch.exp(ls), q / q.norm(dim=-1, keepdim=True)
    xys, depths, radii, conics, _, _ = ops.project_gaussians(m, scales, 1.0, qn, V4[:3], full, K["fx"], K["fy"], K["cx"], K["cy"], H, W, cam["tile_bounds"])
    outs = dict(xys=xys, depths=depths, conics=conics)
    for cset, depth in (("a", True), ("b", False), ("c", False), ("d", False)):
        cot = {k: v[0] for k, v in S.cotangents(name, cset, depth).items() if k in outs}
        loss = sum((outs[k] * _t(v)).sum() for k, v in cot.items())
        gs = torch.autograd.grad(loss, (m, ls, q), retain_graph=True, allow_unused=True)
        got = {k: torch.zeros_like(t) if g is None else g for k, t, g in zip(("means", "scales", "quats"), (m, ls, q), gs)}
        S.check_grads(f"project_gaussians {name} set {cset}", got, S.ref_views(name, cset=cset, depth=depth), keys=("means", "scales", "quats"))
    cot = {k: _t(v[0]) for k, v in S.cotangents(name, "a").items() if k in outs}
    want = torch.autograd.grad(sum((outs[k] * v).sum() for k, v in cot.items()), (m, scales, qn))
    raw = [torch.full((N, 3), NAN, **F32), torch.full((N, 3), NAN, **F32), torch.full((N, 4), NAN, **F32)]
    L.check(L.lib().gc_project_gaussians_bwd(
        L.i64(N), L.ptr(m.detach()), L.ptr(scales.detach()), L.f32(1.0), L.ptr(qn.detach()), L.host_floats(cam["viewmat"]), L.host_floats(cam["fullproj"]),
        L.f32(K["fx"]), L.f32(K["fy"]), L.f32(K["cx"]), L.f32(K["cy"]), L.i32(H), L.i32(W), L.ptr(radii), L.ptr(conics.detach()), L.ptr(cot["xys"]),
        None, L.ptr(cot["conics"]), *[L.ptr(t) for t in raw], L.stream_ptr()), "gc_project_gaussians_bwd")
    for a, b in zip(raw, want):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


# ---------------------------------------------------------------------------------------- fused front end, one camera
@pytest.mark.parametrize("deg,n_use", S.SH_MODES)
@pytest.mark.parametrize("name", ["in3", "in7", "tiny"])
def test_fused_single_view(oracle_c, name, deg, n_use):
    """gc_project_sh_fwd, gc_project_sh_bwd and gc_project_sh_bwd_accumulate through the raw ABI, every K instantiation (deg) and every
    colour path of K = 16 (n_use = -1: sigmoid colours): forward per row against front_ref, radii / num_tiles_hit against the float32 C
    oracle (at most one row may differ, by 1: expf of a log-scale can fall on a ceil edge), the six gradients against float64 under set a --
    at deg = n_use = 3 also b and c; the entry point takes no depth cotangent -- then accumulated onto a seeded non-zero buffer x, where
    (result - x) is held to the bar plus 2^-23 |x_row|."""
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    P, _, K = S.scene(name)
    cam, = _cams(name)
    W, H, N = K["W"], K["H"], P["means"].shape[0]
    tp = _leaves(name, deg)
    o = dict(xys=torch.full((1, N, 2), NAN, **F32), depths=torch.full((1, N), NAN, **F32), radii=torch.full((1, N), -1, **I32),
             conics=torch.full((1, N, 3), NAN, **F32), nth=torch.full((1, N), -1, **I32), rgbs=torch.full((1, N, 3), NAN, **F32),
             opac=torch.full((N,), NAN, **F32))
    camargs = (L.host_floats(cam["viewmat"]), L.host_floats(cam["fullproj"]), L.host_floats(cam["origin"]), L.f32(K["fx"]), L.f32(K["fy"]),
               L.f32(K["cx"]), L.f32(K["cy"]), L.i32(H), L.i32(W))
    L.check(lib.gc_project_sh_fwd(L.i64(N), *_params(tp), L.ptr(tp["features_dc"]), L.ptr(tp["features_rest"]), L.i32(deg), L.i32(n_use), *camargs,
                                  L.i32((W + 15) // 16), L.i32((H + 15) // 16), L.f32(0.01), L.ptr(o["xys"]), L.ptr(o["depths"]), L.ptr(o["radii"]),
                                  L.ptr(o["conics"]), L.ptr(o["nth"]), L.ptr(o["rgbs"]), L.ptr(o["opac"]), L.stream_ptr()), "gc_project_sh_fwd")
    # integers against the float32 C oracle (fed numpy's exp), everything else against float64
    scales = np.exp(P["scales"]).astype(np.float32)
    qn = (P["quats"] / np.linalg.norm(P["quats"], axis=-1, keepdims=True)).astype(np.float32)
    full = np.asarray(cam["fullproj"], np.float32).reshape(4, 4)
    c = oracle_c.project_gaussians(P["means"], scales, 1.0, qn, cam["viewmat4"][:3], full, K["fx"], K["fy"], K["cx"], K["cy"], H, W, cam["tile_bounds"])
    radii, nth = o["radii"][0].cpu().numpy(), o["nth"][0].cpu().numpy()
    off = radii != c[2]
    assert int(off.sum()) <= 1 and np.all(np.abs(radii - c[2]) <= 1) and np.all((nth == c[4]) | off), (int(off.sum()), int((nth != c[4]).sum()))
    ref = S.ref_views(name, deg, n_use, cset="a")
    _check_forward(f"fused {name} deg {deg} n_use {n_use}", o, 0, ref["outs"][0], K)
    bwd_tail = lambda cot, out: (L.ptr(o["radii"]), L.ptr(o["conics"]), L.ptr(cot["xys"]), L.ptr(cot["conics"]), L.ptr(cot["rgbs"]), L.ptr(cot["opac"]),
                                 *[L.ptr(out[k]) for k in S.KEYS], L.stream_ptr())
    head = (L.i64(N), *_params(tp), L.ptr(o["rgbs"]), L.i32(deg), L.i32(n_use), *camargs)
    for cset in ("a", "b", "c") if (deg, n_use) == (3, 3) else ("a",):
        out = _nan_grads(tp)
        L.check(lib.gc_project_sh_bwd(*head, *bwd_tail(_cot(name, cset, False, 1, N), out)), "gc_project_sh_bwd")
        S.check_grads(f"fused {name} deg {deg} n_use {n_use} set {cset}", out, S.ref_views(name, deg, n_use, cset=cset))
        _rest_beyond_is_zero(out["features_rest"], n_use)
    x = _seeded_grads(tp, 11)
    out = {k: on_device(v, DEV) for k, v in x.items()}
    L.check(lib.gc_project_sh_bwd_accumulate(*head, *bwd_tail(_cot(name, "a", False, 1, N), out)), "gc_project_sh_bwd_accumulate")
    S.check_grads(f"fused {name} deg {deg} n_use {n_use} accumulate", out, ref, before=x)


# ---------------------------------------------------------------------------------------- fused front end, C cameras
@pytest.mark.parametrize("C", [9, 1])
def test_views_backward(C):
    """gc_project_sh_bwd_views and gc_project_sh_bwd_depth_views on views9 (C = 9: two launches, the second adds to the first) and on its first
    view (C = 1: the single-view kernel behind the depth entry), accumulate 0 and 1, against the float64 sum over the views"""
    from gaussctrl_amd import _lib as L, gsplat_ops as ops
    lib = L.lib()
    name, views = "views9", tuple(range(C))
    P, _, K = S.scene(name)
    N = P["means"].shape[0]
    tp = _leaves(name)
    cams = _cams(name, views)
    o = _forward_views(tp, cams, 3, 3, K)
    for v in views:
        _check_forward(f"views C {C} view {v}", o, v, S.ref_views(name, views=(v,))["outs"][0], K)
    head = lambda acc: (L.i64(N), L.i32(C), L.i32(acc), *_params(tp), L.ptr(o["rgbs"]), L.i32(3), L.i32(3), ops._cams_host(cams), L.i32(K["H"]),
                        L.i32(K["W"]), L.ptr(o["radii"]), L.ptr(o["conics"]))
    tail = lambda cot, out: (L.ptr(cot["xys"]), L.ptr(cot["conics"]), L.ptr(cot["rgbs"]), L.ptr(cot["opac"]), *[L.ptr(out[k]) for k in S.KEYS])
    for depth, cset, acc in [(d, "a", a) for d in (False, True) for a in (0, 1)] + [(True, s, 0) for s in "bcd"]:
        cot = _cot(name, cset, depth, C, N)
        x = _seeded_grads(tp, 12 + acc) if acc else None
        out = {k: on_device(v, DEV) for k, v in x.items()} if acc else _nan_grads(tp)
        if depth:
            v_dep = cot["depths"] if cot["depths"] is not None else torch.zeros((C, N), **F32)
            L.check(lib.gc_project_sh_bwd_depth_views(*head(acc), *tail(cot, out), L.ptr(v_dep), L.stream_ptr()), "gc_project_sh_bwd_depth_views")
        else:
            L.check(lib.gc_project_sh_bwd_views(*head(acc), *tail(cot, out), L.stream_ptr()), "gc_project_sh_bwd_views")
        S.check_grads(f"views C {C} set {cset}{' depth' if depth else ''} accumulate {acc}", out,
                      S.ref_views(name, cset=cset, depth=depth and cset == "a", views=views), before=x)


@pytest.mark.parametrize("C", [9, 1])
def test_views_antialiased(C):
    """gc_project_sh_fwd_aa_views / gc_project_sh_bwd_aa_views against front_ref(aa=True): compensation at the antialias file's RHO_BAR, the
    gradients at the same BARS as the classic mode (v_rho joins the covariance cotangent in project_one_bwd's closed form), without and
    with a depth cotangent, accumulate 0 and 1"""
    from gaussctrl_amd import _lib as L, gsplat_ops as ops
    lib = L.lib()
    name, views = "views9", tuple(range(C))
    P, _, K = S.scene(name)
    N = P["means"].shape[0]
    tp = _leaves(name)
    cams = _cams(name, views)
    o = _forward_views(tp, cams, 3, 3, K, aa=True)
    for v in views:
        _check_forward(f"aa views C {C} view {v}", o, v, S.ref_views(name, aa=True, views=(v,))["outs"][0], K, aa=True)
    for depth, acc in ((False, 0), (True, 0), (True, 1)):
        cot = _cot(name, "a", depth, C, N)
        x = _seeded_grads(tp, 14) if acc else None
        out = {k: on_device(v, DEV) for k, v in x.items()} if acc else _nan_grads(tp)
        L.check(lib.gc_project_sh_bwd_aa_views(
            L.i64(N), L.i32(C), L.i32(acc), *_params(tp), L.ptr(o["rgbs"]), L.i32(3), L.i32(3), ops._cams_host(cams), L.i32(K["H"]), L.i32(K["W"]),
            L.ptr(o["radii"]), L.ptr(o["conics"]), L.ptr(o["comp"]), L.ptr(cot["xys"]), L.ptr(cot["conics"]), L.ptr(cot["rgbs"]), L.ptr(cot["opac"]),
            *[L.ptr(out[k]) for k in S.KEYS], L.ptr(cot["depths"]), L.stream_ptr()), "gc_project_sh_bwd_aa_views")
        S.check_grads(f"aa views C {C}{' depth' if depth else ''} accumulate {acc}", out, S.ref_views(name, aa=True, depth=depth, views=views), before=x)


# ---------------------------------------------------------------------------------------- whole render from inside, existing bars
def _upstream(H, W, seed, C=None):
    g = np.random.default_rng(seed)
    sh = (H, W) if C is None else (C, H, W)
    return g.normal(size=sh + (3,)).astype(np.float32), g.normal(size=sh).astype(np.float32)


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("name", ["in3", "in7"])
def test_render_view_from_inside(oracle_c, name, training):
    """render_view against oracle_c.render at test_raster_gpu's bars: image, alpha, depth with its far mask, the six gradients, xys_grad"""
    from gaussctrl_amd import gsplat_ops as ops
    P, c2ws, K = S.scene(name)
    W, H = K["W"], K["H"]
    v_rgb, v_a = _upstream(H, W, 2)
    o = oracle_c.render(P, c2ws[0], K["fx"], K["fy"], K["cx"], K["cy"], W, H, BG, training=training, v_rgb=v_rgb, v_alpha=v_a)
    assert int((o["radii"] > 0).sum()) == S.census(name)[0]["visible"] and o["radii"].max() > 500
    tp = {k: _t(v).requires_grad_(True) for k, v in P.items()}
    aux = ops.RenderAux()
    rgb, alpha, depth = ops.render_view(*(tp[k] for k in S.KEYS), _cams(name)[0], _t(BG), not training, 3, aux)
    assert all(bool(torch.isfinite(t).all()) for t in (rgb, alpha))
    _img_close(rgb.detach().cpu().numpy(), o["rgb"])
    _img_close(alpha.detach().cpu().numpy(), o["accumulation"][..., 0])
    assert int((aux.radii.cpu().numpy() != o["radii"]).sum()) <= 1
    if not training:
        d = depth.cpu().numpy(); od = o["depth"][..., 0]
        far = od == 1000.0
        assert np.array_equal(far, d == 1000.0) and np.isfinite(d).all()
        _img_close(np.where(far, 0, d), np.where(far, 0, od))
    ((rgb * _t(v_rgb)).sum() + (alpha * _t(v_a)).sum()).backward()
    scale = max(np.abs(o["grads"][k]).max() for k in P)
    for k in P:
        assert bool(torch.isfinite(tp[k].grad).all()), k
        _grad_close(tp[k].grad.cpu().numpy(), o["grads"][k], scale)
    _grad_close(aux.xys_grad.cpu().numpy(), o["grads"]["xys"], scale)


def test_render_views_from_inside(oracle_c):
    """render_views on three views of views9 against the per-view oracle: images per view, leaf gradients of the summed loss"""
    from gaussctrl_amd import gsplat_ops as ops
    P, c2ws, K = S.scene("views9")
    W, H, views = K["W"], K["H"], S.RENDER_VIEWS
    v_rgb, v_a = _upstream(H, W, 3, len(views))
    tp = {k: _t(v).requires_grad_(True) for k, v in P.items()}
    aux = ops.RenderAux()
    rgb, alpha, _ = ops.render_views(*(tp[k] for k in S.KEYS), _cams("views9", views), _t(BG), False, 3, aux)
    ((rgb * _t(v_rgb)).sum() + (alpha * _t(v_a)).sum()).backward()
    ref_g = {k: np.zeros(v.shape, np.float64) for k, v in P.items()}
    per_view = []
    for i, v in enumerate(views):
        o = oracle_c.render(P, c2ws[v], K["fx"], K["fy"], K["cx"], K["cy"], W, H, BG, training=True, v_rgb=v_rgb[i], v_alpha=v_a[i])
        _img_close(rgb[i].detach().cpu().numpy(), o["rgb"])
        _img_close(alpha[i].detach().cpu().numpy(), o["accumulation"][..., 0])
        per_view.append(o["grads"]["xys"])
        for k in P:
            ref_g[k] += o["grads"][k]
    scale = max(np.abs(v).max() for v in ref_g.values())
    for k in P:
        assert bool(torch.isfinite(tp[k].grad).all()), k
        _grad_close(tp[k].grad.cpu().numpy(), ref_g[k], scale)
    for i in range(len(views)):
        _grad_close(aux.xys_grad[i].cpu().numpy(), per_view[i], scale)

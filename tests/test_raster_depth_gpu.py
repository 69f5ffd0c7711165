"""GPU tests of depth supervision: the depth image of the fused render (gsplat_ops.render_view / render_views with
RenderAux.depth_grad) as a differentiable output, the projection backward with v_depths, and the depth L1 loss.

Reference of every gradient: oracle.raster_torch.get_outputs(params with requires_grad, ..., training=False, dtype=float64) on the CPU,
differentiated by autograd, for

    L = sum(rgb * v_rgb) + sum(alpha * v_a) + sum(where(depth != 1000, depth, 0) * v_d).

Bars: tests/test_raster_gpu.py's _img_close (images) and _grad_close (gradients), which gives NO knife-edge allowance below 500 k
Gaussians.  The scene seeds were therefore picked on the CPU first: the oracle run in float32 and in float64 gives the same final_index,
the same depth == 1000 mask, the same radii and the same sorted lists for every scene and camera used here, i.e. no (pixel, splat)
decision sits on a knife edge.  Seeds (syn.make_gaussians seed / syn.make_cameras seed):

    scene (a) N = 3000, 72 x 40, scale_mean 0.05: Gaussians 4, camera 5  (longest tile list 984 entries, 6.9 % empty pixels, 60 % of the
              pixels saturated at alpha > 0.999; partial tiles on the right and bottom edges)
    scene (b) N = 7, 33 x 17, scale_mean 0.3:     Gaussians 3, camera 4
    scene (c) = (a) with the opacity logits raised by 6: pixels reach the T <= 1e-4 stop and the 0.999 alpha cap
    views     scene (a)'s Gaussians under syn.make_cameras(9, seed=12); C = 3 takes the first three
"""
import numpy as np
import pytest
import torch

from _margins import within
from _redzone import on_device
from _train_step_ref import depth_l1_ref
from gaussctrl_amd import synthetic as syn
from test_raster_gpu import _grad_close, _img_close

pytestmark = pytest.mark.gpu
BG = np.array([0.1, 0.2, 0.3], np.float32)
DEV = "cuda:0"
KEYS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
SCENES = {"a": dict(N=3000, W=72, H=40, fx=60.0, sm=0.05, seed=4, op_shift=0.0),
          "b": dict(N=7, W=33, H=17, fx=40.0, sm=0.3, seed=3, op_shift=0.0),
          "c": dict(N=3000, W=72, H=40, fx=60.0, sm=0.05, seed=4, op_shift=6.0)}
VIEW_CAM_SEED = 12
_CACHE = {}


def _t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _intr(s):
    return dict(fx=s["fx"], fy=s["fx"] * 0.99, cx=s["W"] / 2 + 1.3, cy=s["H"] / 2 - 2.1, W=s["W"], H=s["H"])


def _scene(name):
    """(parameters, camera-to-world of the scene's own camera, intrinsics)"""
    if ("scene", name) not in _CACHE:
        s = SCENES[name]
        P = syn.make_gaussians(s["N"], seed=s["seed"], scale_mean=s["sm"])
        P["opacities"] = (P["opacities"] + np.float32(s["op_shift"])).astype(np.float32)
        _CACHE[("scene", name)] = (P, syn.make_cameras(1, seed=s["seed"] + 1)[0], _intr(s))
    return _CACHE[("scene", name)]


def _cotangents(H, W, seed):
    g = np.random.default_rng(seed)
    return (g.normal(size=(H, W, 3)).astype(np.float32), g.normal(size=(H, W)).astype(np.float32), g.normal(size=(H, W)).astype(np.float32))


def _oracle(P, c2w, K, cot):
    """float64 oracle render + the gradients of L (all three terms), of L without the depth term and of the depth term alone.
    Returns dict(rgb, alpha, depth, full / nodepth / depthonly -> {six leaves + "xys"})."""
    from oracle import raster_torch as rt
    p = {k: torch.tensor(v, dtype=torch.float64).requires_grad_(True) for k, v in P.items()}
    o = rt.get_outputs(p, torch.tensor(c2w), K["fx"], K["fy"], K["cx"], K["cy"], K["W"], K["H"], torch.tensor(BG), training=False,
                       dtype=torch.float64)
    v_rgb, v_a, v_d = (torch.tensor(c, dtype=torch.float64) for c in cot)
    depth = o["depth"][..., 0]
    l_rgb = (o["rgb"] * v_rgb).sum() + (o["accumulation"][..., 0] * v_a).sum()
    l_dep = (torch.where(depth != 1000.0, depth, torch.zeros_like(depth)) * v_d).sum()
    leaves = [p[k] for k in KEYS] + [o["xys"]]
    out = dict(rgb=o["rgb"].detach().numpy(), alpha=o["accumulation"][..., 0].detach().numpy(), depth=depth.detach().numpy())
    for name, loss in (("nodepth", l_rgb), ("depthonly", l_dep)):
        gs = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
        out[name] = {k: (torch.zeros_like(t) if g is None else g).numpy() for k, t, g in zip(KEYS + ("xys",), leaves, gs)}
    out["full"] = {k: out["nodepth"][k] + out["depthonly"][k] for k in out["nodepth"]}
    return out


def _oracle_scene(name):
    if ("oracle", name) not in _CACHE:
        P, c2w, K = _scene(name)
        _CACHE[("oracle", name)] = _oracle(P, c2w, K, _cotangents(K["H"], K["W"], 7))
    return _CACHE[("oracle", name)]


def _view_cams():
    if "cams" not in _CACHE:
        _CACHE["cams"] = syn.make_cameras(9, seed=VIEW_CAM_SEED)
    return _CACHE["cams"]


def _oracle_view(v):
    """oracle of scene (a)'s Gaussians under view v of the 9 batch cameras (cotangents seeded per view)"""
    if ("oracle_view", v) not in _CACHE:
        P, _, K = _scene("a")
        _CACHE[("oracle_view", v)] = _oracle(P, _view_cams()[v], K, _cotangents(K["H"], K["W"], 100 + v))
    return _CACHE[("oracle_view", v)]


def _leaves(P):
    return {k: _t(P[k]).requires_grad_(True) for k in KEYS}


def _render(tp, cam, aux, want_depth=True):
    from gaussctrl_amd import gsplat_ops as ops
    return ops.render_view(*(tp[k] for k in KEYS), cam, _t(BG), want_depth, 3, aux)


def _check_grads(tp, xys_grad, ref):
    scale = max(np.abs(ref[k]).max() for k in KEYS)
    for k in KEYS:
        assert tp[k].grad is not None, k
        _grad_close(tp[k].grad.cpu().numpy(), ref[k], scale)
    _grad_close(xys_grad.cpu().numpy(), ref["xys"], scale)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_depth_grad_single_view(name):
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.camera import camera_to_gsplat
    P, c2w, K = _scene(name)
    H, W = K["H"], K["W"]
    o = _oracle_scene(name)
    v_rgb, v_a, v_d = (_t(c) for c in _cotangents(H, W, 7))
    cam = camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], W, H)
    tp = _leaves(P)
    aux_off = ops.RenderAux()
    _, _, depth_off = _render(tp, cam, aux_off)
    assert depth_off.requires_grad is False
    aux = ops.RenderAux(); aux.depth_grad = True
    rgb, alpha, depth = _render(tp, cam, aux)
    assert depth.requires_grad and torch.equal(depth, depth_off)
    if name == "a":          # the scene is there for this: several staging batches behind one tile, partial tiles on both edges
        bins = aux.tile_bins.cpu().numpy()
        assert (bins[:, 1] - bins[:, 0]).max() > 256 and W % 16 and H % 16
    d = depth.detach().cpu().numpy()
    far = o["depth"] == 1000.0
    assert np.array_equal(far, d == 1000.0)
    _img_close(np.where(far, 0, d), np.where(far, 0, o["depth"]))
    _img_close(rgb.detach().cpu().numpy(), o["rgb"])
    dm = torch.where(depth != 1000.0, depth, torch.zeros_like(depth))
    ((rgb * v_rgb).sum() + (alpha * v_a).sum() + (dm * v_d).sum()).backward()
    _check_grads(tp, aux.xys_grad, o["full"])
    # depth only: a missing depth term cannot hide under the colour gradient
    tq = _leaves(P)
    aux2 = ops.RenderAux(); aux2.depth_grad = True
    _, _, depth2 = _render(tq, cam, aux2)
    (torch.where(depth2 != 1000.0, depth2, torch.zeros_like(depth2)) * v_d).sum().backward()
    _check_grads(tq, aux2.xys_grad, o["depthonly"])
    # sync-free frame: capacity-sized lists, the count stays on the device
    tr = _leaves(P)
    aux3 = ops.RenderAux(); aux3.depth_grad = True; aux3.m_cap = int(aux.M * 1.25) + 16
    rgb3, alpha3, depth3 = _render(tr, cam, aux3)
    cnt, ovf = aux3.M
    assert int(cnt) == aux.M and int(ovf) == 0 and torch.equal(depth3, depth)
    dm3 = torch.where(depth3 != 1000.0, depth3, torch.zeros_like(depth3))
    ((rgb3 * v_rgb).sum() + (alpha3 * v_a).sum() + (dm3 * v_d).sum()).backward()
    _check_grads(tr, aux3.xys_grad, o["full"])


def test_depth_grad_off_is_todays_path():
    """depth_grad = False (the default): depth is not differentiable and the rgb / alpha gradients are the oracle's"""
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.camera import camera_to_gsplat
    P, c2w, K = _scene("a")
    H, W = K["H"], K["W"]
    o = _oracle_scene("a")
    v_rgb, v_a, _ = (_t(c) for c in _cotangents(H, W, 7))
    cam = camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], W, H)
    tp = _leaves(P)
    aux = ops.RenderAux()
    assert aux.depth_grad is False
    rgb, alpha, depth = _render(tp, cam, aux)
    assert depth.requires_grad is False
    ((rgb * v_rgb).sum() + (alpha * v_a).sum()).backward()
    _check_grads(tp, aux.xys_grad, o["nodepth"])


@pytest.mark.parametrize("C", [3, 9])
def test_depth_grad_views(C):
    """render_views with depth_grad: against the oracle summed over the views, against C single-view render_view calls, and with
    grad_into + grad_accumulate on pre-filled buffers (C = 9 runs two camera groups of the projection backward)"""
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.camera import camera_to_gsplat
    P, _, K = _scene("a")
    H, W = K["H"], K["W"]
    cams = [camera_to_gsplat(c, K["fx"], K["fy"], K["cx"], K["cy"], W, H) for c in _view_cams()[:C]]
    cots = [tuple(_t(c) for c in _cotangents(H, W, 100 + v)) for v in range(C)]
    v_rgb, v_a, v_d = (torch.stack([c[j] for c in cots]) for j in range(3))
    ref = {k: sum(_oracle_view(v)["full"][k] for v in range(C)) for k in KEYS}

    def loss(rgb, alpha, depth, vr, va, vd):
        return (rgb * vr).sum() + (alpha * va).sum() + (torch.where(depth != 1000.0, depth, torch.zeros_like(depth)) * vd).sum()

    tp = _leaves(P)
    aux = ops.RenderAux(); aux.depth_grad = True
    rgb, alpha, depth = ops.render_views(*(tp[k] for k in KEYS), cams, _t(BG), True, 3, aux)
    assert depth.requires_grad
    for v in range(C):
        far = _oracle_view(v)["depth"] == 1000.0
        assert np.array_equal(far, depth[v].detach().cpu().numpy() == 1000.0)
    loss(rgb, alpha, depth, v_rgb, v_a, v_d).backward()
    scale = max(np.abs(ref[k]).max() for k in KEYS)
    for k in KEYS:
        _grad_close(tp[k].grad.cpu().numpy(), ref[k], scale)
    for v in range(C):
        _grad_close(aux.xys_grad[v].cpu().numpy(), _oracle_view(v)["full"]["xys"], scale)
    # the same gradients from C single-view calls (autograd sums them)
    ts = _leaves(P)
    for v in range(C):
        a1 = ops.RenderAux(); a1.depth_grad = True
        r1, al1, d1 = _render(ts, cams[v], a1)
        assert torch.equal(d1, depth[v].detach())
        loss(r1, al1, d1, *cots[v]).backward()
    single = {k: ts[k].grad.cpu().numpy() for k in KEYS}
    scale1 = max(np.abs(single[k]).max() for k in KEYS)
    for k in KEYS:
        _grad_close(tp[k].grad.cpu().numpy(), single[k], scale1)
    # grad_into + grad_accumulate on pre-filled buffers: previous contents + gradient
    g = torch.Generator(device="cpu").manual_seed(5)
    into = {k: on_device(torch.randn(tp[k].shape, generator=g) * float(np.abs(ref[k]).max()), DEV) for k in KEYS}
    into["opacities"] = into["opacities"].reshape(-1).contiguous()
    before = {k: t.clone() for k, t in into.items()}
    tq = _leaves(P)
    aux2 = ops.RenderAux(); aux2.depth_grad = True; aux2.grad_into = into; aux2.grad_accumulate = True
    rgb2, alpha2, depth2 = ops.render_views(*(tq[k] for k in KEYS), cams, _t(BG), True, 3, aux2)
    loss(rgb2, alpha2, depth2, v_rgb, v_a, v_d).backward()
    assert all(tq[k].grad is None for k in KEYS)
    for k in KEYS:
        added = (into[k].double() - before[k].double()).reshape(ref[k].shape).cpu().numpy()
        _grad_close(added, ref[k], scale)      # (pre-filled at the gradient's own magnitude: the extra float32 rounding of the sum is ~1e-7 of it)


def test_project_bwd_depth_entry():
    """gc_project_sh_bwd_depth_views with every other cotangent zero: v_means = v_depths * (row 2 of the view matrix) on visible Gaussians,
    zero on culled ones; v_log_scales and v_quats exactly zero.  C = 1 (single-view kernel) and C = 3 (view loop)."""
    from gaussctrl_amd import _lib as L
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.camera import camera_to_gsplat
    P, _, K = _scene("a")
    H, W, N = K["H"], K["W"], P["means"].shape[0]
    lib = L.lib()
    rng = np.random.default_rng(9)
    for C in (1, 3):
        cams = [camera_to_gsplat(c, K["fx"], K["fy"], K["cx"], K["cy"], W, H) for c in _view_cams()[:C]]
        tp = {k: _t(P[k]) for k in KEYS}
        aux = ops.RenderAux()
        with torch.no_grad():
            ops.render_views(*(tp[k] for k in KEYS), cams, _t(BG), True, 3, aux)
        radii = aux.radii.reshape(C, N)
        assert int((radii == 0).sum()) > 0 and int((radii > 0).sum()) > 0          # both kinds present
        # forward intermediates the backward reads (conics, rgbs): recompute through the views forward
        f32 = dict(device=DEV, dtype=torch.float32); i32 = dict(device=DEV, dtype=torch.int32)
        xys = torch.empty(C, N, 2, **f32); depths = torch.empty(C, N, **f32); rad = torch.empty(C, N, **i32); conics = torch.empty(C, N, 3, **f32)
        nth = torch.empty(C, N, **i32); rgbs = torch.empty(C, N, 3, **f32); opac = torch.empty(N, **f32)
        CH = ops._cams_host(cams)
        tb = ((W + 15) // 16, (H + 15) // 16)
        st = L.stream_ptr()
        m, ls, q, op = tp["means"], tp["scales"], tp["quats"], tp["opacities"].reshape(-1).contiguous()
        L.check(lib.gc_project_sh_fwd_views(L.i64(N), L.i32(C), L.ptr(m), L.ptr(ls), L.ptr(q), L.ptr(op), L.ptr(tp["features_dc"]),
                                            L.ptr(tp["features_rest"]), L.i32(3), L.i32(3), CH, L.i32(H), L.i32(W), L.i32(tb[0]), L.i32(tb[1]),
                                            L.f32(0.01), L.ptr(xys), L.ptr(depths), L.ptr(rad), L.ptr(conics), L.ptr(nth), L.ptr(rgbs), L.ptr(opac),
                                            None, None, st), "gc_project_sh_fwd_views")
        assert torch.equal(rad, radii)
        v_dep = _t(rng.normal(size=(C, N)).astype(np.float32))
        z2 = torch.zeros(C, N, 2, **f32); z3 = torch.zeros(C, N, 3, **f32); z1 = torch.zeros(C, N, **f32)
        vm = torch.full((N, 3), 7.0, **f32); vls = torch.full((N, 3), 7.0, **f32); vq = torch.full((N, 4), 7.0, **f32)
        vop = torch.full((N,), 7.0, **f32); vdc = torch.full((N, 3), 7.0, **f32); vrest = torch.full((N, 15, 3), 7.0, **f32)
        L.check(lib.gc_project_sh_bwd_depth_views(L.i64(N), L.i32(C), L.i32(0), L.ptr(m), L.ptr(ls), L.ptr(q), L.ptr(op), L.ptr(rgbs), L.i32(3),
                                                  L.i32(3), CH, L.i32(H), L.i32(W), L.ptr(rad), L.ptr(conics), L.ptr(z2), L.ptr(z3), L.ptr(z3),
                                                  L.ptr(z1), L.ptr(vm), L.ptr(vls), L.ptr(vq), L.ptr(vop), L.ptr(vdc), L.ptr(vrest),
                                                  L.ptr(v_dep), st), "gc_project_sh_bwd_depth_views")
        rows = np.stack([np.asarray(c["viewmat"], np.float64).reshape(-1)[8:11] for c in cams])              # [C,3]: row 2 of each view matrix
        vis = (rad > 0).cpu().numpy()
        want = np.einsum("cn,ck->nk", np.where(vis, v_dep.cpu().numpy().astype(np.float64), 0.0), rows)
        got = vm.cpu().numpy().astype(np.float64)
        never = ~vis.any(0)
        assert np.all(got[never] == 0.0)
        within("v_means vs v_depths * viewmat[2, :3], relative", np.abs(got - want).max() / np.abs(want).max(), 1e-6)
        assert float(vls.abs().max()) == 0.0 and float(vq.abs().max()) == 0.0


def test_depth_l1_loss():
    """B = 3, 40 x 24: sentinel pixels in pred, in target and in both, non-finite values, an exact tie, one view without a valid pixel"""
    from gaussctrl_amd.train_ops import depth_l1_loss, depth_l1_loss_views
    g = np.random.default_rng(4)
    B, H, W = 3, 24, 40
    pred = g.uniform(1.0, 6.0, size=(B, H, W)).astype(np.float32)
    target = g.uniform(1.0, 6.0, size=(B, H, W)).astype(np.float32)
    pred[0, :5] = 1000.0; target[0, 3:9] = 1000.0                     # pred only, both (rows 3-4), target only
    pred[0, 10, 0] = np.inf; target[0, 10, 1] = np.nan; pred[0, 10, 2] = target[0, 10, 2]      # non-finite; a tie (sign 0)
    pred[1, :, ::3] = 1000.0
    target[2] = 1000.0                                               # no valid pixel
    p = _t(pred).requires_grad_(True)
    loss = depth_l1_loss_views(p, _t(target))
    w = _t(np.array([0.5, -2.0, 3.0], np.float32))
    (loss * w).sum().backward()
    valid, diff, cnt, want = depth_l1_ref(pred, target)
    got = loss.detach().cpu().numpy().astype(np.float64)
    assert cnt[2] == 0 and got[2] == 0.0
    within("depth L1 loss, relative", np.abs(got - want).max() / np.abs(want).max(), 1e-6)
    inv = (1.0 / np.maximum(cnt, 1)).astype(np.float32)             # the 1 / count factor, one rounding
    wantg = np.sign(diff) * (inv.astype(np.float64) * w.cpu().numpy().astype(np.float64))[:, None, None]
    gotg = p.grad.cpu().numpy().astype(np.float64)
    assert np.all(gotg[~valid] == 0.0) and gotg[0, 10, 2] == 0.0
    ulp = np.spacing(np.abs(wantg).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(gotg - wantg) <= ulp), float(np.abs(gotg - wantg).max())
    # the single-image form is the B = 1 case
    p1 = _t(pred[0]).requires_grad_(True)
    l1 = depth_l1_loss(p1, _t(target[0]))
    l1.backward()
    assert float(l1) == float(loss[0]) and torch.equal(p1.grad * 0.5, p.grad[0])

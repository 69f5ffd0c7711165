"""GPU tests of absgrad densification: RenderAux.absgrad -> gc_rasterize_bwd_abs_views (k_rasterize_bwd<.., true>) -> RenderAux.xys_absgrad,
GaussCtrlModelConfig.use_absgrad -> RefineState.accumulate.

Reference: tests/_absgrad_ref.py, the float64 oracle composited pixel by pixel, sum_p |dL_p/dxy| (its signed sum is the oracle's autograd
gradient to 1e-12: tests/test_absgrad_cpu.py).  Scenes, seeds, cotangents and intrinsics are those of tests/test_raster_depth_gpu.py, chosen
there so that no (pixel, splat) decision sits on a float32 knife edge.

Bars: xys_absgrad under test_raster_gpu._grad_close with scale = max|ref| -- 1e-3 max|ref| + 1e-6 scale on every row, no row beyond it
below 500 k Gaussians; the project's bar for the signed gradient, which the absolute sums (no cancellation) meet more easily.  xys_grad and the
six leaves: the bars of test_depth_grad_single_view / test_depth_grad_views, unchanged.  xys_absgrad >= |xys_grad| elementwise within that
same bar where a reference exists; for the antialiased render (no oracle) within 2 H W 2^-24 |xys_absgrad|: both numbers are float32 sums of
the same <= H W terms, up to sign, added in different orders, and each sum's rounding error is at most H W 2^-24 times the sum of the terms'
magnitudes, which is xys_absgrad itself."""
import numpy as np
import pytest
import torch

from _absgrad_ref import absgrad_reference
from test_raster_depth_gpu import BG, KEYS, _check_grads, _cotangents, _leaves, _oracle_scene, _oracle_view, _render, _scene, _t, _view_cams
from test_raster_gpu import _grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}


def _ref_scene(name):
    if name not in _REF:
        P, c2w, K = _scene(name)
        _REF[name] = absgrad_reference(P, c2w, K, BG, _cotangents(K["H"], K["W"], 7))
    return _REF[name]


def _ref_view(v):
    if ("view", v) not in _REF:
        P, _, K = _scene("a")
        _REF[("view", v)] = absgrad_reference(P, _view_cams()[v], K, BG, _cotangents(K["H"], K["W"], 100 + v))
    return _REF[("view", v)]


def _cam(name):
    from gaussctrl_amd.camera import camera_to_gsplat
    _, c2w, K = _scene(name)
    return camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], K["W"], K["H"])


def _check_abs(got_abs, got_signed, radii, ref_abs):
    """xys_absgrad against the reference, and the two properties of the device result itself"""
    got_abs, got_signed, radii = got_abs.cpu().numpy(), got_signed.cpu().numpy(), radii.cpu().numpy()
    peak = np.abs(ref_abs).max()
    assert peak > 0
    _grad_close(got_abs, ref_abs, peak)
    bar = 1e-3 * peak + 1e-6 * peak
    assert np.all(got_abs >= np.abs(got_signed) - bar)
    assert np.all(got_abs[radii == 0] == 0.0)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_absgrad_single_view_with_depth(name):
    from gaussctrl_amd import gsplat_ops as ops
    P, _, K = _scene(name)
    o, ref = _oracle_scene(name), _ref_scene(name)
    v_rgb, v_a, v_d = (_t(c) for c in _cotangents(K["H"], K["W"], 7))
    tp = _leaves(P)
    aux = ops.RenderAux(); aux.absgrad = True; aux.depth_grad = True
    rgb, alpha, depth = _render(tp, _cam(name), aux)
    assert aux.xys_absgrad is None
    if name == "a":          # several 256-splat staging batches behind one tile, partial tiles on both edges
        bins = aux.tile_bins.cpu().numpy()
        assert (bins[:, 1] - bins[:, 0]).max() > 256 and K["W"] % 16 and K["H"] % 16
        assert bool((aux.radii == 0).any())                              # culled Gaussians: their rows stay exactly 0
    dm = torch.where(depth != 1000.0, depth, torch.zeros_like(depth))
    ((rgb * v_rgb).sum() + (alpha * v_a).sum() + (dm * v_d).sum()).backward()
    assert aux.xys_absgrad.shape == (P["means"].shape[0], 2)
    _check_grads(tp, aux.xys_grad, o["full"])
    _check_abs(aux.xys_absgrad, aux.xys_grad, aux.radii, ref["abs"])
    # not the depth-less sums by another route: the depth term is part of every |dL_p/dxy|
    assert np.abs(ref["abs"] - ref["abs_nodepth"]).max() > 1e-2 * np.abs(ref["abs"]).max()


@pytest.mark.parametrize("name", ["a", "c"])
def test_absgrad_single_view_without_depth(name):
    """want_depth with depth_grad off: the depth image carries no gradient, the entry point runs with the NULL quartet"""
    from gaussctrl_amd import gsplat_ops as ops
    P, _, K = _scene(name)
    o, ref = _oracle_scene(name), _ref_scene(name)
    v_rgb, v_a, _ = (_t(c) for c in _cotangents(K["H"], K["W"], 7))
    tp = _leaves(P)
    aux = ops.RenderAux(); aux.absgrad = True
    rgb, alpha, depth = _render(tp, _cam(name), aux)
    assert depth.requires_grad is False
    ((rgb * v_rgb).sum() + (alpha * v_a).sum()).backward()
    _check_grads(tp, aux.xys_grad, o["nodepth"])
    _check_abs(aux.xys_absgrad, aux.xys_grad, aux.radii, ref["abs_nodepth"])


def test_absgrad_views():
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.camera import camera_to_gsplat
    C = 3
    P, _, K = _scene("a")
    H, W, N = K["H"], K["W"], P["means"].shape[0]
    cams = [camera_to_gsplat(c, K["fx"], K["fy"], K["cx"], K["cy"], W, H) for c in _view_cams()[:C]]
    cots = [tuple(_t(c) for c in _cotangents(H, W, 100 + v)) for v in range(C)]
    v_rgb, v_a, v_d = (torch.stack([c[j] for c in cots]) for j in range(3))
    ref = {k: sum(_oracle_view(v)["full"][k] for v in range(C)) for k in KEYS}
    tp = _leaves(P)
    aux = ops.RenderAux(); aux.absgrad = True; aux.depth_grad = True
    rgb, alpha, depth = ops.render_views(*(tp[k] for k in KEYS), cams, _t(BG), True, 3, aux)
    assert aux.xys_absgrad is None
    ((rgb * v_rgb).sum() + (alpha * v_a).sum() + (torch.where(depth != 1000.0, depth, torch.zeros_like(depth)) * v_d).sum()).backward()
    assert aux.xys_absgrad.shape == (C, N, 2)
    scale = max(np.abs(ref[k]).max() for k in KEYS)
    for k in KEYS:
        _grad_close(tp[k].grad.cpu().numpy(), ref[k], scale)
    for v in range(C):
        _grad_close(aux.xys_grad[v].cpu().numpy(), _oracle_view(v)["full"]["xys"], scale)
        _check_abs(aux.xys_absgrad[v], aux.xys_grad[v], aux.radii[v], _ref_view(v)["abs"])
    # the depth-less form of the batched path (NULL quartet, C = 3)
    tq = _leaves(P)
    aux2 = ops.RenderAux(); aux2.absgrad = True
    rgb2, alpha2, _ = ops.render_views(*(tq[k] for k in KEYS), cams, _t(BG), True, 3, aux2)
    ((rgb2 * v_rgb).sum() + (alpha2 * v_a).sum()).backward()
    for v in range(C):
        _check_abs(aux2.xys_absgrad[v], aux2.xys_grad[v], aux2.radii[v], _ref_view(v)["abs_nodepth"])


def test_absgrad_leaves_the_forward_alone():
    from gaussctrl_amd import gsplat_ops as ops
    P, _, K = _scene("a")
    cam = _cam("a")
    tp = _leaves(P)
    off = ops.RenderAux(); off.depth_grad = True
    on = ops.RenderAux(); on.depth_grad = True; on.absgrad = True
    out_off, out_on = _render(tp, cam, off), _render(tp, cam, on)
    assert all(torch.equal(a, b) for a, b in zip(out_off, out_on))
    assert on.xys_absgrad is None and off.xys_absgrad is None
    out_on[0].sum().backward()
    assert on.xys_absgrad is not None and on.xys_grad is not None
    out_off[0].sum().backward()
    assert off.xys_absgrad is None and off.xys_grad is not None          # a backward without the switch leaves none
    # an aux that is used again: every forward clears the last backward's buffer
    _render(tp, cam, on)
    assert on.xys_absgrad is None and on.xys_grad is None


def test_absgrad_with_antialiased():
    """the projection backward is not involved: the antialiased mode (per-view effective opacities) combines with the switch"""
    from gaussctrl_amd import gsplat_ops as ops
    P, _, K = _scene("a")
    H, W = K["H"], K["W"]
    cam = _cam("a")
    v_rgb, v_a, v_d = (_t(c) for c in _cotangents(H, W, 7))
    res = {}
    for absgrad in (False, True):
        tp = _leaves(P)
        aux = ops.RenderAux(); aux.antialiased = True; aux.depth_grad = True; aux.absgrad = absgrad
        rgb, alpha, depth = _render(tp, cam, aux)
        dm = torch.where(depth != 1000.0, depth, torch.zeros_like(depth))
        ((rgb * v_rgb).sum() + (alpha * v_a).sum() + (dm * v_d).sum()).backward()
        res[absgrad] = (aux, rgb.detach(), tp)
    off, on = res[False][0], res[True][0]
    assert torch.equal(on.compensation, off.compensation) and torch.equal(res[True][1], res[False][1])
    assert off.xys_absgrad is None
    a, s = on.xys_absgrad.double(), on.xys_grad.double()
    assert float(a.max()) > 0
    assert bool((a >= s.abs() - 2 * H * W * 2.0 ** -24 * a).all())
    assert bool((a[on.radii == 0] == 0).all()) and bool((on.radii == 0).any())
    # the switch does not change what the leaves receive: same kernels' sums up to the order of the float atomics
    for k in KEYS:
        g_on, g_off = res[True][2][k].grad.cpu().numpy(), res[False][2][k].grad.cpu().numpy()
        _grad_close(g_on, g_off, max(np.abs(res[False][2][j].grad.cpu().numpy()).max() for j in KEYS))


def test_absgrad_feeds_the_device_refinement():
    """use_absgrad on the stand-alone model: one training step, RefineState.accumulate sums the norm of xys_absgrad, not of xys_grad"""
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.ns_compat import Cameras
    from gaussctrl_amd.refine import RefineState
    EPS = 2.0 ** -24
    P, c2w, K = _scene("a")
    H, W = K["H"], K["W"]
    cams = Cameras(np.asarray(c2w)[None], K["fx"], K["fy"], K["cx"], K["cy"], W, H)
    v_rgb, v_a, _ = (_t(c) for c in _cotangents(H, W, 7))
    cfg = GaussCtrlModelConfig(background_color="black", use_absgrad=True, refine_on_device=True)
    model = GaussCtrlModel(cfg, params={k: v.copy() for k, v in P.items()}, device=DEV)
    model.train()
    out = model.get_outputs(cams[0])
    assert model.xys_absgrad is None
    ((out["rgb"] * v_rgb).sum() + (out["accumulation"][..., 0] * v_a).sum()).backward()
    state = RefineState()
    state.accumulate(model)
    vis = (model.radii > 0).cpu()
    assert int(vis.sum()) > 100
    got = state.grad_norm_sum.cpu().double()
    want = model.xys_absgrad.cpu().double().norm(dim=-1)
    signed = model.xys_grad.cpu().double().norm(dim=-1)
    assert bool(((got - want).abs()[vis] <= 4 * EPS * want[vis]).all())
    assert bool((got[~vis] == 0).all())
    differs = (got - signed).abs()[vis] > 4 * EPS * signed[vis]
    assert float(differs.double().mean()) >= 0.5
    # evaluation renders do not pay for it
    model.eval()
    with torch.no_grad():
        model.get_outputs(cams[0])
    assert model._aux.absgrad is False
    # the switch off: the signed gradient, as before
    model.train()
    model.config.use_absgrad = False
    out = model.get_outputs(cams[0])
    ((out["rgb"] * v_rgb).sum() + (out["accumulation"][..., 0] * v_a).sum()).backward()
    assert model.xys_absgrad is None
    state2 = RefineState()
    state2.accumulate(model)
    signed2 = model.xys_grad.cpu().double().norm(dim=-1)
    assert bool(((state2.grad_norm_sum.cpu().double() - signed2).abs()[vis] <= 4 * EPS * signed2[vis]).all())


def test_mixed_depth_quartet_is_refused():
    """one Gaussian over one 16 x 16 tile, through the C ABI: a quartet with only `extra` set returns GC_EINVAL with a message and writes
    nothing; the same call with the NULL quartet and with the full one runs"""
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    f32 = dict(device=DEV, dtype=torch.float32); i32 = dict(device=DEV, dtype=torch.int32)
    H = W = 16
    ids = torch.zeros(1, **i32); bins = torch.tensor([[0, 1]], **i32)
    xys = torch.tensor([[6.3, 9.1]], **f32); conics = torch.tensor([[0.08, 0.01, 0.05]], **f32)
    colors = torch.tensor([[0.5, 0.4, 0.3]], **f32); opac = torch.tensor([0.6], **f32); bg = torch.zeros(3, **f32)
    fT = torch.full((H, W), 0.5, **f32); fi = torch.zeros(H, W, **i32)
    vo = torch.ones(H, W, 3, **f32); va = torch.ones(H, W, **f32)
    extra = torch.tensor([2.0], **f32); depth = torch.full((H, W), 2.0, **f32); vd = torch.ones(H, W, **f32)

    def call(quartet):
        out = torch.zeros(12, **f32)          # v_xy 2 | v_conic 3 | v_colors 3 | v_opacity 1 | v_extra 1 | v_xy_abs 2
        e, d, g, x = quartet(out)
        rc = lib.gc_rasterize_bwd_abs_views(
            L.i32(1), L.i64(1), L.i64(1), L.i32(1), L.i32(1), L.i32(H), L.i32(W), L.i32(1), L.i32(1), L.ptr(ids), L.ptr(bins), L.ptr(xys),
            L.ptr(conics), L.ptr(colors), L.ptr(opac), L.ptr(bg), L.ptr(fT), L.ptr(fi), L.ptr(vo), L.ptr(va), None, L.ptr(out[0:2]),
            L.ptr(out[2:5]), L.ptr(out[5:8]), L.ptr(out[8:9]), L.ptr(e), L.ptr(d), L.ptr(g), L.ptr(x), L.ptr(out[10:12]), L.stream_ptr())
        torch.cuda.synchronize()
        return rc, out.cpu()

    rc, out = call(lambda out: (extra, None, None, None))
    assert rc == -1                                                         # GC_EINVAL
    msg = lib.gc_last_error_string().decode()
    assert "gc_rasterize_bwd_abs_views" in msg and "extra" in msg
    assert bool((out == 0).all())                                           # nothing was launched
    rc, out = call(lambda out: (extra, depth, vd, None))
    assert rc == -1 and bool((out == 0).all())
    rc, plain = call(lambda out: (None, None, None, None))
    assert rc == 0 and float(plain[9]) == 0.0
    assert bool((plain[10:12] > 0).all()) and bool((plain[10:12] >= plain[0:2].abs()).all())
    rc, full = call(lambda out: (extra, depth, vd, out[9:10]))
    assert rc == 0 and float(full[9]) != 0.0 and bool((full[10:12] > 0).all())

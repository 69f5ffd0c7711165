"""GPU: the distortion map (include/ext/gaussctrl_distort.h) -- k_distort_fwd / k_distort_bwd alone on the crafted tile lists of
tests/_composite_scene.py against the float64 closed form of tests/_distort_ref.py (row metric and bars formed on the CPU from the
reference's own float32-vs-float64 distance; tests/test_distort_cpu.py), the wiring through render_view / render_views, and the model's
switch.

The kernel and ops-level cases run inside _redzone.guard: inputs go through on_device, outputs start zero (or seeded) where the ABI adds
into them and NaN otherwise and must be finite afterwards; the capacity padding of ids_sorted is 0."""
import sys

import numpy as np
import pytest
import torch

import _composite_scene as cs
import _distort_ref as dr
from _margins import within
from _redzone import guard, on_device
from gaussctrl_amd import _lib as L
from gaussctrl_amd import gsplat_ops as ops
from gaussctrl_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = np.float64
PAD = 37
KEYS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
NEAR, FAR = float(dr.NEAR), float(dr.FAR)


def _d(a):
    return on_device(torch.from_numpy(np.ascontiguousarray(a)), DEV)


def _h(t):
    return t.detach().cpu().numpy()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _guarded(fn, *args, nbytes=64 << 20, **kw):
    with guard(ops, sys.modules[__name__], nbytes=nbytes):
        return fn(*args, **kw)


# ---------------------------------------------------------------------------------------- the kernels alone
class Lists:
    """the device arrays of V views of one crafted scene ([V][N][..], ids_sorted [V][M + pad] zero-padded) and what gc_rasterize_fwd_views
    leaves on them; opacities are view 0's when shared"""

    def __init__(self, name, V, shared):
        self.scs = [cs.scene(name, v, not shared) for v in range(V)]
        s0 = self.scs[0]
        self.V, self.N, self.H, self.W, self.shared = V, s0["N"], s0["H"], s0["W"], int(shared)
        self.tx, self.ty = s0["tiles"]
        M = len(s0["ids_sorted"])
        self.M_cap = M + (PAD if V > 1 else 0)
        ids = np.zeros((V, self.M_cap), np.int32)
        for v, sc in enumerate(self.scs):
            ids[v, :M] = sc["ids_sorted"]
        stack = lambda k: _d(np.stack([sc[k] for sc in self.scs]))
        self.ids, self.bins, self.xys, self.conics, self.depths = _d(ids), stack("tile_bins"), stack("xys"), stack("conics"), stack("extra")
        self.opac = _d(s0["opac"]) if shared else stack("opac")
        colors, bg = stack("colors"), _d(s0["background"])
        self.fT = _nan(V, self.H, self.W)
        self.fi = torch.full((V, self.H, self.W), -7, dtype=torch.int32, device=DEV)
        img = _nan(V, self.H, self.W, 3)
        L.call("gc_rasterize_fwd_views", V, self.N, self.M_cap, self.shared, 1, self.H, self.W, self.tx, self.ty, self.ids, self.bins, self.xys,
               self.conics, colors, self.opac, None, bg, img, None, self.fT, self.fi)
        torch.cuda.synchronize()
        for v, sc in enumerate(self.scs):          # the lists the distortion kernels walk are the ones the forward just walked, decision for decision
            assert np.array_equal(_h(self.fi[v]), cs.forward(sc, F64)["final_index"]), f"{name} view {v}: final_index differs from the float64 reference"

    def head(self):
        return (self.V, self.N, self.M_cap, self.shared, self.H, self.W, self.tx, self.ty, self.ids, self.bins, self.xys, self.conics, self.opac,
                self.depths)


def _kernel_case(name, V, shared):
    ls = Lists(name, V, shared)
    label = f"{name} V={V} shared={shared}"
    for mode in dr.MODES:
        dist, wt = _nan(V, ls.H, ls.W), _nan(V, ls.H, ls.W)
        L.call("gcx_distort_fwd_views", *ls.head(), mode, NEAR, FAR, dist, wt)
        torch.cuda.synchronize()
        for v, sc in enumerate(ls.scs):
            for k, e in dr.forward_errors(dict(distort=_h(dist[v]), wt=_h(wt[v])), dr.forward(sc, mode)).items():
                within(f"{label} map {mode} view {v}: forward {k}", e, dr.FWD_BARS[k])
        for cset, prefill in (("a", False), ("b", True)):
            refs = [dr.reference(sc, cset, mode) for sc in ls.scs]
            g = np.random.default_rng(4242 + mode)
            init = {}
            for k, w in dr.WIDTH.items():
                # prefill: 0.1 of the row's term-wise sum A times a normal draw; a row no term reaches gets a plain draw and must come back bit for bit
                A = np.stack([r[k][1] for r in refs])
                an = np.linalg.norm(A, axis=2, keepdims=True)
                init[k] = (g.normal(size=A.shape) * np.where(an > 0, 0.1 * an, 1.0)).astype(np.float32) if prefill else np.zeros(A.shape, np.float32)
            out = {k: _d(x) for k, x in init.items()}
            v_dist = _d(np.stack([dr.cotangent(sc, cset) for sc in ls.scs]))
            L.call("gcx_distort_bwd_views", *ls.head(), mode, NEAR, FAR, ls.fT, ls.fi, wt, v_dist, out["v_xy"], out["v_conic"], out["v_opacity"],
                   out["v_depths"])
            torch.cuda.synchronize()
            for v, ref in enumerate(refs):
                for k in dr.KEYS:
                    got, x = np.asarray(_h(out[k][v]), F64), np.asarray(init[k][v], F64)
                    assert np.isfinite(got).all(), (label, k)
                    slack = 2.0 ** -23 * np.linalg.norm(x.reshape(x.shape[0], -1), axis=1) if prefill else None
                    worst, n = cs.row_errors((got - x).reshape(ref[k][0].shape), ref[k][0], ref[k][1], slack)
                    within(f"{label} map {mode} set {cset} prefill={prefill} view {v}: {k} worst row error ({n} rows)", worst, dr.BARS[k])


@pytest.mark.parametrize("V,shared", [(1, True), (2, True), (2, False)])
@pytest.mark.parametrize("name", cs.SCENES)
def test_kernels_on_crafted_lists(name, V, shared):
    """tiny: the staging tails; deep: one to three backward batches and both sides of each batch edge; stop: early stops; opaque: the cap and
    ra up to 1000.  Both depth maps; set a into zeroed gradient arrays, set b into seeded ones (the call ADDS)"""
    _guarded(_kernel_case, name, V, shared)


def test_empty_scene_zeroes_the_maps():
    def body():
        dist, wt = _nan(2, 9, 17), _nan(2, 9, 17)
        L.call("gcx_distort_fwd_views", 2, 0, 0, 1, 9, 17, 2, 1, None, None, None, None, None, None, 0, NEAR, FAR, dist, wt)
        torch.cuda.synchronize()
        assert bool((dist == 0).all()) and bool((wt == 0).all())
    _guarded(body)


# ---------------------------------------------------------------------------------------- wiring
W_, H_ = 64, 48
INTR = dict(fx=60.0, fy=59.4, cx=W_ / 2 + 1.3, cy=H_ / 2 - 2.1)
BG = np.array([0.1, 0.2, 0.3], np.float32)
# |autograd - by hand| <= WIRE_BAR x the tensor's largest entry: both routes run the same launches on the same bits, so they differ only in
# the order of the float atomics (a few partial sums per (tile, splat), four waves per tile); no term-wise sums exist at this level, so the
# scale is the tensor's own and the bar the largest of the compositing bars
WIRE_BAR = max(cs.BARS.values())


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _scene():
    from gaussctrl_amd.camera import camera_to_gsplat
    P = syn.make_gaussians(3000, seed=4, scale_mean=0.05)
    cams = [camera_to_gsplat(c, INTR["fx"], INTR["fy"], INTR["cx"], INTR["cy"], W_, H_) for c in syn.make_cameras(2, seed=12)]
    return P, cams


def _leaves(P):
    return {k: _t(P[k]).requires_grad_(True) for k in KEYS}


def _by_hand(tp, cams, g, mode):
    """the distortion map and the six leaf gradients of (g * map).sum(), entry point by entry point: the front half of render_views, the
    compositing forward, the two distortion entry points on zeroed arrays, and the depth form of the projection backward"""
    with torch.no_grad():
        fr = ops._views_front(*(tp[k] for k in KEYS), cams, 3, None)
        C, N, H, W, tb = fr.C, fr.N, fr.H, fr.W, fr.tb
        m, ls, q, op, dc, rest = fr.leaves
        img, fT = torch.empty(C, H, W, 3, device=DEV), torch.empty(C, H, W, device=DEV)
        fi = torch.empty(C, H, W, dtype=torch.int32, device=DEV)
        L.call("gc_rasterize_fwd_views", C, N, fr.M_cap, fr.shared_op, 1, H, W, tb[0], tb[1], fr.ids_s, fr.bins, fr.xys, fr.conics, fr.rgbs, fr.opac,
               None, _t(BG), img, None, fT, fi)
        head = (C, N, fr.M_cap, fr.shared_op, H, W, tb[0], tb[1], fr.ids_s, fr.bins, fr.xys, fr.conics, fr.opac, fr.depths, mode, NEAR, FAR)
        dist, wt = torch.empty(C, H, W, device=DEV), torch.empty(C, H, W, device=DEV)
        L.call("gcx_distort_fwd_views", *head, dist, wt)
        v_xy, v_conic, v_col = torch.zeros(C, N, 2, device=DEV), torch.zeros(C, N, 3, device=DEV), torch.zeros(C, N, 3, device=DEV)
        v_op, v_ex = torch.zeros(C, N, device=DEV), torch.zeros(C, N, device=DEV)
        L.call("gcx_distort_bwd_views", *head, fT, fi, wt, g.reshape(C, H, W).contiguous(), v_xy, v_conic, v_op, v_ex)
        assert float(v_ex.abs().max()) > 0 and float(v_xy.abs().max()) > 0
        vm, vls, vq, vop = torch.zeros_like(m), torch.zeros_like(ls), torch.zeros_like(q), torch.zeros(N, device=DEV)
        vdc, vrest = torch.zeros_like(dc), torch.zeros_like(rest)
        L.call("gc_project_sh_bwd_depth_views", N, C, 0, m, ls, q, op, fr.rgbs, fr.sh_degree, 3, fr.CH, H, W, fr.radii, fr.conics, v_xy, v_conic, v_col,
               v_op, vm, vls, vq, vop, vdc, vrest, v_ex)
        torch.cuda.synchronize()
    return dist, dict(zip(KEYS, (vm, vls, vq, vop[:, None], vdc, vrest))), v_xy


def _close(label, got, want):
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(got).all()), label
    within(label, float((got - want).abs().max()), WIRE_BAR * float(want.abs().max()))


def _wiring_case(views, mode_name, into):
    P, cams = _scene()
    cams = cams if views else cams[:1]
    mode = ops.distort_depth_mode(mode_name)
    g = _t(np.random.default_rng(31).normal(size=(len(cams), H_, W_)) if views else np.random.default_rng(31).normal(size=(H_, W_)))
    hand_map, hand, hand_xy = _by_hand(_leaves(P), cams, g, mode)
    tp = _leaves(P)
    aux = ops.RenderAux()
    aux.distort, aux.distort_depth_map, aux.distort_near, aux.distort_far = True, mode_name, NEAR, FAR
    if into:
        aux.grad_into = {k: torch.zeros(tp[k].shape[:1] if k == "opacities" else tp[k].shape, device=DEV) for k in KEYS}
    args = tuple(tp[k] for k in KEYS)
    out = ops.render_views(*args, cams, _t(BG), True, 3, aux) if views else ops.render_view(*args, cams[0], _t(BG), True, 3, aux)
    assert len(out) == 3                                               # the signatures and return values stay
    dmap = aux.distort_map
    assert dmap is not None and dmap.requires_grad and tuple(dmap.shape) == ((len(cams), H_, W_) if views else (H_, W_))
    assert torch.equal(dmap.detach().reshape(hand_map.shape), hand_map) and float(dmap.detach().max()) > 0
    # the switch leaves the other outputs alone, bit for bit
    off = ops.RenderAux()
    with torch.no_grad():
        ref = ops.render_views(*args, cams, _t(BG), True, 3, off) if views else ops.render_view(*args, cams[0], _t(BG), True, 3, off)
    assert off.distort_map is None and all(torch.equal(a.detach(), b) for a, b in zip(out, ref))
    (g * dmap).sum().backward()
    label = f"{'render_views' if views else 'render_view'} {mode_name} into={into}"
    for k in KEYS:
        if into:
            assert tp[k].grad is None
            got = aux.grad_into[k].reshape(hand[k].shape)
        else:
            got = tp[k].grad
        _close(f"{label}: {k}", got, hand[k])
    for k in ("means", "scales", "opacities"):
        assert float(hand[k].abs().max()) > 0
    for k in ("features_dc", "features_rest"):                          # nothing goes to colours
        assert float(hand[k].abs().max()) == 0
    _close(f"{label}: xys_grad", aux.xys_grad.reshape(hand_xy.shape), hand_xy)          # includes the distortion's pull
    assert aux.xys_absgrad is None


@pytest.mark.parametrize("into", [False, True])
@pytest.mark.parametrize("views,mode_name", [(False, "linear"), (True, "ndc"), (True, "linear"), (False, "ndc")])
def test_autograd_equals_the_entry_points_by_hand(views, mode_name, into):
    _guarded(_wiring_case, views, mode_name, into, nbytes=256 << 20)


class _Recording:
    """stands at `_lib._lib` and remembers which entry points are looked up, in order"""

    def __init__(self, real):
        self.__dict__["_real"], self.__dict__["names"] = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._real, name)


# what one training render_view and its backward look up today (tight boxes, exact list sizes)
OFF_CALLS = ["gc_project_sh_fwd_boxes", "gc_raster_depth_order_workspace_bytes", "gc_raster_depth_order", "gc_raster_read_count",
             "gc_raster_bin_workspace_bytes", "gc_raster_bin_tiles_boxes", "gc_rasterize_fwd", "gc_raster_finalize_into",
             "gc_rasterize_bwd_views", "gc_project_sh_bwd"]


def _record(switch, use_map):
    P, cams = _scene()
    tp = _leaves(P)
    aux = ops.RenderAux()
    aux.distort = switch
    real = L.lib()
    rec = _Recording(real)
    L._lib = rec
    try:
        rgb, alpha, _ = ops.render_view(*(tp[k] for k in KEYS), cams[0], _t(BG), False, 3, aux)
        loss = rgb.sum() + alpha.sum()
        if use_map:
            loss = loss + aux.distort_map.sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        L._lib = real
    return rec.names, aux


def test_switch_off_launches_what_it_always_did():
    names, aux = _record(False, False)
    assert names == OFF_CALLS and aux.distort_map is None
    assert not [n for n in names if n.startswith("gcx_distort")]
    # on, the map unused: the forward pays for the map, the backward is the plain one
    names, aux = _record(True, False)
    assert names == OFF_CALLS[:8] + ["gcx_distort_fwd_views"] + OFF_CALLS[8:] and aux.distort_map is not None
    # on and used: the distortion backward between the compositing and the projection backward, which takes its depth form
    names, _ = _record(True, True)
    assert names == OFF_CALLS[:8] + ["gcx_distort_fwd_views", "gc_rasterize_bwd_views", "gcx_distort_bwd_views", "gc_project_sh_bwd_depth_views"]
    # no gradient asked for: no map, nothing launched for it
    P, cams = _scene()
    aux = ops.RenderAux()
    aux.distort = True
    with torch.no_grad():
        ops.render_view(*(_t(P[k]) for k in KEYS), cams[0], _t(BG), False, 3, aux)
    assert aux.distort_map is None


# ---------------------------------------------------------------------------------------- the model
def _model(P, **cfg):
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    return GaussCtrlModel(GaussCtrlModelConfig(background_color="black", **cfg), params={k: v.copy() for k, v in P.items()}, device=DEV)


def _camera(c2w):
    from gaussctrl_amd.ns_compat import Cameras
    return Cameras(np.asarray(c2w, np.float32)[None], INTR["fx"], INTR["fy"], INTR["cx"], INTR["cy"], W_, H_)[0]


@pytest.mark.parametrize("mode_name", ops.DISTORT_DEPTH_MAPS)
def test_model_outputs_loss_and_gradients(mode_name):
    P = syn.make_gaussians(3000, seed=4, scale_mean=0.05)
    cam = _camera(syn.make_cameras(1, seed=12)[0])
    mult = 0.25
    model = _model(P, distortion_loss_mult=mult, distortion_depth_map=mode_name)
    model.train()
    out = model.get_outputs(cam)
    assert tuple(out["distortion"].shape) == (H_, W_, 1) and float(out["distortion"].max()) > 0
    batch = {"image": torch.zeros(H_, W_, 3, device=DEV)}
    loss = model.get_loss_dict(out, batch)
    assert torch.equal(loss["distortion_loss"], mult * out["distortion"].mean())
    metrics = model.get_metrics_dict(out, batch)
    assert torch.equal(metrics["distortion"], out["distortion"].detach().mean()) and not metrics["distortion"].requires_grad
    loss["distortion_loss"].backward()                                  # that term alone
    for k in ("means", "opacities", "scales"):
        grad = getattr(model, k).grad
        assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0, k
    # evaluation and the camera renders never compute it
    model.eval()
    with torch.no_grad():
        ev = model.get_outputs(cam)
    assert "distortion" not in ev and model._aux.distort is False and "distortion_loss" not in model.get_loss_dict(ev, batch)
    assert "distortion" not in model.get_metrics_dict(ev, batch)
    model.train()
    assert "distortion" not in model.get_outputs_for_camera(cam) and model._aux.distort is False


def test_model_switch_off_has_no_key_and_no_launch():
    P = syn.make_gaussians(3000, seed=4, scale_mean=0.05)
    cam = _camera(syn.make_cameras(1, seed=12)[0])
    model = _model(P)
    model.train()
    real = L.lib()
    rec = _Recording(real)
    L._lib = rec
    try:
        out = model.get_outputs(cam)
        batch = {"image": torch.zeros(H_, W_, 3, device=DEV)}
        loss = model.get_loss_dict(out, batch)
        sum(loss.values()).backward()
        torch.cuda.synchronize()
    finally:
        L._lib = real
    assert "distortion" not in out and "distortion_loss" not in loss and "distortion" not in model.get_metrics_dict(out, batch)
    assert not [n for n in rec.names if n.startswith("gcx_distort")]
    assert [n for n in rec.names if n.startswith(("gc_project", "gc_raster"))] == OFF_CALLS


def _looking_away():
    """300 Gaussians behind a camera at (0, 0, 3) that looks at the origin: the view sees none, its lists are empty (M == 0)"""
    P = syn.make_gaussians(300, seed=8, scale_mean=0.05)
    P["means"] = (P["means"] * 0.5 + np.array([0.0, 0.0, 5.5], np.float32)).astype(np.float32)
    return P, syn.look_at_c2w(np.array([0.0, 0.0, 3.0]), np.zeros(3), up=(0.0, 1.0, 0.0))


def test_view_that_sees_nothing_through_the_operator():
    """render_view with the switch on and empty lists (ids_sorted has no element, hence no address): no exception, a zero map, no distortion
    launch, and a backward through the map that leaves zero gradients"""
    from gaussctrl_amd.camera import camera_to_gsplat
    P, c2w = _looking_away()
    cam = camera_to_gsplat(c2w, INTR["fx"], INTR["fy"], INTR["cx"], INTR["cy"], W_, H_)
    tp = _leaves(P)
    aux = ops.RenderAux()
    aux.distort = True
    real = L.lib()
    rec = _Recording(real)
    L._lib = rec
    try:
        rgb, alpha, _ = ops.render_view(*(tp[k] for k in KEYS), cam, _t(BG), False, 3, aux)
        assert aux.M == 0 and aux.gaussian_ids_sorted.numel() == 0
        dmap = aux.distort_map
        assert tuple(dmap.shape) == (H_, W_) and bool((dmap == 0).all()) and bool((alpha == 0).all())
        (dmap.sum() + rgb.sum()).backward()
        torch.cuda.synchronize()
    finally:
        L._lib = real
    assert not [n for n in rec.names if n.startswith("gcx_distort")]
    for k in KEYS:
        assert tp[k].grad is not None and bool((tp[k].grad == 0).all()), k


def test_model_view_that_sees_nothing_takes_the_early_return():
    """training mode, mult > 0, every Gaussian behind the camera: {"rgb": background}, no key, no loss term, no exception"""
    P, c2w = _looking_away()
    model = _model(P, distortion_loss_mult=0.5)
    model.train()
    out = model.get_outputs(_camera(c2w))
    assert set(out) == {"rgb"} and tuple(out["rgb"].shape) == (H_, W_, 3) and bool((out["rgb"] == 0).all())          # background "black"
    batch = {"image": torch.zeros(H_, W_, 3, device=DEV)}
    assert "distortion_loss" not in model.get_loss_dict(out, batch) and "distortion" not in model.get_metrics_dict(out, batch)


def test_twenty_adam_steps_on_the_term_alone_lower_it():
    """a sheet of 14 x 14 splats in the plane z = 0 seen from (0, 0, 3), and eight translucent ones halfway to the camera: floaters.  Adam on
    means, scales, quats and opacities with the distortion term as the whole loss: after 20 steps the mean of the map is below where it began"""
    g = np.random.default_rng(5)
    u = np.linspace(-1.0, 1.0, 14)
    sheet = np.stack([*np.meshgrid(u, u, indexing="ij"), np.zeros((14, 14))], -1).reshape(-1, 3)
    floaters = np.concatenate([g.uniform(-0.5, 0.5, (8, 2)), np.full((8, 1), 1.5)], 1)
    n = len(sheet) + len(floaters)
    P = syn.make_gaussians(n, seed=6)
    P["means"] = np.concatenate([sheet, floaters]).astype(np.float32)
    P["scales"] = np.log(np.concatenate([np.full((len(sheet), 3), 0.12), np.full((len(floaters), 3), 0.15)])).astype(np.float32)
    P["opacities"] = np.concatenate([np.full((len(sheet), 1), 2.0), np.full((len(floaters), 1), -1.0)]).astype(np.float32)
    cam = _camera(syn.look_at_c2w(np.array([0.0, 0.0, 3.0]), np.zeros(3), up=(0.0, 1.0, 0.0)))
    model = _model(P, distortion_loss_mult=1.0)
    model.train()
    opt = torch.optim.Adam([model.means, model.scales, model.quats, model.opacities], lr=1e-2)
    batch = {"image": torch.zeros(H_, W_, 3, device=DEV)}
    history = []
    for _ in range(21):
        opt.zero_grad(set_to_none=True)
        out = model.get_outputs(cam)
        loss = model.get_loss_dict(out, batch)["distortion_loss"]
        history.append(float(loss))
        loss.backward()
        opt.step()
    print("mean distortion, step 0 / 20:", history[0], history[-1])
    assert history[0] > 1e-4 and np.isfinite(history).all()
    assert history[-1] < history[0]

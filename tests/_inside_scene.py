"""Scenes with the camera INSIDE the cloud, and a float64 reference of the per-Gaussian front end alone (plain helper, like _margins.py).

syn.make_gaussians puts the means in [-1, 1]^3 and syn.make_cameras its cameras on the 2-3 shell: nothing is ever behind a camera, close to
it or around it, and the frustum clamp of the projection (lim = 1.3 * half-fov) fires on a handful of rows.  Real captures have the camera
inside the cloud.  Here the same generators with make_cameras(..., rmin=0.3, rmax=0.6):

    in3, in7   N = 3000, 96 x 64, fx 80, scale_mean 0.05, seeds 3 / 7 (camera seed + 1)
    tiny       N = 299, 33 x 17, fx 40, scale_mean 0.3, seed 5: one full workgroup and one of 43 records (the scalar tails of the 16-byte
               staging loops of raster_project.hip run)
    views9     in3's Gaussians under make_cameras(9, seed=VIEWS9_CAM_SEED, rmin=0.3, rmax=0.6): crosses the 8-views-per-launch split

In every scene 200 seeded rows get features_dc -= 2.5, so that clamp(SH + 0.5, min 0) masks many channels; intrinsics follow
test_raster_gpu._scene (fy = 0.99 fx, cx = W / 2 + 1.3, cy = H / 2 - 2.1).  tests/test_project_vjp_cpu.py holds the census of every scene.

front_ref is the front end of oracle.raster_torch.get_outputs restated from the oracle's own pieces; its autograd in float64 is the reference
of the VJPs of raster_project.hip (project_one_bwd / geom_vjp / colour_vjp) in tests/test_project_vjp_gpu.py.

Row metric: e_row = |got - ref|_2 / (|ref_row|_2 + floor_row).  floor_row is 0 except for the quaternions, where it is the norm of the same
Gaussian's reference log-scale gradient: both come from the same vM, and a nearly isotropic Gaussian's quaternion gradient cancels to about
0 (unfloored, the float32 reference itself is off by 1e8 of such a row).  For a sum over views |ref_row| is the sum of the per-view row
norms (the views are added in float32).  A row whose denominator is 0 (culled in every view, or no cotangent reaches the tensor) must be
exactly 0 on both sides.

BARS: one constant per leaf tensor = 4 x the worst e_row between the float32 and the float64 front_ref over all scenes, views, n_use values
and cotangent sets with aa off (the device's operation order differs from torch's, hence the 4).  Measured (test_project_vjp_cpu.
test_bars_are_four_times_the_reference_distance asserts bar / 8 <= measured <= bar / 3 for each):

    means 1.16e-4   log-scales 8.24e-6   quaternions (floored) 2.75e-6   opacity logits 3.12e-5   features_dc 1.93e-7   features_rest 3.09e-7

(the means figure is the conic-only set's, where the mean's gradient is the frustum path alone and cancels on a few large Gaussians; 99 % of
its rows are below 2.1e-6).  The antialiased runs use the same bars.  Both precisions are handed the float32 camera matrices the kernels get.
"""
import contextlib

import numpy as np
import torch

from _margins import within
from gaussctrl_amd import synthetic as syn

KEYS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
OUTS = ("xys", "depths", "conics", "rgbs", "opac")
SCENES = {"in3": dict(N=3000, W=96, H=64, fx=80.0, sm=0.05, seed=3),
          "in7": dict(N=3000, W=96, H=64, fx=80.0, sm=0.05, seed=7),
          "tiny": dict(N=299, W=33, H=17, fx=40.0, sm=0.3, seed=5),
          "views9": dict(N=3000, W=96, H=64, fx=80.0, sm=0.05, seed=3, views=9)}
VIEWS9_CAM_SEED = 4          # view 0 is in3's own camera
RENDER_VIEWS = (1, 2, 3)          # the views of views9 that the whole-render test uses
DARK_ROWS = 200
BARS = {"means": 4.6e-4, "scales": 3.3e-5, "quats": 1.1e-5, "opacities": 1.25e-4, "features_dc": 7.7e-7, "features_rest": 1.24e-6}
# every (sh_degree, sh_degree_to_use) pair the GPU tests run: each K instantiation, and each colour path of K = 16
SH_MODES = ((3, -1), (3, 0), (3, 1), (3, 2), (3, 3), (0, 0), (1, 1), (2, 2))
_CACHE = {}


def intrinsics(s):
    return dict(fx=s["fx"], fy=s["fx"] * 0.99, cx=s["W"] / 2 + 1.3, cy=s["H"] / 2 - 2.1, W=s["W"], H=s["H"])


def scene(name):
    """(parameters with sh_degree 3, camera-to-world matrices [C, 3, 4], intrinsics); cached: do not write to the arrays"""
    if ("scene", name) not in _CACHE:
        s = SCENES[name]
        P = syn.make_gaussians(s["N"], seed=s["seed"], scale_mean=s["sm"])
        dark = np.random.default_rng(s["seed"] + 100).choice(s["N"], DARK_ROWS, replace=False)
        P["features_dc"][dark] -= np.float32(2.5)
        if "views" in s:
            c2ws = syn.make_cameras(s["views"], seed=VIEWS9_CAM_SEED, rmin=0.3, rmax=0.6)
        else:
            c2ws = syn.make_cameras(1, seed=s["seed"] + 1, rmin=0.3, rmax=0.6)
        _CACHE[("scene", name)] = (P, c2ws, intrinsics(s))
    return _CACHE[("scene", name)]


def with_degree(P, deg):
    """the scene with features_rest cut to the (deg + 1)^2 - 1 bases of sh_degree = deg"""
    return dict(P, features_rest=np.ascontiguousarray(P["features_rest"][:, :(deg + 1) ** 2 - 1]))


def _rho(rt, means, scales, quats, viewmat, K, radii):
    """The compensation, from a restatement of the 2 x 2 covariance of rt.project_gaussians (its lines between `W3 = ...` and `cov = ...`,
    before the + 0.3); 0 where the projection culls (radii == 0).  The square root is only taken where its argument is positive (autograd)."""
    W3 = viewmat[:3, :3]
    t = means @ W3.T + viewmat[:3, 3]
    keep = t[:, 2] > 0.01
    tz = torch.where(keep, t[:, 2], torch.ones_like(t[:, 2]))
    M = rt.quat_to_rotmat(quats) * scales[:, None, :]
    Sigma = M @ M.transpose(1, 2)
    txc = tz * torch.clamp(t[:, 0] / tz, -1.3 * (0.5 * K["W"] / K["fx"]), 1.3 * (0.5 * K["W"] / K["fx"]))
    tyc = tz * torch.clamp(t[:, 1] / tz, -1.3 * (0.5 * K["H"] / K["fy"]), 1.3 * (0.5 * K["H"] / K["fy"]))
    rz = 1.0 / tz
    zero = torch.zeros_like(rz)
    J = torch.stack([K["fx"] * rz, zero, -K["fx"] * txc * rz * rz, zero, K["fy"] * rz, -K["fy"] * tyc * rz * rz], -1).reshape(-1, 2, 3)
    Tm = J @ W3
    cov = Tm @ Sigma @ Tm.transpose(1, 2)
    a0, b, d0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    ratio = (a0 * d0 - b * b) / ((a0 + 0.3) * (d0 + 0.3) - b * b)
    ok = keep & (radii > 0) & (ratio > 0)
    return torch.where(ok, torch.sqrt(torch.where(ok, ratio, torch.ones_like(ratio))), torch.zeros_like(ratio))


class _StraightThroughTorch:
    """`torch` for oracle.raster_torch while the sensitivity check runs: clamp(x, lo, hi) keeps its value and passes the gradient of x
    through unchanged -- what a wrong clx / cly routing at the end of project_one_bwd would compute.  (rt.project_gaussians calls the
    two-bound form for the frustum clamp, and for the integer tile boxes, which carry no gradient; clamp(x, min=...) is left alone.)"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def clamp(x, *bounds, **kw):
        y = torch.clamp(x, *bounds, **kw)
        return x + (y - x).detach() if len(bounds) == 2 and x.requires_grad else y


@contextlib.contextmanager
def _straight_through_clamp(rt):
    real = rt.torch
    rt.torch = _StraightThroughTorch()
    try:
        yield
    finally:
        rt.torch = real


def front_ref(P, c2w, K, deg, n_use, aa, cotangents, dtype, straight_through=False):
    """The front end of rt.get_outputs for one camera: exp(scales), q / |q|, rt.project_gaussians, detached view directions,
    rt.spherical_harmonics(n_use) + 0.5 clamped at 0 (n_use = -1: sigmoid(features_dc)), sigmoid(opacity) -- times the rho of _rho with aa.
    As in the fused kernels, a Gaussian the view culls (radii == 0) has zero colour and its opacity takes no cotangent ("opac" is
    sigmoid * [radii > 0]; "opac_all" the unmasked value the classic forward stores).

    cotangents: {name in OUTS: array shaped like that output} (a missing name is a zero cotangent) or None for the forward alone.
    Returns (out, grads): out = numpy arrays xys, depths, conics, rgbs, opac, opac_all, radii, num_tiles_hit, t (camera-space means)
    [, rho]; grads = {leaf: d sum(out * cotangent) / d leaf} by autograd (zeros where nothing reaches a leaf), or None."""
    from oracle import raster_c, raster_torch as rt
    p = {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for k, v in with_degree(P, deg).items()}
    W, H = K["W"], K["H"]
    c2w_t = torch.tensor(np.asarray(c2w))
    # the camera the kernels are handed: the float32 matrices of the oracle's numpy glue (the product's camera_to_gsplat bit for bit,
    # test_project_vjp_cpu.py), in both precisions, so that the reference differs from the device in its arithmetic alone, not in its inputs
    viewmat, full = (torch.tensor(m, dtype=dtype) for m in raster_c.camera_glue(c2w, K["fx"], K["fy"], W, H))
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    scales = torch.exp(p["scales"])
    quats = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
    with (_straight_through_clamp(rt) if straight_through else contextlib.nullcontext()):
        xys, depths, radii, conics, nth, _ = rt.project_gaussians(p["means"], scales, 1.0, quats, viewmat[:3, :], full, K["fx"], K["fy"],
                                                                  K["cx"], K["cy"], H, W, tb)
    keep = (radii > 0).to(dtype)
    viewdirs = p["means"].detach() - c2w_t[:3, 3].to(dtype)
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    if n_use < 0:
        rgbs = torch.sigmoid(p["features_dc"])
    else:
        colors = torch.cat([p["features_dc"][:, None, :], p["features_rest"]], 1)
        rgbs = torch.clamp(rt.spherical_harmonics(n_use, viewdirs, colors) + 0.5, min=0.0)
    rgbs = rgbs * keep[:, None]
    opac_all = torch.sigmoid(p["opacities"])[:, 0]
    o = dict(xys=xys, depths=depths, conics=conics, rgbs=rgbs, opac_all=opac_all)
    if aa:
        o["rho"] = _rho(rt, p["means"], scales, quats, viewmat[:3, :], K, radii)
        o["opac"] = opac_all * o["rho"]
    else:
        o["opac"] = opac_all * keep
    grads = None
    if cotangents is not None:
        loss = sum((o[k] * torch.tensor(np.asarray(v), dtype=dtype)).sum() for k, v in cotangents.items())
        gs = torch.autograd.grad(loss, [p[k] for k in KEYS], allow_unused=True)
        grads = {k: (np.zeros(p[k].shape) if g is None else g.numpy().astype(np.float64)) for k, g in zip(KEYS, gs)}
    out = {k: v.detach().numpy() for k, v in o.items()}
    with torch.no_grad():
        out["t"] = (p["means"] @ viewmat[:3, :3].T + viewmat[:3, 3]).numpy()
    out["radii"], out["num_tiles_hit"] = radii.numpy(), nth.numpy()
    return out, grads


def census(name):
    """Per view of the scene, in float64: who is where.  clamp_x / clamp_y: (rows clamped at -lim, at +lim) among the visible ones."""
    if ("census", name) not in _CACHE:
        P, c2ws, K = scene(name)
        lim_x, lim_y = 1.3 * (0.5 * K["W"] / K["fx"]), 1.3 * (0.5 * K["H"] / K["fy"])
        tiles = ((K["W"] + 15) // 16) * ((K["H"] + 15) // 16)
        rows = []
        for c2w in c2ws:
            o, _ = front_ref(P, c2w, K, 3, 3, False, None, torch.float64)
            vis = o["radii"] > 0
            tz = o["t"][:, 2]
            safe = np.where(tz > 0.01, tz, 1.0)
            rx, ry = o["t"][:, 0] / safe, o["t"][:, 1] / safe
            rows.append(dict(visible=int(vis.sum()),
                             clamp_x=(int((vis & (rx < -lim_x)).sum()), int((vis & (rx > lim_x)).sum())),
                             clamp_y=(int((vis & (ry < -lim_y)).sum()), int((vis & (ry > lim_y)).sum())),
                             clamp_both=int((vis & (np.abs(rx) > lim_x) & (np.abs(ry) > lim_y)).sum()),
                             behind=int((tz <= 0.01).sum()), near=int((vis & (tz < 0.2)).sum()),
                             full_boxes=int((vis & (o["num_tiles_hit"] == tiles)).sum()),
                             dark_channels=int((vis[:, None] & (o["rgbs"] == 0)).sum()), max_radius=int(o["radii"].max())))
        _CACHE[("census", name)] = rows
    return _CACHE[("census", name)]


def clamped_rows(name, view=0):
    """(visible rows the frustum clamp acts on, visible rows it leaves alone) of one view, float64"""
    P, c2ws, K = scene(name)
    o, _ = front_ref(P, c2ws[view], K, 3, 3, False, None, torch.float64)
    vis = o["radii"] > 0
    tz = np.where(vis, o["t"][:, 2], 1.0)
    cl = (np.abs(o["t"][:, 0] / tz) > 1.3 * (0.5 * K["W"] / K["fx"])) | (np.abs(o["t"][:, 1] / tz) > 1.3 * (0.5 * K["H"] / K["fy"]))
    return vis & cl, vis & ~cl


# ---------------------------------------------------------------------------------------- cotangents and cached references
COTANGENT_SETS = {"a": ("xys", "conics", "rgbs", "opac"),            # every output of the entry point (+ depths where it takes one)
                  "b": ("conics",), "c": ("xys",), "d": ("depths",)}


def cotangents(name, cset, depth=False):
    """seeded normal float32 cotangents [C][N][..] of one scene; the sets share their draws"""
    if ("cot", name) not in _CACHE:
        P, c2ws, _ = scene(name)
        C, N = len(c2ws), P["means"].shape[0]
        g = np.random.default_rng(1000 + SCENES[name]["seed"])
        _CACHE[("cot", name)] = {k: g.normal(size=(C, N) + sh).astype(np.float32) for k, sh in
                                 (("xys", (2,)), ("depths", ()), ("conics", (3,)), ("rgbs", (3,)), ("opac", ()))}
    names = COTANGENT_SETS[cset] + (("depths",) if depth and cset == "a" else ())
    return {k: _CACHE[("cot", name)][k] for k in names}


def row_norms(a):
    a = np.asarray(a, np.float64)
    return np.linalg.norm(a.reshape(a.shape[0], -1), axis=1)


def ref_views(name, deg=3, n_use=3, aa=False, cset="a", depth=False, dtype=torch.float64, views=None, straight_through=False):
    """front_ref of the given views of a scene (default: all) under the cotangent set, cached: {"outs": per-view outputs, "views": per-view
    gradients, "sum": their float64 sum, "den": the row metric's denominators (sum of the per-view row norms, plus the floor)}"""
    P, c2ws, K = scene(name)
    views = tuple(range(len(c2ws))) if views is None else tuple(views)
    cot = cotangents(name, cset, depth)
    per = []
    for v in views:
        key = ("ref", name, deg, n_use, aa, cset, depth, dtype, v, straight_through)
        if key not in _CACHE:
            _CACHE[key] = front_ref(P, c2ws[v], K, deg, n_use, aa, {k: c[v] for k, c in cot.items()}, dtype, straight_through)
        per.append(_CACHE[key])
    grads = [g for _, g in per]
    den = {k: sum(row_norms(g[k]) for g in grads) for k in KEYS}
    den["quats"] = den["quats"] + den["scales"]
    return dict(outs=[o for o, _ in per], views=grads, sum={k: sum(g[k] for g in grads) for k in KEYS}, den=den)


def row_errors(got, ref, den, slack=None):
    """e_row of every row with a non-zero denominator -> (worst e_row, rows compared).  slack [rows]: an absolute allowance per row,
    subtracted from |got - ref| first (the rounding of an accumulation onto a non-zero buffer).  Where the denominator is 0 the row must
    be exactly 0 on both sides (within the slack)."""
    d = row_norms(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    if slack is not None:
        d = np.maximum(d - slack, 0.0)
    live = den > 0
    assert np.all(row_norms(ref)[~live] == 0) and np.all(d[~live] == 0), "a row without a reference gradient is not exactly zero"
    return (float((d[live] / den[live]).max()) if live.any() else 0.0), int(live.sum())


def check_grads(label, got, ref, keys=KEYS, before=None):
    """every leaf gradient in `got` (arrays or tensors) against ref_views' sum, by the row metric and BARS.  before: the buffers' earlier
    contents x of an accumulating entry point -- (result - x) is held to the bar plus 2^-23 |x_row|."""
    for k in keys:
        g = np.asarray(got[k].detach().cpu().numpy() if torch.is_tensor(got[k]) else got[k], np.float64)
        assert np.isfinite(g).all(), (label, k)
        slack = None
        if before is not None:
            x = np.asarray(before[k].detach().cpu().numpy() if torch.is_tensor(before[k]) else before[k], np.float64)
            g, slack = g - x, 2.0 ** -23 * row_norms(x.reshape(ref["sum"][k].shape))
        worst, _ = row_errors(g, ref["sum"][k], ref["den"][k], slack)
        within(f"{label}: {k} worst row error", worst, BARS[k])


def reference_distances():
    """worst e_row of the float32 front_ref against the float64 one, per leaf tensor, over every scene (each view alone, and views9's sum
    over its 9 views), every SH_MODES pair under set a with a depth cotangent, and sets b, c, d: what BARS is four times of"""
    if "dist" not in _CACHE:
        worst = dict.fromkeys(KEYS, 0.0)
        for name in SCENES:
            P, c2ws, K = scene(name)
            for deg, n_use, cset in [(deg, n_use, "a") for deg, n_use in SH_MODES] + [(3, 3, s) for s in "bcd"]:
                cot = cotangents(name, cset, depth=True)
                tot = None                                             # (float64 sum, float32 sum, denominators) over the views so far
                for v, c2w in enumerate(c2ws):
                    g64, g32 = (front_ref(P, c2w, K, deg, n_use, False, {k: c[v] for k, c in cot.items()}, dt)[1]
                                for dt in (torch.float64, torch.float32))
                    den = {k: row_norms(g64[k]) for k in KEYS}
                    one = (g64, g32, den)
                    tot = one if tot is None else tuple({k: a[k] + b[k] for k in KEYS} for a, b in zip(tot, one))
                    for s64, s32, d in (one, tot) if v == len(c2ws) - 1 and v > 0 else (one,):
                        for k in KEYS:
                            dk = d[k] + d["scales"] if k == "quats" else d[k]
                            worst[k] = max(worst[k], row_errors(s32[k], s64[k], dk)[0])
        _CACHE["dist"] = worst
    return _CACHE["dist"]


# ---------------------------------------------------------------------------------------- forward outputs, per row
# e_row of a forward output over the rows the view keeps: |got - ref|_2 / (|ref_row|_2 + floor).  Floors: xys cx + cy (the principal point is
# added last, so a pixel coordinate near 0 carries the rounding of a number of that size); rgbs and opac 1 (clamp(SH + 0.5) and sigmoid are
# sums of O(1) terms: absolute error); depths and conics 0.  FWD_BARS = 4 x the worst float32-vs-float64 front_ref distance, as BARS.  The
# float32 side sums `means @ W3.T` in the order of the CPU's BLAS, so xys, depths and conics differ between machines -- measured on two:
# xys 1.59e-6 / 1.65e-6, depths 1.65e-6 / 2.65e-6 (a Gaussian 0.011 in front of the camera: a sum of terms of size 0.5), conics 2.89e-6 /
# 5.35e-6; the bars are four times the larger figure.  rgbs 9.19e-8 and opac 4.35e-8 are elementwise and the same on both.
FWD_BARS = {"xys": 6.6e-6, "depths": 1.06e-5, "conics": 2.14e-5, "rgbs": 3.7e-7, "opac": 1.7e-7}


def forward_errors(got, ref_out, K, aa=False):
    """{output: worst e_row} of one view's forward outputs (arrays [N][..]) against front_ref's, over the rows with radii > 0; every other row
    must be exactly 0 -- except opac of the classic forward, which is sigmoid(logit) for every row, and the conic, which the kernels (like gsplat)
    write before the tile-box cull, where nothing reads it"""
    vis = ref_out["radii"] > 0
    floors = {"xys": K["cx"] + K["cy"], "depths": 0.0, "conics": 0.0, "rgbs": 1.0, "opac": 1.0}
    worst = {}
    for k, g in got.items():
        g = np.asarray(g, np.float64)
        assert np.isfinite(g).all(), k
        ref = ref_out["opac_all" if k == "opac" and not aa else k]
        rows = np.ones_like(vis) if k == "opac" and not aa else vis
        assert k == "conics" or np.all(g[~rows] == 0), f"{k}: a culled row is not zero"
        worst[k] = float((row_norms(g - ref)[rows] / (row_norms(ref)[rows] + floors[k])).max())
    return worst


def forward_distances():
    """worst forward e_row of the float32 front_ref against the float64 one over every scene, view and SH mode: what FWD_BARS is four times of"""
    if "fdist" not in _CACHE:
        worst = dict.fromkeys(FWD_BARS, 0.0)
        for name in SCENES:
            P, c2ws, K = scene(name)
            for c2w in c2ws:
                for deg, n_use in SH_MODES:
                    o32, o64 = (front_ref(P, c2w, K, deg, n_use, False, None, dt)[0] for dt in (torch.float32, torch.float64))
                    for k, v in forward_errors({k: o32["opac_all" if k == "opac" else k] for k in FWD_BARS}, o64, K).items():
                        worst[k] = max(worst[k], v)
        _CACHE["fdist"] = worst
    return _CACHE["fdist"]

"""Price of the differentiable depth of the fused render (RenderAux.depth_grad).  Scene: 1 M Gaussians at 512 x 512, 8 views per launch
set (the synthetic scene and cameras of scripts/bench_raster_nd.py's family: seed 3, scale_mean 0.01, fx 540).  Times are per view
(median of 5 runs of `--iters` launch sets each) for

  off      render_views forward + backward with depth_grad off (rgb + alpha cotangents; the kernels of the parent commit),
  on       the same with depth_grad on and a depth cotangent,
  stages   the compositing backward, the projection backward and the depth L1 loss alone, with and without the depth channel,
  ops      the operator-surface way to the same gradients: project_gaussians + SH + rasterize_gaussians for rgb, and a second
           rasterize_gaussians call on depths[:, None] colours, per view.

--mode off runs on a checkout of the parent commit too: configuration (i) of an A/B on one box.
usage: python scripts/bench_raster_depth.py [--mode all|off] [--iters 5] [--gaussians 1000000]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gaussctrl_amd import _lib as L, gsplat_ops as ops, synthetic as syn
from gaussctrl_amd.camera import camera_to_gsplat

DEV = "cuda:0"
KEYS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def timeit(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record(); torch.cuda.synchronize()
        runs.append(s.elapsed_time(e) / iters * 1e3)
    return statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=("all", "off"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=8)
    a = ap.parse_args()
    N, W, H, C = a.gaussians, 512, 512, a.views
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device=DEV)
    P = syn.make_gaussians(N, seed=3, scale_mean=0.01)
    K = dict(fx=540.0, fy=540.0 * 0.99, cx=W / 2 + 1.3, cy=H / 2 - 2.1)
    c2ws = syn.make_cameras(C, seed=4)
    cams = [camera_to_gsplat(c, K["fx"], K["fy"], K["cx"], K["cy"], W, H) for c in c2ws]
    tp = {k: t(P[k]).requires_grad_(True) for k in KEYS}
    bg = t([0.1, 0.2, 0.3])
    g = torch.Generator(device=DEV).manual_seed(0)
    v_rgb = torch.randn(C, H, W, 3, device=DEV, generator=g); v_a = torch.randn(C, H, W, device=DEV, generator=g)
    v_d = torch.randn(C, H, W, device=DEV, generator=g)
    print(f"# {torch.cuda.get_device_name(0)}  N={N} {W}x{H} views={C}; times in us per VIEW")
    res = {}

    def fused(depth_grad):
        def run():
            for p in tp.values():
                p.grad = None
            aux = ops.RenderAux()
            if depth_grad:
                aux.depth_grad = True
            rgb, alpha, depth = ops.render_views(*(tp[k] for k in KEYS), cams, bg, True, 3, aux)
            grads = [v_rgb, v_a] + ([v_d] if depth_grad else [])
            torch.autograd.backward([rgb, alpha] + ([depth] if depth_grad else []), grads)
        return run

    res["fused_off_us"] = timeit(fused(False), a.iters) / C
    print(f"fused fwd+bwd, depth_grad off: {res['fused_off_us']:9.1f}")
    if a.mode == "off":
        print(json.dumps({k: round(v, 1) for k, v in res.items()}))
        return
    res["fused_on_us"] = timeit(fused(True), a.iters) / C
    print(f"fused fwd+bwd, depth_grad on : {res['fused_on_us']:9.1f}   ({res['fused_on_us'] / res['fused_off_us']:.3f}x)")

    # ---- per stage, on the tensors of one forward
    lib = L.lib()
    st = L.stream_ptr()
    # the stages run on what one differentiable forward saved for its backward
    aux = ops.RenderAux(); aux.depth_grad = True
    rgb, alpha, depth = ops.render_views(*(tp[k] for k in KEYS), cams, bg, True, 3, aux)
    ctx = rgb.grad_fn
    (m, ls, q, op, dc, rest, radii, conics, xys, rgbs, opac, ids_s, bins, bgc, fT, fi, pre_clamp, depths, dep) = ctx.saved_tensors
    cams_, CH, tb, N_, C_, M_cap, shared_bg, sh_degree, n_use = ctx.meta
    zeros = lambda with_depth: torch.zeros(C * N * (10 if with_depth else 9), device=DEV)

    def comp(with_depth):
        def run():
            vb = zeros(with_depth)
            v_xy = vb[:2 * C * N]; v_con = vb[2 * C * N:5 * C * N]; v_col = vb[5 * C * N:8 * C * N]; v_op = vb[8 * C * N:9 * C * N]
            common = (L.i32(C), L.i64(N), L.i64(M_cap), L.i32(1), L.i32(shared_bg), L.i32(H), L.i32(W), L.i32(tb[0]), L.i32(tb[1]), L.ptr(ids_s),
                      L.ptr(bins), L.ptr(xys), L.ptr(conics), L.ptr(rgbs), L.ptr(opac), L.ptr(bgc), L.ptr(fT), L.ptr(fi), L.ptr(v_rgb), L.ptr(v_a),
                      L.ptr(pre_clamp), L.ptr(v_xy), L.ptr(v_con), L.ptr(v_col), L.ptr(v_op))
            if with_depth:
                L.check(lib.gc_rasterize_bwd_depth_views(*common, L.ptr(depths), L.ptr(dep), L.ptr(v_d), L.ptr(vb[9 * C * N:]), st))
            else:
                L.check(lib.gc_rasterize_bwd_views(*common, st))
            return vb
        return run

    vb = comp(True)()
    outs = [torch.empty_like(x) for x in (m, ls, q, op, dc, rest)]

    def proj(with_depth):
        def run():
            common = (L.i64(N), L.i32(C), L.i32(0), L.ptr(m), L.ptr(ls), L.ptr(q), L.ptr(op), L.ptr(rgbs), L.i32(sh_degree), L.i32(n_use), CH,
                      L.i32(H), L.i32(W), L.ptr(radii), L.ptr(conics), L.ptr(vb[:2 * C * N]), L.ptr(vb[2 * C * N:5 * C * N]),
                      L.ptr(vb[5 * C * N:8 * C * N]), L.ptr(vb[8 * C * N:9 * C * N])) + tuple(L.ptr(o) for o in outs)
            if with_depth:
                L.check(lib.gc_project_sh_bwd_depth_views(*common, L.ptr(vb[9 * C * N:]), st))
            else:
                L.check(lib.gc_project_sh_bwd_views(*common, st))
        return run

    from gaussctrl_amd.train_ops import depth_l1_loss_views
    target = depth.detach().clone() + 0.01

    def loss():
        d = depth.detach().requires_grad_(True)
        depth_l1_loss_views(d, target).sum().backward()

    for name, fn in (("composite_bwd_off_us", comp(False)), ("composite_bwd_on_us", comp(True)), ("project_bwd_off_us", proj(False)),
                     ("project_bwd_on_us", proj(True)), ("depth_l1_us", loss)):
        res[name] = timeit(fn, a.iters) / C
        print(f"{name:24s}: {res[name]:9.1f}")

    # ---- operator surface: rgb chain + a second rasterize_gaussians call on depth colours, one view at a time
    def surface():
        for p in tp.values():
            p.grad = None
        for v, (cam, c2w) in enumerate(zip(cams, c2ws)):
            colors = torch.cat([tp["features_dc"][:, None, :], tp["features_rest"]], 1)
            qn = tp["quats"] / tp["quats"].norm(dim=-1, keepdim=True)
            V4 = t(cam["viewmat4"]); full = t(np.asarray(cam["fullproj"], np.float32).reshape(4, 4))
            xy, dz, rad, con, nth, _ = ops.project_gaussians(tp["means"], torch.exp(tp["scales"]), 1, qn, V4[:3], full, K["fx"], K["fy"],
                                                             K["cx"], K["cy"], H, W, cam["tile_bounds"])
            vd = tp["means"].detach() - t(c2w[:3, 3]); vd = vd / vd.norm(dim=-1, keepdim=True)
            col = torch.clamp(ops.spherical_harmonics(3, vd, colors) + 0.5, min=0.0)
            o = torch.sigmoid(tp["opacities"])
            im, al = ops.rasterize_gaussians(xy, dz, rad, con, nth, col, o, H, W, background=bg, return_alpha=True)
            de = ops.rasterize_gaussians(xy, dz, rad, con, nth, dz[:, None], o, H, W, background=torch.zeros(1, device=DEV))[..., 0]
            dn = torch.where(al > 0, de / al.clamp(min=1e-30), torch.full_like(de, 1000.0))
            torch.autograd.backward([torch.clamp(im, max=1.0), al, dn], [v_rgb[v], v_a[v], v_d[v]])

    res["surface_us"] = timeit(surface, max(1, a.iters // 2)) / C
    print(f"operator surface, rgb + depth call: {res['surface_us']:9.1f}   ({res['surface_us'] / res['fused_on_us']:.2f}x the fused form)")
    print(json.dumps({k: round(v, 1) for k, v in res.items()}))


if __name__ == "__main__":
    main()

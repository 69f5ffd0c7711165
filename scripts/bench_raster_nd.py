"""N-channel compositing (gc_rasterize_nd_fwd / _bwd) against the 3-channel op called once per channel triple, which is what a caller
would write without it.  Scene: 1 M Gaussians at 512 x 512, the synthetic scene of tests/test_raster_gpu.py (seed 3, scale_mean 0.01,
fx 540); the tile lists are built once and both sides composite the same lists.  Times are per call (median of 5 runs of `--iters`
calls each), compositing only: forward, and forward + backward (gradient buffers zero-filled inside the timed region on both sides).
The per-triple side gets its colour / background / upstream slices prepared outside the timed region.
usage: python scripts/bench_raster_nd.py [--channels 1,4,8,16,32,64] [--iters 10]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gaussctrl_amd import gsplat_ops as ops, synthetic as syn
from gaussctrl_amd.camera import camera_to_gsplat

DEV = "cuda:0"


def scene(N, W, H, fx):
    P = syn.make_gaussians(N, seed=3, scale_mean=0.01)
    c2w = syn.make_cameras(1, seed=4)[0]
    K = dict(fx=fx, fy=fx * 0.99, cx=W / 2 + 1.3, cy=H / 2 - 2.1)
    cam = camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], W, H)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
    q = P["quats"] / np.linalg.norm(P["quats"], axis=-1, keepdims=True)
    V4 = t(cam["viewmat4"]); full = t(np.asarray(cam["fullproj"], np.float32).reshape(4, 4))
    with torch.no_grad():
        xys, depths, radii, conics, nth, _ = ops.project_gaussians(t(P["means"]), torch.exp(t(P["scales"])), 1, t(q), V4[:3], full,
                                                                   K["fx"], K["fy"], K["cx"], K["cy"], H, W, cam["tile_bounds"])
        opac = torch.sigmoid(t(P["opacities"])).reshape(-1).contiguous()
    tb = cam["tile_bounds"]
    M, _, ids, bins, _ = ops.bin_and_sort_gaussians(N, xys, depths, radii, nth, tb)
    return xys, conics, opac, tb, ids, bins, M


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
    ap.add_argument("--channels", default="1,4,8,16,32,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    a = ap.parse_args()
    N, W, H = a.gaussians, 512, 512
    xys, conics, opac, tb, ids, bins, M = scene(N, W, H, 540.0)
    print(f"# {torch.cuda.get_device_name(0)}  N={N} {W}x{H} intersections={M}; times in us per call")
    print(f"# {'C':>3} {'triples':>7} {'nd fwd':>9} {'3ch x k fwd':>11} {'fwd ratio':>9} {'nd f+b':>9} {'3ch x k f+b':>11} {'f+b ratio':>9}")
    g = torch.Generator(device=DEV).manual_seed(0)
    for C in [int(c) for c in a.channels.split(",")]:
        k = -(-C // 3)
        colors = torch.rand(N, C, device=DEV, generator=g)
        bg = torch.rand(C, device=DEV, generator=g)
        v_out = torch.randn(H, W, C, device=DEV, generator=g)
        v_alpha = torch.randn(H, W, device=DEV, generator=g)
        pad = lambda t: torch.nn.functional.pad(t, (0, 3 * k - C))
        col3 = [pad(colors)[:, 3 * i:3 * i + 3].contiguous() for i in range(k)]
        bg3 = [pad(bg)[3 * i:3 * i + 3].contiguous() for i in range(k)]
        vo3 = [pad(v_out)[..., 3 * i:3 * i + 3].contiguous() for i in range(k)]

        def nd_fwd():
            return ops._rasterize_nd_fwd(H, W, tb, ids, bins, xys, conics, colors, opac, bg)

        def nd_fb():
            _, fT, fi = nd_fwd()
            ops._rasterize_nd_bwd(H, W, tb, N, ids, bins, xys, conics, colors, opac, bg, fT, fi, v_out, v_alpha)

        def tri_fwd():
            return [ops._rasterize_fwd(H, W, tb, ids, bins, xys, conics, col3[i], opac, None, bg3[i]) for i in range(k)]

        def tri_fb():
            for i, (_, _, fT, fi) in enumerate(tri_fwd()):
                ops._rasterize_bwd(H, W, tb, N, ids, bins, xys, conics, col3[i], opac, bg3[i], fT, fi, vo3[i], v_alpha if i == 0 else None)

        t = [timeit(f, a.iters) for f in (nd_fwd, tri_fwd, nd_fb, tri_fb)]
        print(f"  {C:>3} {k:>7} {t[0]:9.1f} {t[1]:11.1f} {t[1] / t[0]:9.2f} {t[2]:9.1f} {t[3]:11.1f} {t[3] / t[2]:9.2f}")
        print(json.dumps({"C": C, "triples": k, "nd_fwd_us": round(t[0], 1), "triples_fwd_us": round(t[1], 1),
                          "nd_fwd_bwd_us": round(t[2], 1), "triples_fwd_bwd_us": round(t[3], 1)}))
        sys.stdout.flush()


if __name__ == "__main__":
    main()

"""Camera pose gradient at the raster workload's launch set (1 M synthetic Gaussians, 8 cameras, 512 x 512: the configuration of
profiles/absgrad_cost.txt): what RenderAux.pose_grad costs.

  1. the kernel pair alone: gcx_pose_bwd_views (k_pose_bwd_views + k_pose_sum, csrc/raster_project.hip) on the forward state of the 8 views
     with seeded cotangents and a depth cotangent, classic and antialiased, workspace and output allocated once outside the timing; against
     the bytes it has to move -- 56 per Gaussian (means, log-scales, quaternions, opacity logit), 4 per Gaussian and view (radii) and 40 per
     KEPT Gaussian and view (conics, v_xy, v_conic, v_depths; 44 antialiased: v_opac);
  2. one training step of the fused path -- render_views, the L1 + SSIM loss over the views, backward to the six leaves -- with pose_grad on
     against off.

5 warm-up + 20 timed repetitions each, both sides ALTERNATING in one process, device events around every repetition, median and min
reported.  No ratio is promised: the numbers are recorded as measured.

    python scripts/bench_pose.py [--n 1000000] [--views 8] [--size 512] [--out profiles/pose_bench.txt]

Needs a GPU: without one it fails and writes nothing."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussctrl_amd import _lib as L, gsplat_ops as ops, synthetic as syn  # noqa: E402
from gaussctrl_amd.camera import camera_to_gsplat  # noqa: E402
from gaussctrl_amd.train_ops import l1_ssim_loss_views  # noqa: E402

DEV = "cuda:0"


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, warmup=5, reps=20):
    """{name: [ms]} of the named callables run in turn"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(event_ms(f))
    return out


def line(name, ms):
    return f"  {name:<44s} median {statistics.median(ms):8.3f} ms   min {min(ms):8.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_bench.txt"))
    a = ap.parse_args()
    lib = L.lib()
    st = L.stream_ptr()
    N, C, H, W = a.n, a.views, a.size, a.size
    P = syn.make_gaussians(N, seed=0, scale_mean=0.01)
    names = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
    tp = [torch.tensor(P[k], device=DEV) for k in names]
    cams = [camera_to_gsplat(c2w, 540.0, 540.0, W / 2, H / 2, W, H) for c2w in syn.make_cameras(C, seed=1)]
    CH = ops._cams_host(cams)
    report = [f"Camera pose gradient (gcx_pose_bwd_views, RenderAux.pose_grad), python scripts/bench_pose.py --n {N} --views {C} --size {H}",
              f"device: {torch.cuda.get_device_name(0)}", ""]

    # ---- 1. the kernel pair alone
    g = torch.Generator(device=DEV).manual_seed(0)
    report.append("1. gcx_pose_bwd_views alone (k_pose_bwd_views per group of 8 views + k_pose_sum), workspace and output allocated outside")
    nbytes = int(lib.gcx_pose_bwd_views_workspace_bytes(L.i64(N), L.i32(C)))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=DEV)
    out = torch.empty(C, 2, 3, 4, device=DEV)
    v_xy = torch.randn(C, N, 2, device=DEV, generator=g); v_conic = torch.randn(C, N, 3, device=DEV, generator=g)
    v_opac = torch.randn(C, N, device=DEV, generator=g); v_dep = torch.randn(C, N, device=DEV, generator=g)
    m, ls, q, op = tp[0], tp[1], tp[2], tp[3].reshape(-1).contiguous()
    fns, kept = {}, {}
    for aa in (False, True):
        aux = ops.RenderAux()
        aux.antialiased = aa
        with torch.no_grad():
            fr = ops._views_front(*tp, cams, 3, aux)
        kept[aa] = int((fr.radii > 0).sum())

        def call(aa=aa, radii=fr.radii, conics=fr.conics):
            L.check(lib.gcx_pose_bwd_views(L.i64(N), L.i32(C), L.i32(int(aa)), L.ptr(m), L.ptr(ls), L.ptr(q), L.ptr(op), CH, L.i32(H), L.i32(W),
                                           L.ptr(radii), L.ptr(conics), L.ptr(v_xy), L.ptr(v_conic), L.ptr(v_opac) if aa else None, L.ptr(v_dep),
                                           L.ptr(ws), L.ptr(out), st), "gcx_pose_bwd_views")
        fns["antialiased" if aa else "classic"] = call
        del fr
    t = alternate(fns)
    for aa, key in ((False, "classic"), (True, "antialiased")):
        algo = N * 56 + C * N * 4 + kept[aa] * (44 if aa else 40) + nbytes * 2
        med = statistics.median(t[key])
        report += [line(f"{key}, {kept[aa]} kept (Gaussian, view) pairs", t[key]),
                   f"    bytes N x 56 + C N x 4 + kept x {44 if aa else 40} + partials = {algo / 1e6:.1f} MB -> {algo / med / 1e6:.1f} GB/s at the median"]
    call = fns["classic"]
    call(); torch.cuda.synchronize(); first = out.clone()
    call(); torch.cuda.synchronize()
    report += [f"  two calls give the same bits: {bool(torch.equal(first.view(torch.int32), out.view(torch.int32)))}; workspace {nbytes} bytes", ""]

    # ---- 2. a training step of the fused path, pose_grad on against off
    leaves = [t_.clone().requires_grad_(True) for t_ in tp]
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    with torch.no_grad():
        target = ops.render_views(*tp, cams, bg, False, 3, ops.RenderAux())[0].clone()
        target = (target + 0.05 * torch.randn(target.shape, device=DEV, generator=g)).clamp(0, 1)

    def step(flag):
        def run():
            for t_ in leaves:
                t_.grad = None
            aux = ops.RenderAux()
            aux.pose_grad = flag
            rgb, _, _ = ops.render_views(*leaves, cams, bg, False, 3, aux)
            l1_ssim_loss_views(rgb, target, 0.2).sum().backward()
        return run

    def backward_only(flag):
        state = {}

        def prepare():
            for t_ in leaves:
                t_.grad = None
            aux = ops.RenderAux()
            aux.pose_grad = flag
            rgb, _, _ = ops.render_views(*leaves, cams, bg, False, 3, aux)
            state["loss"] = l1_ssim_loss_views(rgb, target, 0.2).sum()
        return prepare, lambda: state["loss"].backward()

    t = alternate({"off": step(False), "on": step(True)})
    mo, mn = statistics.median(t["off"]), statistics.median(t["on"])
    report += ["2. one training step of the fused path (render_views + L1 / SSIM loss over the views + backward to the six leaves)",
               line("pose_grad off", t["off"]), line("pose_grad on", t["on"]),
               f"  on / off = {mn / mo:.4f} (+{mn - mo:.3f} ms at the medians)"]
    # the backward alone (the forward and the loss are prepared outside the timed region)
    bw = {}
    for key, flag in (("off", False), ("on", True)):
        prepare, run = backward_only(flag)
        bw[key] = (prepare, run)
    ms = {"off": [], "on": []}
    for rep in range(25):
        for key in ("off", "on"):
            prepare, run = bw[key]
            prepare()
            torch.cuda.synchronize()
            v = event_ms(run)
            if rep >= 5:
                ms[key].append(v)
    bo, bn = statistics.median(ms["off"]), statistics.median(ms["on"])
    report += [line("backward alone, pose_grad off", ms["off"]), line("backward alone, pose_grad on", ms["on"]),
               f"  on / off = {bn / bo:.4f} (+{bn - bo:.3f} ms at the medians: the kernel pair, its allocations and the [C, 3, 4] chain)"]
    text = "\n".join(report) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

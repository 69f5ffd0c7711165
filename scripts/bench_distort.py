"""Distortion loss at the raster workload's launch set (1 M synthetic Gaussians, 8 cameras, 512 x 512: the configuration of
profiles/pose_bench.txt): what RenderAux.distort costs, and that it costs nothing when it is off.

  1. each kernel alone: gcx_distort_fwd_views (k_distort_fwd) and gcx_distort_bwd_views (k_distort_bwd, csrc/raster_distort.hip) on the lists
     of the 8 views, both depth maps, buffers allocated once outside the timing; against the algorithmic bytes -- 32 per list entry (id,
     xy, conic, opacity, depth) per kept (tile, Gaussian) pair, M of them over the views, plus the images (forward: 2 written; backward: 4
     read); the gradient atomics of the backward are not counted;
  2. one training step of the fused path -- render_views, the L1 + SSIM loss over the views, backward to the six leaves -- with the switch
     on (the mean of the map added to the loss) against off;
  3. with --parent DIR (a checkout of the parent commit, built): the step with the switch off against the parent's step, and the parent
     against itself, all three ALTERNATING in one process (the parent's package is loaded under another name next to this one; each has
     its own library).  The off path must not differ from the parent by more than the parent differs from itself: the difference of the
     medians is reported against BOTH the interquartile range of the parent's single repetitions and the difference between the medians
     of its two series (one draw of a small number: the first is the spread the verdict rests on).

5 warm-up + 20 timed repetitions each, device events around every repetition, median and min reported.  No figure is promised: the numbers
are recorded as measured.

    python scripts/bench_distort.py [--n 1000000] [--views 8] [--size 512] [--parent DIR] [--out profiles/distort_bench.txt]

Needs a GPU: without one it fails and writes nothing."""
import argparse
import importlib.util
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
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


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
    return f"  {name:<44s} median {statistics.median(ms):8.3f} ms   min {min(ms):8.3f} ms   max {max(ms):8.3f} ms"


def load_parent(path):
    """the package gaussctrl_amd of another checkout as `gaussctrl_amd_parent` (its modules import each other relatively, its loader finds
    the library next to itself)"""
    pkg = os.path.join(os.path.abspath(path), "gaussctrl_amd")
    spec = importlib.util.spec_from_file_location("gaussctrl_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["gaussctrl_amd_parent"] = mod
    spec.loader.exec_module(mod)
    import gaussctrl_amd_parent.gsplat_ops as p_ops
    import gaussctrl_amd_parent.train_ops as p_train
    assert os.path.dirname(p_ops.L.LIB_PATH) == pkg and p_ops.L.lib() is not L.lib()
    return p_ops, p_train.l1_ssim_loss_views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distort_bench.txt"))
    a = ap.parse_args()
    N, C, H, W = a.n, a.views, a.size, a.size
    P = syn.make_gaussians(N, seed=0, scale_mean=0.01)
    tp = [torch.tensor(P[k], device=DEV) for k in NAMES]
    cams = [camera_to_gsplat(c2w, 540.0, 540.0, W / 2, H / 2, W, H) for c2w in syn.make_cameras(C, seed=1)]
    report = [f"Distortion loss (gcx_distort_fwd_views / gcx_distort_bwd_views, RenderAux.distort), python scripts/bench_distort.py --n {N} --views {C} "
              f"--size {H}" + (" --parent <parent checkout>" if a.parent else ""), f"device: {torch.cuda.get_device_name(0)}", ""]

    # ---- 1. each kernel alone
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        fr = ops._views_front(*tp, cams, 3, None)
    tb = fr.tb
    M = int(fr.cnt.sum())
    img, fT = torch.empty(C, H, W, 3, device=DEV), torch.empty(C, H, W, device=DEV)
    fi = torch.empty(C, H, W, dtype=torch.int32, device=DEV)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    L.call("gc_rasterize_fwd_views", C, N, fr.M_cap, fr.shared_op, 1, H, W, tb[0], tb[1], fr.ids_s, fr.bins, fr.xys, fr.conics, fr.rgbs, fr.opac, None, bg,
           img, None, fT, fi)
    v_dist = torch.randn(C, H, W, device=DEV, generator=g)
    dist, wt = torch.empty(C, H, W, device=DEV), torch.empty(C, H, W, device=DEV)
    grads = [torch.zeros(C, N, w, device=DEV) for w in (2, 3)] + [torch.zeros(C, N, device=DEV) for _ in range(2)]
    head = (C, N, fr.M_cap, fr.shared_op, H, W, tb[0], tb[1], fr.ids_s, fr.bins, fr.xys, fr.conics, fr.opac, fr.depths)
    fns = {}
    for mode, name in enumerate(ops.DISTORT_DEPTH_MAPS):
        fns[f"k_distort_fwd, {name}"] = lambda mode=mode: L.call("gcx_distort_fwd_views", *head, mode, 0.2, 100.0, dist, wt)
        fns[f"k_distort_bwd, {name}"] = lambda mode=mode: L.call("gcx_distort_bwd_views", *head, mode, 0.2, 100.0, fT, fi, wt, v_dist, *grads)
    fns["k_distort_fwd, linear"]()          # wt for the backward
    t = alternate(fns)
    report.append(f"1. each kernel alone: M = {M} kept (tile, Gaussian) pairs over {C} views, {C * H * W} pixels")
    for key, ms in t.items():
        fwd = "fwd" in key
        algo = M * 32 + C * H * W * 4 * (2 if fwd else 4)
        med = statistics.median(ms)
        report += [line(key, ms), f"    algorithmic bytes M x 32 + images x {2 if fwd else 4} = {algo / 1e6:.1f} MB ({algo / M:.1f} per kept pair) -> "
                                  f"{algo / med / 1e6:.1f} GB/s at the median"]
    report.append("")

    # ---- 2. a training step of the fused path, the switch on against off
    def make_step(o, loss_views, flag):
        leaves = [t_.clone().requires_grad_(True) for t_ in tp]
        with torch.no_grad():
            target = o.render_views(*tp, cams, bg, False, 3, o.RenderAux())[0].clone()
            target = (target + 0.05 * torch.randn(target.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))).clamp(0, 1)

        def run():
            for t_ in leaves:
                t_.grad = None
            aux = o.RenderAux()
            if flag:
                aux.distort = True
            rgb, _, _ = o.render_views(*leaves, cams, bg, False, 3, aux)
            loss = loss_views(rgb, target, 0.2).sum()
            if flag:
                loss = loss + 0.01 * aux.distort_map.mean()
            loss.backward()
        return run

    t = alternate({"off": make_step(ops, l1_ssim_loss_views, False), "on": make_step(ops, l1_ssim_loss_views, True)})
    mo, mn = statistics.median(t["off"]), statistics.median(t["on"])
    report += ["2. one training step of the fused path (render_views + L1 / SSIM loss over the views + backward to the six leaves)",
               line("distort off", t["off"]), line("distort on (+ 0.01 x mean of the map)", t["on"]),
               f"  on / off = {mn / mo:.4f} (+{mn - mo:.3f} ms at the medians)", ""]

    # ---- 3. the off path against the parent commit
    if a.parent:
        p_ops, p_loss = load_parent(a.parent)
        t = alternate({"parent": make_step(p_ops, p_loss, False), "head, off": make_step(ops, l1_ssim_loss_views, False),
                       "parent again": make_step(p_ops, p_loss, False)}, reps=30)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = abs(med["parent"] - med["parent again"])
        q = statistics.quantiles(t["parent"] + t["parent again"], n=4)
        diff = med["head, off"] - 0.5 * (med["parent"] + med["parent again"])
        report += ["3. the step with the switch off against the parent commit's step, three series alternating in one process (30 repetitions each)",
                   *(line(k, v) for k, v in t.items()),
                   f"  parent against itself: medians differ by {spread:.3f} ms; interquartile range of its 60 repetitions {q[2] - q[0]:.3f} ms",
                   f"  head (off) - parent = {diff:+.3f} ms at the medians ({100 * diff / med['parent']:+.2f} %): "
                   + ("inside" if abs(diff) <= q[2] - q[0] else "OUTSIDE") + " the interquartile range of the parent's single repetitions, "
                   + ("inside" if abs(diff) <= spread else "outside") + " the difference between the parent's two medians", ""]
    else:
        report += ["3. the off path against the parent commit: not measured (no --parent)", ""]
    text = "\n".join(report)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""Cost of RenderAux.absgrad on the training render's backward, at the raster workload's scene size (bench.py --workload raster: 1 M Gaussians,
8 cameras per launch set, 512 x 512, fx = fy = 540, no depth).  One process, one scene; the backward of gsplat_ops.render_views is timed
between HIP events on the launch stream, the switch off and on in alternation (off, on, off, on, ...) so that clock drift lands on both.

    python scripts/absgrad_cost.py [--gaussians N] [--views C] [--reps R] [--out FILE]

Prints the per-repetition times, their medians and the on / off ratio; --out also writes them as text."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gaussctrl_amd import gsplat_ops as ops, synthetic as syn  # noqa: E402
from gaussctrl_amd.camera import camera_to_gsplat  # noqa: E402

KEYS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    K = syn.ROUND_INTRINSICS
    H, W = K["H"], K["W"]
    P = syn.make_gaussians(args.gaussians, seed=0)
    tp = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in P.items()}
    cams = [camera_to_gsplat(c, K["fx"], K["fy"], K["cx"], K["cy"], W, H) for c in syn.make_cameras(args.views, seed=1)]
    g = torch.Generator(device=dev).manual_seed(2)
    target = torch.rand(args.views, H, W, 3, device=dev, generator=g)
    bg = torch.rand(args.views, 3, device=dev, generator=g)

    def once(absgrad):
        for t in tp.values():
            t.grad = None
        aux = ops.RenderAux()
        aux.absgrad = absgrad
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        rgb, alpha, _ = ops.render_views(*(tp[k] for k in KEYS), cams, bg, False, 3, aux)
        loss = (rgb - target).abs().mean()
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        assert (aux.xys_absgrad is not None) == absgrad
        return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

    for _ in range(args.warmup):
        once(False); once(True)
    fwd = {False: [], True: []}
    bwd = {False: [], True: []}
    for _ in range(args.reps):
        for sw in (False, True):
            f, b = once(sw)
            fwd[sw].append(f); bwd[sw].append(b)
    med = {sw: statistics.median(bwd[sw]) for sw in bwd}
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"scene: {args.gaussians} Gaussians, {args.views} cameras, {W} x {H}, render_views, no depth, loss = mean |rgb - target|",
             f"backward (loss.backward(): loss + compositing + projection backward), ms, {args.reps} alternating repetitions",
             "  absgrad off: " + " ".join(f"{v:.3f}" for v in bwd[False]),
             "  absgrad on : " + " ".join(f"{v:.3f}" for v in bwd[True]),
             f"  median off {med[False]:.3f} ms, on {med[True]:.3f} ms, ratio on / off {med[True] / med[False]:.4f}",
             f"  spread (max - min) off {max(bwd[False]) - min(bwd[False]):.3f} ms, on {max(bwd[True]) - min(bwd[True]):.3f} ms",
             f"forward + loss, ms: median off {statistics.median(fwd[False]):.3f}, on {statistics.median(fwd[True]):.3f} (the switch does not touch it)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

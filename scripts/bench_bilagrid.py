"""Bilateral-grid colour compensation (include/gaussctrl_bilagrid.h, csrc/train_bilagrid.hip) at C = 1 and C = 8 images of 512 x 512, a
16 x 16 x 8 grid per view, V = 40 views: what the kernels cost against the same maths composed in torch, and against the step they sit
beside.

  1. slice forward + backward (gcx_bilagrid_slice_fwd_views + gcx_bilagrid_slice_bwd_views, the zeroing of v_grids included) against
     F.grid_sample on 5-D input + the 3x4 product + autograd, float32, same GPU, same process; with --ab-lib also the same two kernels
     from a build that never stages grid values in LDS (-DGC_BILAGRID_STAGE_MAX_BYTES=0: vertex reads through L1 / L2), alternating;
  2. total variation value + gradient (gcx_bilagrid_tv_fwd_bwd, one launch pair) against index differences + autograd;
  3. the fused render + L1/SSIM loss + backward of the same C views (ops.render_views, l1_ssim_loss_views) on a synthetic scene.

The images are smooth (a render-like gradient plus a little noise), as the luma axis of a real render is: neighbouring pixels mostly share
a z cell (few cells per wave: the backward sums them in registers); a uniform-random image (many cells per wave) is timed beside it.

5 warm-up + 20 timed repetitions each, ALTERNATING; a repetition is a batch of back-to-back calls (as many as fill about a millisecond, at
most 20) between one pair of device events, reported per call; median and min.  No ratio is fixed in advance: the numbers are recorded
as measured.

The A/B library is not part of the default build:

    make -C gaussctrl_amd/csrc ../libbilagrid_nostage.so
    python scripts/bench_bilagrid.py --ab-lib gaussctrl_amd/libbilagrid_nostage.so

    python scripts/bench_bilagrid.py [--size 512] [--views 40] [--gaussians 200000] [--ab-lib PATH] [--out profiles/bilagrid_bench.txt]

Needs a GPU: without one it fails and writes nothing."""
import argparse
import ctypes
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussctrl_amd import _lib as L, bilagrid, gsplat_ops as ops, synthetic as syn  # noqa: E402
from gaussctrl_amd.camera import camera_to_gsplat  # noqa: E402
from gaussctrl_amd.train_ops import l1_ssim_loss_views  # noqa: E402

DEV = "cuda:0"
LUMA = (0.299, 0.587, 0.114)


def event_ms(fn, n=1):
    """milliseconds per call of n back-to-back calls between one pair of device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, warmup=5, reps=20):
    """{name: [ms per call]} of the named callables run in turn.  A call of a few hundredths of a millisecond is shorter than what one
    event pair resolves and than the gap between two launches from Python, so each repetition times a batch: as many back-to-back calls
    as fill about a millisecond (1 to 20, from one timed call after the warm-up)."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    batch = {k: max(1, min(20, int(round(1.0 / max(event_ms(f), 1e-3))))) for k, f in fns.items()}
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(event_ms(f, batch[k]))
    return out


def line(name, ms):
    return f"  {name:<52s} median {statistics.median(ms):8.3f} ms   min {min(ms):8.3f} ms"


def torch_slice(grids, rgb, view_idx):
    """the contract of the header composed from torch operators, in the dtype of its inputs"""
    C, H, W, _ = rgb.shape
    dt, dev = rgb.dtype, rgb.device
    xs = 2 * (torch.arange(W, dtype=dt, device=dev) + 0.5) / W - 1
    ys = 2 * (torch.arange(H, dtype=dt, device=dev) + 0.5) / H - 1
    zs = 2 * (rgb * torch.tensor(LUMA, dtype=dt, device=dev)).sum(-1).clamp(0, 1) - 1
    coords = torch.stack([xs[None, None, :].expand(C, H, W), ys[None, :, None].expand(C, H, W), zs], dim=-1)[:, None]
    A = F.grid_sample(grids[view_idx], coords, mode="bilinear", padding_mode="border", align_corners=True)
    A = A[:, :, 0].permute(0, 2, 3, 1).reshape(C, H, W, 3, 4)
    return torch.matmul(A[..., :3], rgb[..., None])[..., 0] + A[..., 3]


def torch_tv(g):
    return ((g[..., 1:] - g[..., :-1]) ** 2).mean() + ((g[..., 1:, :] - g[..., :-1, :]) ** 2).mean() + ((g[:, :, 1:] - g[:, :, :-1]) ** 2).mean()


def smooth_images(C, H, W, gen):
    y, x = torch.meshgrid(torch.linspace(0, 1, H, device=DEV), torch.linspace(0, 1, W, device=DEV), indexing="ij")
    base = torch.stack([0.15 + 0.7 * x, 0.2 + 0.6 * y, 0.5 + 0.4 * torch.sin(6.0 * (x + y))], -1)
    phase = torch.arange(C, device=DEV).float().reshape(C, 1, 1, 1) * 0.05
    return (base[None] + phase + 0.01 * torch.randn(C, H, W, 3, device=DEV, generator=gen)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--gaussians", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilagrid_bench.txt"))
    ap.add_argument("--ab-lib", default=None, help="a library with csrc/train_bilagrid.hip built -DGC_BILAGRID_STAGE_MAX_BYTES=0 (and abi.cpp)")
    a = ap.parse_args()
    lib = L.lib()
    ab = ctypes.CDLL(a.ab_lib) if a.ab_lib else None
    st = L.stream_ptr()
    H = W = a.size
    V, GW, GH, Lz = a.views, 16, 16, 8
    gen = torch.Generator(device=DEV).manual_seed(0)
    grids = (bilagrid.identity_grids(V, GW, GH, Lz, DEV) + 0.05 * torch.randn(V, 12, Lz, GH, GW, device=DEV, generator=gen)).contiguous()
    report = [f"Bilateral-grid colour compensation (gcx_bilagrid_*), python scripts/bench_bilagrid.py --size {H} --views {V} --gaussians {a.gaussians}"
              + (f" --ab-lib {os.path.relpath(a.ab_lib, ROOT)}  (make -C gaussctrl_amd/csrc ../libbilagrid_nostage.so)" if ab is not None else ""),
              f"device: {torch.cuda.get_device_name(0)}",
              f"grids: {V} views x 12 x {Lz} x {GH} x {GW} ({grids.numel() * 4 / 1e6:.2f} MB); images {H} x {W}", ""]
    dims = (L.i32(H), L.i32(W), L.i32(V), L.i32(GW), L.i32(GH), L.i32(Lz))
    P = syn.make_gaussians(a.gaussians, seed=0, scale_mean=0.01)
    tp = [torch.tensor(P[k], device=DEV, requires_grad=True) for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")]
    bg = torch.zeros(3, device=DEV)

    for C in (1, 8):
        idx = [(7 * c + 3) % V for c in range(C)]
        cidx = (L.i32 * C)(*idx)
        report.append(f"C = {C} (views {idx})")
        both_ms = {}
        for kind in ("smooth", "uniform"):
            rgb = smooth_images(C, H, W, gen) if kind == "smooth" else (torch.rand(C, H, W, 3, device=DEV, generator=gen) * 1.3 - 0.15).contiguous()
            v_out = torch.randn(C, H, W, 3, device=DEV, generator=gen)
            out = torch.empty_like(rgb); v_rgb = torch.empty_like(rgb); v_grids = torch.empty_like(grids)

            def fwd():
                L.check(lib.gcx_bilagrid_slice_fwd_views(L.i32(C), *dims, L.ptr(grids), L.ptr(rgb), cidx, L.ptr(out), st), "gcx_bilagrid_slice_fwd_views")

            def fwd_direct():
                L.check(ab.gcx_bilagrid_slice_fwd_views(L.i32(C), *dims, L.ptr(grids), L.ptr(rgb), cidx, L.ptr(out), st), "A/B forward")

            def bwd_direct():
                v_grids.zero_()
                L.check(ab.gcx_bilagrid_slice_bwd_views(L.i32(C), *dims, L.ptr(grids), L.ptr(rgb), cidx, L.ptr(v_out), L.ptr(v_grids), L.ptr(v_rgb), st),
                        "A/B backward")

            def bwd():
                v_grids.zero_()
                L.check(lib.gcx_bilagrid_slice_bwd_views(L.i32(C), *dims, L.ptr(grids), L.ptr(rgb), cidx, L.ptr(v_out), L.ptr(v_grids), L.ptr(v_rgb), st),
                        "gcx_bilagrid_slice_bwd_views")

            def both():
                fwd(); bwd()

            tg = grids.clone().requires_grad_(True)
            tr = rgb.clone().requires_grad_(True)
            tidx = torch.tensor(idx, device=DEV)

            def composed():
                tg.grad = None; tr.grad = None
                torch_slice(tg, tr, tidx).backward(v_out)

            def composed_fwd():
                with torch.no_grad():
                    torch_slice(tg, tr, tidx)

            both(); composed()
            torch.cuda.synchronize()
            e_out = float((out - torch_slice(tg.detach(), tr.detach(), tidx)).abs().max() / out.abs().max())
            e_g = float((v_grids - tg.grad).abs().max() / tg.grad.abs().max())
            e_r = float((v_rgb - tr.grad).abs().max() / tr.grad.abs().max())
            fns = {"fwd": fwd, "bwd": bwd, "both": both, "composed_fwd": composed_fwd, "composed": composed}
            if ab is not None:
                fns.update(fwd_direct=fwd_direct, bwd_direct=bwd_direct)
            t = alternate(fns)
            mb, mc = statistics.median(t["both"]), statistics.median(t["composed"])
            both_ms[kind] = mb
            report += [f" {kind} images: slice",
                       line("forward (grid values from the slab staged in LDS)", t["fwd"]),
                       line("backward (zeroing of v_grids included)", t["bwd"]), line("forward + backward", t["both"]),
                       line("torch: grid_sample + matmul, forward only", t["composed_fwd"]), line("torch: grid_sample + matmul + autograd", t["composed"]),
                       *([line("A/B: forward, vertex reads through L1 / L2", t["fwd_direct"]),
                          line("A/B: backward, vertex reads through L1 / L2", t["bwd_direct"])] if ab is not None else []),
                       f"  kernels / torch = {mb / mc:.3f}; against torch float32: out {e_out:.2e}, v_grids {e_g:.2e}, v_rgb {e_r:.2e} of the maximum"]

        # ---- total variation (does not depend on C; reported once)
        if C == 1:
            tv = torch.empty(1, device=DEV); vg = torch.zeros_like(grids)
            nbytes = lib.gcx_bilagrid_tv_workspace_bytes(L.i32(V), L.i32(GW), L.i32(GH), L.i32(Lz))
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)

            def tv_kernel():
                vg.zero_()
                L.check(lib.gcx_bilagrid_tv_fwd_bwd(L.i32(V), L.i32(GW), L.i32(GH), L.i32(Lz), L.ptr(grids), L.f32(10.0), L.ptr(tv), L.ptr(vg), L.ptr(ws),
                                                    ctypes.c_size_t(nbytes), st), "gcx_bilagrid_tv_fwd_bwd")

            tg2 = grids.clone().requires_grad_(True)

            def tv_torch():
                tg2.grad = None
                (10.0 * torch_tv(tg2)).backward()

            tv_kernel(); tv_torch()
            torch.cuda.synchronize()
            e_v = abs(float(tv) - float(torch_tv(grids))) / float(torch_tv(grids))
            e_g = float((vg - tg2.grad).abs().max() / tg2.grad.abs().max())
            t = alternate({"kernel": tv_kernel, "torch": tv_torch})
            report += [f" total variation of all {V} grids, value + gradient (the zeroing of the gradient buffer included)",
                       line("gcx_bilagrid_tv_fwd_bwd", t["kernel"]), line("torch: index differences + autograd", t["torch"]),
                       f"  kernel / torch = {statistics.median(t['kernel']) / statistics.median(t['torch']):.3f}; value {e_v:.2e}, gradient {e_g:.2e} apart"]

        # ---- the step it sits beside: fused render + loss + backward of the same C views
        cams = [camera_to_gsplat(c2w, 540.0, 540.0, W / 2, H / 2, W, H) for c2w in syn.make_cameras(C, seed=1)]
        target = torch.rand(C, H, W, 3, device=DEV, generator=gen)

        def step():
            for p in tp:
                p.grad = None
            img, _, _ = ops.render_views(*tp, cams, bg, False, 3, None)
            l1_ssim_loss_views(img, target, 0.2).sum().backward()

        t = alternate({"step": step})
        report += [f" the step beside it: render_views + l1_ssim_loss_views + backward, {a.gaussians} Gaussians, {C} view(s)", line("fused render + loss step", t["step"]),
                   f"  slice forward + backward (smooth images) is {100.0 * both_ms['smooth'] / statistics.median(t['step']):.1f} % of it", ""]
    text = "\n".join(report) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

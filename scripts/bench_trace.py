"""Edit-region tracing at the raster workload's launch set (1 M synthetic Gaussians, 8 cameras, 512 x 512: the configuration of
profiles/absgrad_cost.txt): what the two new hot paths cost against what a caller could compose from the existing operators.

  1. compositing stage: ONE gc_trace_mask_views launch over the 8 views' lists (k_trace_mask, csrc/raster_trace.hip) against the composed
     form on the SAME lists -- per view a 2-channel gc_rasterize_nd_fwd + gc_rasterize_nd_bwd with colors = 1 and v_out = (mask, 1), whose
     v_colors are the same sums (plus the images, final_Ts / final_index and six geometry partials per pair nobody reads).  The zeroing of
     the outputs is inside both timings.  Projection, depth order and binning are shared and outside both.
  2. gc_adam_step_rows at 10 % and 100 % selected rows against gc_adam_step, on the [N, 45] tensor (features_rest) and on [N, 3].

5 warm-up + 20 timed repetitions each, ALTERNATING, device events around every repetition, median and min reported.  No speed bar is fixed:
the numbers are recorded as measured.

    python scripts/bench_trace.py [--n 1000000] [--views 8] [--out profiles/trace_bench.txt]

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
    return f"  {name:<34s} median {statistics.median(ms):8.3f} ms   min {min(ms):8.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench.txt"))
    a = ap.parse_args()
    lib = L.lib()
    st = L.stream_ptr()
    N, C, H, W = a.n, a.views, a.size, a.size
    P = syn.make_gaussians(N, seed=0, scale_mean=0.01)
    tp = [torch.tensor(P[k], device=DEV) for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")]
    cams = [camera_to_gsplat(c2w, 540.0, 540.0, W / 2, H / 2, W, H) for c2w in syn.make_cameras(C, seed=1)]
    with torch.no_grad():
        fr = ops._views_front(*tp, cams, 0, None)
    cnt = fr.cnt.cpu()
    M = int(cnt.sum())
    masks = torch.zeros(C, H, W, device=DEV)
    masks[:, :, :W // 2] = 1.0
    tb = fr.tb
    report = [f"Edit-region tracing (gc_trace_mask_views / gc_adam_step_rows), python scripts/bench_trace.py --n {N} --views {C} --size {H}",
              f"device: {torch.cuda.get_device_name(0)}",
              f"scene: {N} Gaussians, {C} cameras, {H} x {W}, half-plane masks; {M} (tile, Gaussian) list entries over the views", ""]

    # ---- 1. the compositing stage
    w_in = torch.empty(N, device=DEV); w_all = torch.empty(N, device=DEV)

    def trace():
        w_in.zero_(); w_all.zero_()
        L.check(lib.gc_trace_mask_views(L.i32(C), L.i64(N), L.i64(fr.M_cap), L.i32(fr.shared_op), L.i32(H), L.i32(W), L.i32(tb[0]), L.i32(tb[1]),
                                        L.ptr(fr.ids_s), L.ptr(fr.bins), L.ptr(fr.xys), L.ptr(fr.conics), L.ptr(fr.opac), L.ptr(masks), L.ptr(w_in),
                                        L.ptr(w_all), st), "gc_trace_mask_views")

    ones2 = torch.ones(N, 2, device=DEV); bg2 = torch.zeros(2, device=DEV)
    v_out = torch.stack([masks, torch.ones_like(masks)], -1).contiguous()              # [C, H, W, 2]
    img = torch.empty(H, W, 2, device=DEV); fT = torch.empty(H, W, device=DEV); fi = torch.empty(H, W, dtype=torch.int32, device=DEV)
    vbuf = torch.empty(N * 8, device=DEV)                                               # v_xy 2 + v_conic 3 + v_colors 2 + v_opacity 1
    v_xy, v_conic, v_col, v_op = vbuf[:2 * N], vbuf[2 * N:5 * N], vbuf[5 * N:7 * N], vbuf[7 * N:]
    c_in = torch.empty(N, device=DEV); c_all = torch.empty(N, device=DEV)

    def composed():
        c_in.zero_(); c_all.zero_()
        for c in range(C):
            ids, bins, xys, conics = fr.ids_s[c], fr.bins[c], fr.xys[c], fr.conics[c]
            L.check(lib.gc_rasterize_nd_fwd(L.i32(H), L.i32(W), L.i32(tb[0]), L.i32(tb[1]), L.i32(2), L.ptr(ids), L.ptr(bins), L.ptr(xys), L.ptr(conics),
                                            L.ptr(ones2), L.ptr(fr.opac), L.ptr(bg2), L.ptr(img), L.ptr(fT), L.ptr(fi), st), "gc_rasterize_nd_fwd")
            vbuf.zero_()
            L.check(lib.gc_rasterize_nd_bwd(L.i32(H), L.i32(W), L.i32(tb[0]), L.i32(tb[1]), L.i64(N), L.i32(2), L.ptr(ids), L.ptr(bins), L.ptr(xys),
                                            L.ptr(conics), L.ptr(ones2), L.ptr(fr.opac), L.ptr(bg2), L.ptr(fT), L.ptr(fi), L.ptr(v_out[c]), None,
                                            L.ptr(v_xy), L.ptr(v_conic), L.ptr(v_col), L.ptr(v_op), st), "gc_rasterize_nd_bwd")
            vc = v_col.view(N, 2)
            c_in.add_(vc[:, 0]); c_all.add_(vc[:, 1])

    assert fr.shared_op == 1
    trace(); composed()
    torch.cuda.synchronize()
    scale = float(c_all.abs().max())
    err = max(float((w_in - c_in).abs().max()), float((w_all - c_all).abs().max())) / scale
    t = alternate({"trace": trace, "composed": composed})
    mt, mc = statistics.median(t["trace"]), statistics.median(t["composed"])
    algo = M * 28 + C * H * W * 4 + N * 8
    report += ["1. compositing stage over the same lists (the zeroing of the outputs included)",
               line("gc_trace_mask_views, one launch", t["trace"]), line(f"composed: {C} x (nd fwd + nd bwd, C=2)", t["composed"]),
               f"  trace / composed = {mt / mc:.3f}; the sums agree to {err:.2e} of max(w_all)",
               f"  algorithmic bytes M x 28 + HW x 4 x views + N x 8 = {algo / 1e6:.1f} MB -> {algo / mt / 1e6:.1f} GB/s at the median", ""]

    # ---- 2. the row-masked Adam
    g = torch.Generator(device=DEV).manual_seed(0)
    hyper = (L.f32(1e-3), L.f32(0.9), L.f32(0.999), L.f32(1e-15), L.i32(3))
    report.append("2. Adam on [N, rf] float32 (param, grad and both moments: 16 bytes read and 12 written per stepped element)")
    for rf in (45, 3):
        p = torch.randn(N, rf, device=DEV, generator=g); gr = torch.randn(N, rf, device=DEV, generator=g) * 1e-2
        m = torch.zeros(N, rf, device=DEV); v = torch.zeros(N, rf, device=DEV)
        sel10 = (torch.rand(N, device=DEV, generator=g) < 0.1).to(torch.uint8)
        sel100 = torch.ones(N, dtype=torch.uint8, device=DEV)

        def full():
            L.check(lib.gc_adam_step(L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), L.i64(N * rf), *hyper, st), "gc_adam_step")

        def rows(sel):
            return lambda: L.check(lib.gc_adam_step_rows(L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), L.i64(N), L.i32(rf), L.ptr(sel), *hyper, st),
                                   "gc_adam_step_rows")
        t = alternate({"full": full, "rows100": rows(sel100), "rows10": rows(sel10)})
        mf = statistics.median(t["full"])
        report += [f"  rf = {rf} ({N * rf * 28 / 1e6:.0f} MB when every element steps)", "  " + line("gc_adam_step", t["full"]),
                   "  " + line("gc_adam_step_rows, 100 % selected", t["rows100"]) + f"   x{statistics.median(t['rows100']) / mf:.3f}",
                   "  " + line(f"gc_adam_step_rows, {100.0 * float(sel10.float().mean()):.1f} % selected", t["rows10"])
                   + f"   x{statistics.median(t['rows10']) / mf:.3f}"]
    text = "\n".join(report) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

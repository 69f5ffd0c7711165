"""How close does the round-2 group-statistics epilogue come to the bar of test_conv_output_group_statistics (2e-5 relative to |ref| + 1e-3 max|ref|) over RANDOM
bias / row-vector draws (the test draws them from the unseeded global generator)?  python scripts/diag/group_stats_margin.py <draws> [mt]"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gaussctrl_amd.sd import ops
from gaussctrl_amd.sd.weights import conv3x3_weight

draws = int(sys.argv[1]) if len(sys.argv) > 1 else 300
mt = int(sys.argv[2]) if len(sys.argv) > 2 else 4
dev = "cuda:0"
print("initial cuda seed", torch.cuda.initial_seed())
for dt in (torch.float16, torch.bfloat16):
    for (B, H, Cin, Cout) in ((14, 8, 1280, 1280), (3, 16, 1280, 1280)):
        g = torch.Generator(device="cpu").manual_seed(1)
        x = (torch.randn((B, H, H, Cin), generator=g)).to(dt).to(dev)
        g = torch.Generator(device="cpu").manual_seed(2)
        w = conv3x3_weight((torch.randn((Cout, Cin, 3, 3), generator=g) * (9 * Cin) ** -0.5).to(dt).to(dev), dt)
        worst, worst_abs, over = 0.0, 0.0, 0
        ops.configure(gemm_variant=mt << ops.GC_GEMM_VAR_MT_SHIFT)
        for it in range(draws):
            b = torch.randn(Cout, device=dev); rv = torch.randn(B, Cout, device=dev)
            gs = torch.zeros(B, 32, 2, device=dev)
            out = ops.conv3x3(x, w, b, rowvec=rv, group_stats=gs)
            o = out.double().reshape(B, H * H, 32, Cout // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
            ref = torch.stack([o.sum(-1), (o * o).sum(-1)], -1)
            err = (gs.double() - ref).abs()
            rel = err / (ref.abs() + 1e-3 * ref.abs().max())
            r = float(rel.max())
            if r > worst:
                worst = r; idx = tuple((rel == rel.max()).nonzero()[0].tolist()); worst_abs = float(err[idx]); wref = float(ref[idx]); wmax = float(ref.abs().max())
            over += r >= 2e-5
        ops.configure(gemm_variant=0)
        print(f"{dt} B{B} {H}x{H}: worst rel {worst:.3e} of bar 2e-5 (abs err {worst_abs:.4g} on ref {wref:.6g}, max|ref| {wmax:.5g}); {over} of {draws} draws over the bar")

"""k_attn5 (the default D = 40 kernel; GC_ATTN_VAR_K4 selects k_attn4) vs k_attn4 and a torch fp32 reference: parity at small sizes, timing at the production launch
(L = 4096, 8 heads x D = 40, B = 6 frames, 5 K/V sets incl. a cached reference bank).   python scripts/attn5_check.py"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gaussctrl_amd.sd import ops

DEV = "cuda:0"


def ref_attn(q, k, v, heads, scale):
    B, L, C = q.shape
    D = C // heads
    qh = q.float().view(B, L, heads, D).transpose(1, 2); kh = k.float().view(B, -1, heads, D).transpose(1, 2)
    vh = v.float().view(B, -1, heads, D).transpose(1, 2)
    p = (qh @ kh.transpose(-1, -2) * scale).softmax(-1)
    return (p @ vh).transpose(1, 2).reshape(B, L, C)

K4 = ops.GC_ATTN_VAR_K4


def run(variant, *a, **kw):
    ops.configure(attn_variant=variant)
    try:
        return ops.attention(*a, **kw)
    finally:
        ops.configure(attn_variant=0)


def parity(dt, f, L, heads, coeff, spike=False, pre=False):
    D = 40
    B, C = 2 * f, heads * D
    g = torch.Generator(device=DEV).manual_seed(L + f)
    q = torch.randn(B, L, C, device=DEV, generator=g).to(dt); k = torch.randn(B, L, C, device=DEV, generator=g).to(dt)
    v = torch.randn(B, L, C, device=DEV, generator=g).to(dt)
    if spike:
        k[:, 200, :] = q[:, 17, :] * 40.0
    vt = v.transpose(1, 2).contiguous()
    scale = D ** -0.5
    sets = ([(-1, coeff)] if coeff != 0 else []) + [(r, (1 - coeff) / 4) for r in range(4)]
    qq = (q.float() * (scale * 1.4426950408889634)).to(dt) if pre else q
    sc = float(np.log(2.0)) if pre else scale
    ref = coeff * ref_attn(qq, k, v, heads, sc)
    for r in range(4):
        idx = torch.arange(B, device=DEV) // f * f + r
        ref = ref + (1 - coeff) / 4 * ref_attn(qq, k[idx], v[idx], heads, sc)
    a4 = run(K4, qq, k, vt, heads, sets, f, Lk=L, q_prescaled=pre).float()
    a5 = run(0, qq, k, vt, heads, sets, f, Lk=L, q_prescaled=pre).float()
    e4 = float((a4 - ref).norm() / ref.norm()); e5 = float((a5 - ref).norm() / ref.norm())
    d45 = float((a5 - a4).abs().max())
    print(f"{str(dt):16s} f={f} L={L} heads={heads} coeff={coeff} spike={spike} pre={pre}: rel L2 k_attn4 {e4:.3e}  k_attn5 {e5:.3e}  max|a5-a4| {d45:.3e}"
          f"  finite={bool(torch.isfinite(a5).all())}")
    return e4, e5


def timing(dt, variant, iters=20, qscale=0.5):
    f, L, heads, D = 3, 4096, 8, 40
    B, C = 2 * f, heads * D
    g = torch.Generator(device=DEV).manual_seed(0)
    qk = (torch.randn(B, L, 2 * C, device=DEV, generator=g) * qscale).to(dt)      # logits of a few units: inside f16's P range
    q, k = qk[..., :C], qk[..., C:]
    vt = torch.randn(B, C, L, device=DEV, generator=g).to(dt)
    kr = torch.randn(8, L, 2 * C, device=DEV, generator=g).to(dt)[..., C:]
    vtr = torch.randn(8, C, L, device=DEV, generator=g).to(dt)
    sets = [(-1, 0.6)] + [(r, 0.1) for r in range(4)]
    for _ in range(3):
        run(variant, q, k, vt, heads, sets, f, Lk=L, kref=kr, vtref=vtr, ref_fph=4, q_prescaled=True)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops.configure(attn_variant=variant)
    s.record()
    for _ in range(iters):
        ops.attention(q, k, vt, heads, sets, f, Lk=L, kref=kr, vtref=vtr, ref_fph=4, q_prescaled=True)
    e.record(); torch.cuda.synchronize()
    ops.configure(attn_variant=0)
    us = s.elapsed_time(e) * 1e3 / iters
    fl = 4.0 * B * L * L * C * 5
    print(f"timing {str(dt):16s} qscale {qscale} variant {variant:2d}: {us:8.1f} us   {fl / us / 1e6:7.1f} TF/s   frac of 2.5 PF {fl / us / 1e6 / 2500:.3f}")
    return us


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "abl":           # timing ablations of k_attn5 (results wrong by construction)
        names = {0: "everything (instrumented build)", 1: "no v_exp", 2: "no exp units (no v_exp, no v_cvt_pk)", 4: "no s_barrier", 8: "no LDS-DMA",
                 16: "no LDS fragment reads", 24: "no DMA, no fragment reads", 26: "MFMA only (+ barrier)", 30: "MFMA only",
                 32: "units read a constant, not S", 64: "units write a sink, not P", 96: "units detached from both MFMAs", 120: "detached units, no LDS traffic",
                 192: "units write a sink, P = non-zero constants", 130: "no units, P = non-zero constants", 2 + 128 + 24: "no units, P constants, no LDS traffic"}
        timing(torch.bfloat16, 0)
        timing(torch.bfloat16, 0)
        for bits, nm in names.items():
            print(f"ablation {bits:3d} {nm:46s}", end=" ")
            timing(torch.bfloat16, (bits or 256) << ops.GC_ATTN_VAR_ABL_SHIFT)          # (256: no ablation bit set, instrumented instantiation)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "shift":          # f16: offset shift c (GC_ATTN_VAR_CSHIFT_*): fallback rate (time) and accuracy
        import numpy as np
        for qs in (0.35, 0.6, 1.0):
            for c in (0, 4, 8, 12, 14):
                f, L, heads, D = 4, 1024, 8, 40
                B, C = 2 * f, heads * D
                g = torch.Generator(device=DEV).manual_seed(1)
                q = (torch.randn(B, L, C, device=DEV, generator=g) * qs).half(); k = torch.randn(B, L, C, device=DEV, generator=g).half()
                v = torch.randn(B, L, C, device=DEV, generator=g).half(); vt = v.transpose(1, 2).contiguous()
                sets = [(-1, 0.6)] + [(r, 0.1) for r in range(4)]
                ref = 0.6 * ref_attn(q, k, v, heads, float(np.log(2.0)))
                for r in range(4):
                    idx = torch.arange(B, device=DEV) // f * f + r
                    ref = ref + 0.1 * ref_attn(q, k[idx], v[idx], heads, float(np.log(2.0)))
                got = run(c << ops.GC_ATTN_VAR_CSHIFT_SHIFT, q, k, vt, heads, sets, f, Lk=L, q_prescaled=True).float()
                err = float((got - ref).norm() / ref.norm())
                print(f"qscale {qs} shift {c:2d}: rel L2 {err:.3e}", end="   ")
                timing(torch.float16, c << ops.GC_ATTN_VAR_CSHIFT_SHIFT, iters=5, qscale=qs)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "f16":            # why is f16 slower at wide logit spreads?  safe kernel, k_attn4, k_attn5
        for qs in (0.25, 0.5, 0.7):
            for v in (ops.GC_ATTN_VAR_ONLINE_ONLY, K4, 0):
                timing(torch.float16, v, iters=5, qscale=qs)
                timing(torch.bfloat16, v, iters=5, qscale=qs)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "time":          # timing only (PMC passes: python scripts/pmc.py 'k_attn' -- python scripts/attn5_check.py time 16)
        timing(torch.bfloat16, int(sys.argv[2]), iters=3)
        sys.exit(0)
    ok = True
    for dt in (torch.bfloat16, torch.float16):
        for (f, L, heads, coeff, spike, pre) in [(4, 256, 2, 0.6, False, False), (5, 512, 2, 0.6, False, True), (5, 256, 1, 0.0, False, True),
                                                 (4, 256, 2, 0.6, True, False), (4, 1024, 8, 0.6, False, True)]:
            e4, e5 = parity(dt, f, L, heads, coeff, spike, pre)
            ok = ok and e5 <= max(1.5 * e4, 2e-3 if dt == torch.float16 else 1.2e-2)
    print("PARITY", "OK" if ok else "FAIL")
    for dt in (torch.bfloat16, torch.float16):
        for v in (K4, 0, K4, 0):
            timing(dt, v)
    for qs in (0.25, 0.35):
        for v in (K4, 0):
            timing(torch.float16, v, qscale=qs)
    for v in (0, K4, 0, K4):       # k_attn5, k_attn4
        timing(torch.bfloat16, v)

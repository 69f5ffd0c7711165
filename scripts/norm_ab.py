"""A/B tool for csrc/dn_norm.hip: every entry point of the file on seeded inputs, outputs to an .npz; a second mode compares two such
files (two builds of the library on the same machine).

    python scripts/norm_ab.py run OUT.npz
    python scripts/norm_ab.py compare A.npz B.npz

Outputs that involve no float atomic must be byte-equal.  gc_dn_group_stats and concat_add(group_stats=) end in float atomics whose order
varies from run to run: each file's sums are held to the fp64 sums of the stored tensor with the bar of test_concat_add_with_statistics
(the reference and its scale are computed on the CPU and travel in the file).  Statistics fed INTO a kernel (group sums, slab partials
of the GroupNorm shapes) are computed on the CPU, so both builds see the same bytes."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
G = 32
GN_SHAPES = [(2, 256, 320), (2, 36, 960), (1, 16, 1920), (2, 100, 2560), (2, 64, 1280)]     # full lanes; idle threads + tail slab; lanes = 1; two slices; small form
LN_SHAPES = [(5, 64), (77, 640), (1001, 1280)]
CAT_SHAPES = [(2, 16, 1280, 640), (2, 18, 320, 320)]                                         # the second: HW 324, 3 lanes, a last slab of 4 pixels


def rand(shape, dt, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(dt).to(DEV)


def group_sums(x, groups):
    """[B, L, C] -> fp64 (sum, sum^2) and their scale (sum |x|, sum x^2), both [B, G, 2], on the CPU"""
    B, L, C = x.shape
    t = x.double().cpu().reshape(B, L, groups, C // groups).permute(0, 2, 1, 3).reshape(B, groups, -1)
    return torch.stack([t.sum(-1), (t * t).sum(-1)], -1), torch.stack([t.abs().sum(-1), (t * t).sum(-1)], -1)


def cpu_parts(ops, x, groups, rows):
    """ChanParts of x [B, HW, C] as a producer with `rows`-pixel slabs restarting at every batch and one column tile would leave them"""
    B, HW, C = x.shape
    ns = (HW + rows - 1) // rows
    buf = torch.zeros(B, ns, groups, 2, 2, dtype=torch.float32)
    for s in range(ns):
        buf[:, s, :, 0, :] = group_sums(x[:, s * rows:(s + 1) * rows], groups)[0].float()
    return ops.ChanParts(buf.to(DEV), rows, ns, 1, C, groups)


def run(path):
    from gaussctrl_amd.sd import ops
    ops.DEBUG_FILL = 0.0          # a producer writes only the halves of ChanParts that exist; the rest of the buffer is torch.empty
    out = {}

    def put(key, t):
        t = t.detach().contiguous().cpu()
        out[key] = (t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t).numpy()

    def put_stats(key, got, stored):
        ref, scale = group_sums(stored.reshape(stored.shape[0], -1, stored.shape[-1]), got.shape[-2])
        put("tol:" + key, got); out["ref:" + key] = ref.numpy(); out["scale:" + key] = scale.numpy()

    for dt in (torch.bfloat16, torch.float16):
        d = "bf16" if dt == torch.bfloat16 else "f16"
        for B, HW, C in GN_SHAPES:
            k = f"{d}/gn{B}x{HW}x{C}"
            x = rand((B, HW, C), dt, 1, 2.0, 1.0)
            gamma = rand((C,), torch.float32, 2); beta = rand((C,), torch.float32, 3)
            gs = group_sums(x, G)[0].float().to(DEV)
            parts = cpu_parts(ops, x, G, 16)
            put(k + "/coef", ops.groupnorm_coef(x, gamma, beta, G, 1e-5))
            put(k + "/coef_parts", ops.groupnorm_coef(x, gamma, beta, G, 1e-5, parts=parts))
            put_stats(k + "/group_stats", ops.group_stats(x, torch.zeros(B, G, 2, device=DEV)), x)
            for silu in (False, True):
                ks = k + ("/silu" if silu else "/plain")
                for inv in (False, True):           # batch-invariant planning takes the three-kernel form where the default takes k_gn_small
                    ops.configure(batch_invariant=inv)
                    put(ks + ("/groupnorm_inv" if inv else "/groupnorm"), ops.groupnorm(x, gamma, beta, G, 1e-5, silu))
                ops.configure(batch_invariant=False)
                put(ks + "/apply", ops.groupnorm_apply(x, gs, gamma, beta, G, 1e-5, silu))
                put(ks + "/apply_parts", ops.groupnorm(x, gamma, beta, G, 1e-5, silu, parts=parts))
                for a_scale in (127, 125):
                    put(ks + f"/apply_fp8_{a_scale}", ops.groupnorm_apply_fp8(x, gs, gamma, beta, G, 1e-5, silu, a_scale))
                    put(ks + f"/apply_parts_fp8_{a_scale}", ops.groupnorm_apply_parts_fp8(x, parts, gamma, beta, G, 1e-5, silu, a_scale))
        for M, C in LN_SHAPES:
            x = rand((M, C), dt, 4, 1.5, 0.5)
            gamma = rand((C,), torch.float32, 5); beta = rand((C,), torch.float32, 6)
            put(f"{d}/ln{M}x{C}", ops.layernorm(x, gamma, beta))
            for a_scale in (127, 125):
                put(f"{d}/ln{M}x{C}/fp8_{a_scale}", ops.layernorm_fp8(x, gamma, beta, 1e-5, a_scale))
        for B, H, C1, C2 in CAT_SHAPES:
            k = f"{d}/cat{B}x{H}x{C1}x{C2}"
            a = rand((B, H, H, C1), dt, 7, 1.0, 2.0); b = rand((B, H, H, C2), dt, 8); c = rand((B, H, H, C2), dt, 9)
            gamma = rand((C1 + C2,), torch.float32, 2); beta = rand((C1 + C2,), torch.float32, 3)
            for cc, kc in ((c, "/abc"), (None, "/ab")):
                put(k + kc, ops.concat_add(a, b, cc))
                gs = torch.zeros(B, G, 2, device=DEV)
                cat = ops.concat_add(a, b, cc, group_stats=gs)
                put(k + kc + "/with_stats", cat); put_stats(k + kc + "/stats", gs, cat)
                cat, parts = ops.concat_add(a, b, cc, chan_parts=True)
                assert parts is not None, "this shape must take the partials path"
                put(k + kc + "/with_parts", cat); put(k + kc + "/parts", parts.buf)
                for silu in (False, True):
                    put(k + kc + f"/gn_parts{int(silu)}", ops.groupnorm(cat, gamma, beta, G, 1e-5, silu, parts=parts))
                    put(k + kc + f"/gn_parts_fp8_{int(silu)}", ops.groupnorm_apply_parts_fp8(cat, parts, gamma, beta, G, 1e-5, silu, 126))
                put(k + kc + "/coef_parts", ops.groupnorm_coef(cat.reshape(B, H * H, C1 + C2), gamma, beta, G, 1e-5, parts=parts))
        # elementwise
        a = rand((4, 10, 10, 64), dt, 10); b = rand((4, 10, 10, 64), dt, 11)
        put(f"{d}/axpby", ops.axpby(a, 0.5, b, 2.0, act=1)); put(f"{d}/axpby1", ops.axpby(a, 1.5))
        put(f"{d}/cast", ops.cast_f32(rand((7, 1280), torch.float32, 12), dt, silu=True))
        put(f"{d}/softmax", ops.softmax_rows_(rand((37, 300), dt, 13, 3.0), 0.3))
        f, H = 3, 8
        eps = rand((2 * f, H, H, 8), torch.float32, 14); lat = rand((f, H, H, 4), torch.float32, 15)
        xin = torch.full((2 * f, H, H, 8), 7.0, dtype=dt, device=DEV)
        ops.cfg_ddim_step(eps, lat, xin, 5.0, True, 0.3, 0.45, 2)
        put(f"{d}/ddim_lat", lat); put(f"{d}/ddim_xin", xin)
        put(f"{d}/disparity", ops.depth_to_disparity(rand((24, 40), torch.float32, 16).abs() + 0.5, dt))
    e = rand((16, 24, 4), torch.float32, 17); u = rand((16, 24, 3), torch.float32, 18); m = rand((16, 24), torch.float32, 19).sigmoid()
    put("mask_composite", ops.mask_composite(e, u, m)); put("mask_composite_nomask", ops.mask_composite(e))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"norm_ab: {len(out)} arrays -> {path}")


def stats_use(got, ref, scale):
    """share of the bar of tests/test_denoise_kernels_gpu.py::_stats_close in use (< 1 passes)"""
    err = np.abs(got.astype(np.float64) - ref)
    return float(np.minimum(err / (2e-5 * (np.abs(ref) + 1e-3 * np.abs(ref).max())), err / (2e-6 * np.maximum(scale, 1e-6))).max())


def compare(pa, pb):
    A, Bz = np.load(pa), np.load(pb)
    bad = sorted(set(A.files) ^ set(Bz.files))
    nexact = ntol = 0
    worst = 0.0
    for k in A.files:
        if k in bad or k.startswith(("ref:", "scale:")):
            continue
        if k.startswith("tol:"):
            ntol += 1
            ua, ub = (stats_use(z[k], A["ref:" + k[4:]], A["scale:" + k[4:]]) for z in (A, Bz))
            worst = max(worst, ua, ub)
            if not (ua < 1.0 and ub < 1.0):
                bad.append(f"{k}: {ua:.3f} / {ub:.3f} of the statistics bar")
        else:
            nexact += 1
            if A[k].shape != Bz[k].shape or A[k].tobytes() != Bz[k].tobytes():
                ne = np.argwhere(A[k] != Bz[k]) if A[k].shape == Bz[k].shape else np.zeros((0, 0))
                bad.append(f"{k}: {len(ne)} of {A[k].size} elements differ, first at {ne[:3].tolist()}")
    print(f"norm_ab: {nexact} outputs compared byte for byte, {ntol} atomic sums against fp64 (worst {worst:.3f} of the bar)")
    for line in bad:
        print("MISMATCH", line)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)

"""An independent restatement, on the CPU, of the contract of include/gaussctrl_bilagrid.h: the slice through F.grid_sample on 5-D input
(align_corners=True, padding_mode="border") with autograd for both gradients, and the total variation as index differences.  Evaluated in
float64 it is the reference of tests/test_bilagrid_gpu.py; evaluated in float32 on the same inputs it shows what error the number format
alone leaves, and that error (x 16) is the bar of the GPU kernels.

Inputs are seeded: grids are identity + 0.3 randn, rgb is uniform in [-0.15, 1.15] (both clamps of the luma axis are active), and rgb is
nudged until no pixel's z = luma (L - 1) lies within 1e-4 of an integer inside the grid's range (in float64): dA/dz jumps from one cell to
the next, so that the reference alone decides the cell.  No pixel is left out of any comparison.

A plain helper like _margins.py; results are cached per case and never modified."""
import torch
import torch.nn.functional as F

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
LUMA = (0.299, 0.587, 0.114)


def make_grids(V, GW, GH, L, seed):
    g = torch.Generator().manual_seed(seed)
    eye = torch.tensor(IDENTITY, dtype=torch.float32).reshape(1, 12, 1, 1, 1)
    return (eye + 0.3 * torch.randn(V, 12, L, GH, GW, generator=g)).contiguous()


def make_inputs(C, H, W, GW, GH, L, V, seed):
    """(grids [V,12,L,GH,GW], rgb [C,H,W,3], v_out [C,H,W,3]) float32 on the CPU"""
    g = torch.Generator().manual_seed(seed + 1000)
    grids = make_grids(V, GW, GH, L, seed)
    rgb = torch.rand(C, H, W, 3, generator=g) * 1.3 - 0.15
    v_out = torch.randn(C, H, W, 3, generator=g)
    coef = torch.tensor(LUMA, dtype=torch.float64)
    for _ in range(100):
        z = (rgb.double() * coef).sum(-1) * (L - 1)
        near = ((z - z.round()).abs() < 1e-4) & (z > -0.5) & (z < L - 0.5)
        if not bool(near.any()):
            break
        rgb[near] += 1e-3
    else:
        raise AssertionError("the nudge did not converge")
    return grids, rgb.contiguous(), v_out.contiguous()


def slice_ref(grids, rgb, view_idx, v_out, dtype=torch.float64):
    """-> (out [C,H,W,3], v_grids [V,12,L,GH,GW], v_rgb [C,H,W,3]) in `dtype`, from inputs converted to it"""
    g = grids.detach().to(dtype).clone().requires_grad_(True)          # (a copy: .to() of the same type returns its argument)
    x = rgb.detach().to(dtype).clone().requires_grad_(True)
    C, H, W, _ = x.shape
    xs = 2 * (torch.arange(W, dtype=dtype) + 0.5) / W - 1
    ys = 2 * (torch.arange(H, dtype=dtype) + 0.5) / H - 1
    luma = (x * torch.tensor(LUMA, dtype=dtype)).sum(-1)
    zs = 2 * luma.clamp(0, 1) - 1
    coords = torch.stack([xs[None, None, :].expand(C, H, W), ys[None, :, None].expand(C, H, W), zs], dim=-1)[:, None]      # [C,1,H,W,3]
    A = F.grid_sample(g[list(view_idx)], coords, mode="bilinear", padding_mode="border", align_corners=True)                # [C,12,1,H,W]
    A = A[:, :, 0].permute(0, 2, 3, 1).reshape(C, H, W, 3, 4)
    out = (A[..., :3] * x[..., None, :]).sum(-1) + A[..., 3]
    out.backward(v_out.to(dtype))
    return out.detach(), g.grad.detach(), x.grad.detach()


def tv_ref(grids, dtype=torch.float64):
    """-> (tv scalar, d tv / d grids) in `dtype`"""
    g = grids.detach().to(dtype).clone().requires_grad_(True)
    tv = ((g[..., 1:] - g[..., :-1]) ** 2).mean() + ((g[..., 1:, :] - g[..., :-1, :]) ** 2).mean() + ((g[:, :, 1:] - g[:, :, :-1]) ** 2).mean()
    tv.backward()
    return tv.detach(), g.grad.detach()


def rel_err(got, ref):
    """maximum error over the maximum |reference|"""
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


_SLICE, _TV = {}, {}


def slice_case(name, C, H, W, GW, GH, L, V, view_idx, seed):
    """the inputs, the float64 reference and the float32 restatement's own errors (out, v_grids, v_rgb) of a named case, computed once"""
    if name not in _SLICE:
        grids, rgb, v_out = make_inputs(C, H, W, GW, GH, L, V, seed)
        ref = slice_ref(grids, rgb, view_idx, v_out, torch.float64)
        f32 = slice_ref(grids, rgb, view_idx, v_out, torch.float32)
        _SLICE[name] = dict(grids=grids, rgb=rgb, v_out=v_out, view_idx=list(view_idx), ref=ref, f32_err=tuple(rel_err(a, b) for a, b in zip(f32, ref)))
    return _SLICE[name]


def tv_case(V, GW, GH, L, seed):
    key = (V, GW, GH, L, seed)
    if key not in _TV:
        grids = make_grids(V, GW, GH, L, seed)
        ref = tv_ref(grids, torch.float64)
        f32 = tv_ref(grids, torch.float32)
        _TV[key] = dict(grids=grids, ref=ref, f32_err=tuple(rel_err(a, b) for a, b in zip(f32, ref)))
    return _TV[key]

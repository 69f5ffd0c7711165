"""Bilateral-grid colour compensation for training on edited views (include/gaussctrl_bilagrid.h, csrc/train_bilagrid.hip): what later
splatfacto / gsplat versions call use_bilateral_grid ("Bilateral Guided Radiance Field Processing"; gsplat 1.x lib_bilagrid.py).  The
reference of this project (gsplat 0.1.3, nerfstudio 1.0) has none of it; the formulas are recalled and were not checked against their
source -- the header states them and is the contract.

Every training view owns a small 3D grid of 3x4 colour transforms.  The grid is sliced at (x, y, luma) and applied to the render before
the loss, a total-variation term keeps it smooth, and evaluation never sees it: exposure, white-balance and contrast drift between the
edited views lands in the grids instead of in floaters and view-dependent SH.

  identity_grids(V, GW, GH, L, device)   : [V, 12, L, GH, GW] with every vertex the identity transform;
  bilagrid_apply(grids, rgb, view_idx)   : [C, H, W, 3] images through the grids view_idx names, differentiable in grids and rgb;
  bilagrid_tv_loss(grids)                : the total variation of all grids, differentiable in grids.

Opt-in: GaussCtrlModelConfig.use_bilateral_grid (stand-alone model)."""
from __future__ import annotations

import torch

from . import _lib as L

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def check_shape(shape) -> tuple:
    """bilateral_grid_shape -> (GW, GH, L); anything but three integers of at least 2 is a ValueError"""
    try:
        dims = tuple(shape)
    except TypeError:
        dims = ()
    if len(dims) != 3 or any(isinstance(d, bool) or not isinstance(d, int) or d < 2 for d in dims):
        raise ValueError(f"bilateral_grid_shape must be three integers (GW, GH, L) of at least 2, got {shape!r}")
    return dims


def identity_grids(V: int, GW: int = 16, GH: int = 16, L: int = 8, device="cuda") -> torch.Tensor:
    """[V, 12, L, GH, GW] float32: every vertex of every grid holds [1,0,0,0, 0,1,0,0, 0,0,1,0], the transform that changes nothing"""
    check_shape((GW, GH, L))
    if V < 0:
        raise ValueError(f"identity_grids: V must not be negative, got {V}")
    eye = torch.tensor(IDENTITY, dtype=torch.float32, device=device)
    return eye.reshape(1, 12, 1, 1, 1).repeat(V, 1, L, GH, GW).contiguous()


def refuse_unsupported(model_config, world_size: int) -> None:
    """use_bilateral_grid refuses, rather than half-works, where the grid's gradient would not reach its optimizer"""
    if getattr(model_config, "use_bilateral_grid", False) and world_size > 1:
        raise ValueError("use_bilateral_grid trains on one GPU only (world_size > 1: the grid gradient is not in the flat gradient buffers "
                         "of any train_mode)")


def check_view(image_idx, V: int) -> int:
    """batch["image_idx"] -> the grid it names; an index outside [0, V) is a ValueError"""
    idx = int(image_idx)
    if not 0 <= idx < V:
        raise ValueError(f"use_bilateral_grid: image_idx {idx} is outside [0, {V}): the model was built for {V} training views")
    return idx


def _grid_dims(grids, what):
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"{what}: grids must be [V, 12, L, GH, GW], got {tuple(grids.shape)}")
    V, _, Lz, GH, GW = (int(s) for s in grids.shape)
    return V, GW, GH, Lz


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, rgb, view_idx):
        if not (grids.is_cuda and rgb.is_cuda):
            raise L.GaussCtrlHipError("bilagrid_apply needs GPU tensors (HIP path only; no CPU fallback)")
        V, GW, GH, Lz = _grid_dims(grids, "bilagrid_apply")
        if rgb.dim() != 4 or rgb.shape[3] != 3:
            raise ValueError(f"bilagrid_apply: rgb must be [C, H, W, 3], got {tuple(rgb.shape)}")
        Cn, H, W, _ = (int(s) for s in rgb.shape)
        if len(view_idx) != Cn:
            raise ValueError(f"bilagrid_apply: {Cn} images, {len(view_idx)} view indices")
        g = grids.detach().float().contiguous()
        x = rgb.detach().float().contiguous()
        idx = (L.C.c_int32 * Cn)(*view_idx)
        out = torch.empty(Cn, H, W, 3, dtype=torch.float32, device=x.device)
        L.call("gcx_bilagrid_slice_fwd_views", Cn, H, W, V, GW, GH, Lz, g, x, idx, out)
        ctx.save_for_backward(g, x)
        ctx.view_idx = idx
        return out

    @staticmethod
    def backward(ctx, v_out):
        g, x = ctx.saved_tensors
        V, GW, GH, Lz = _grid_dims(g, "bilagrid_apply")
        Cn, H, W, _ = (int(s) for s in x.shape)
        v = v_out.detach().float().contiguous()
        v_grids = torch.zeros(V, 12, Lz, GH, GW, dtype=torch.float32, device=x.device)
        v_rgb = torch.empty(Cn, H, W, 3, dtype=torch.float32, device=x.device)
        L.call("gcx_bilagrid_slice_bwd_views", Cn, H, W, V, GW, GH, Lz, g, x, ctx.view_idx, v, v_grids, v_rgb)
        return v_grids, v_rgb, None


def bilagrid_apply(grids, rgb, view_idx):
    """grids [V, 12, L, GH, GW], rgb [C, H, W, 3] float32 on the GPU, view_idx: C integers in [0, V) (a list, or a tensor that is read
    back) -> [C, H, W, 3]: image c through the grid view_idx[c] sliced at (x, y, luma of the input).  Differentiable in grids and rgb."""
    if torch.is_tensor(view_idx):
        view_idx = view_idx.reshape(-1).tolist()
    idx = tuple(int(v) for v in view_idx)
    V = int(grids.shape[0]) if grids.dim() == 5 else 0
    for v in idx:
        if not 0 <= v < V:
            raise ValueError(f"bilagrid_apply: view index {v} is outside [0, {V})")
    return _Apply.apply(grids, rgb, idx)


class _TV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        if not grids.is_cuda:
            raise L.GaussCtrlHipError("bilagrid_tv_loss needs GPU tensors (HIP path only; no CPU fallback)")
        V, GW, GH, Lz = _grid_dims(grids, "bilagrid_tv_loss")
        g = grids.detach().float().contiguous()
        tv = torch.zeros(1, dtype=torch.float32, device=g.device)
        v = torch.zeros(V, 12, Lz, GH, GW, dtype=torch.float32, device=g.device)
        nbytes = L.call("gcx_bilagrid_tv_workspace_bytes", V, GW, GH, Lz)
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=g.device)
        L.call("gcx_bilagrid_tv_fwd_bwd", V, GW, GH, Lz, g, 1.0, tv, v, ws, nbytes)
        ctx.save_for_backward(v)
        return tv[0]

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return v * g


def bilagrid_tv_loss(grids):
    """grids [V, 12, L, GH, GW] float32 on the GPU -> scalar: for each of the three spatial axes the mean of the squared forward
    differences over all V grids, summed (value and gradient in one launch pair).  Differentiable in grids."""
    return _TV.apply(grids)

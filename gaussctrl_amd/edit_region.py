"""Edit regions traced onto the Gaussians (include/gaussctrl_trace.h; GaussianEditor's semantic tracing, recalled from the paper).

The masked edit protects the background in image space only: mask_composite pastes the unedited pixels back into every edited view, and
the training that follows still moves every Gaussian.  Here the 2D masks are lifted onto the Gaussians by the compositing weights
alpha * T each one receives from masked against all pixels over all views (trace), the rows above a ratio are picked (select), and the
optimisers step those rows only (train_ops.FusedAdam.row_select); a cull carries the selection along (follow_cull).  Opt-in:
GaussCtrlPipelineConfig.edit_region = "traced"."""
from __future__ import annotations

import torch

from . import _lib as L
from . import gsplat_ops as ops

MODES = ("image", "traced")


def check_mode(mode) -> bool:
    """edit_region -> is it "traced"; anything but the two names is a ValueError"""
    if mode not in MODES:
        raise ValueError(f"edit_region must be one of {MODES}, got {mode!r}")
    return mode == "traced"


@torch.no_grad()
def trace(model, cameras, masks, views_per_launch: int = 8):
    """(w_in, w_all), float32 [N] each: sum over the cameras' pixels of alpha * T * mask and of alpha * T for every Gaussian of `model`
    (a GaussCtrlModel), as the model's evaluation render composites them (rasterize_mode included).  cameras: a list of Cameras of one
    size; masks: one [H, W] tensor per camera (bool or any number type).  views_per_launch cameras share one launch set."""
    from .camera import camera_to_gsplat
    from .gc_model import _antialiased
    if len(cameras) != len(masks):
        raise ValueError(f"edit_region.trace: {len(cameras)} cameras, {len(masks)} masks")
    dev = model.means.device
    N = model.means.shape[0]
    w_in = torch.zeros(N, dtype=torch.float32, device=dev)
    w_all = torch.zeros(N, dtype=torch.float32, device=dev)
    step = max(1, int(views_per_launch))
    for s0 in range(0, len(cameras), step):
        cams = [c.to(dev) for c in cameras[s0:s0 + step]]
        W, H = int(cams[0].width.reshape(-1)[0]), int(cams[0].height.reshape(-1)[0])
        gcams = [camera_to_gsplat(c.camera_to_worlds[0].detach().cpu().numpy(), float(c.fx.reshape(-1)[0]), float(c.fy.reshape(-1)[0]),
                                  float(c.cx.reshape(-1)[0]), float(c.cy.reshape(-1)[0]), int(c.width.reshape(-1)[0]),
                                  int(c.height.reshape(-1)[0])) for c in cams]
        mk = torch.empty(len(cams), H, W, dtype=torch.float32, device=dev)
        for k, m in enumerate(masks[s0:s0 + step]):
            mk[k].copy_(m.reshape(H, W))
        aux = ops.RenderAux()
        aux.antialiased = _antialiased(getattr(model.config, "rasterize_mode", "classic"))
        ops.trace_masks_views(model.means, model.scales, model.quats, model.opacities, model.features_dc, model.features_rest, gcams, mk,
                              w_in, w_all, aux)
    return w_in, w_all


@torch.no_grad()
def select(w_in, w_all, ratio_thresh: float = 0.5, min_weight: float = 0.0):
    """(select uint8 [N], count): select[n] = w_all[n] > min_weight and w_in[n] > ratio_thresh * w_all[n] (gc_trace_select); a Gaussian
    no view composites is never selected.  One 4-byte readback (count)."""
    if not (w_in.is_cuda and w_all.is_cuda):
        raise L.GaussCtrlHipError("edit_region.select needs GPU tensors (HIP path only; no CPU fallback)")
    N = w_in.numel()
    if w_all.numel() != N or w_in.dtype != torch.float32 or w_all.dtype != torch.float32 or not (w_in.is_contiguous() and w_all.is_contiguous()):
        raise ValueError("edit_region.select: w_in and w_all must be contiguous float32 tensors of one length")
    sel = torch.empty(N, dtype=torch.uint8, device=w_in.device)
    count = torch.empty(1, dtype=torch.int32, device=w_in.device)
    L.call("gc_trace_select", N, w_in, w_all, ratio_thresh, min_weight, sel, count)
    return sel, int(count.item())


def follow_cull(select, keep):
    """the selection of the rows a cull keeps: select [N], keep bool [N] -> contiguous [keep.sum()] of select's type"""
    if select.shape[0] != keep.shape[0]:
        raise ValueError(f"edit_region.follow_cull: select has {select.shape[0]} rows, keep {keep.shape[0]}")
    return select[keep.to(torch.bool)].contiguous()


def refuse_unsupported(config, model, world_size: int, have_masks: bool, have_nerfstudio: bool) -> None:
    """edit_region "traced" refuses, rather than half-works, where rows are not stepped by this package's FusedAdam on one GPU or where
    rows are added and moved"""
    if not have_masks:
        raise ValueError("edit_region 'traced' needs masks: set langsam_obj and pass a mask_fn")
    if have_nerfstudio:
        raise ValueError("edit_region 'traced' is not available under nerfstudio (its own optimizers step every row)")
    mcfg = getattr(model, "config", None)
    if getattr(mcfg, "refine_on_device", False):
        raise ValueError("edit_region 'traced' does not combine with refine_on_device (rows are added and moved)")
    if getattr(mcfg, "densify_strategy", "default") == "mcmc":
        raise ValueError("edit_region 'traced' does not combine with densify_strategy 'mcmc' (rows are added and moved)")
    if world_size > 1:
        raise ValueError("edit_region 'traced' runs on one GPU only (float atomics make near-threshold selections differ between ranks)")
    if getattr(config, "train_mode", "parity") == "sharded":
        raise ValueError("edit_region 'traced' does not combine with train_mode 'sharded' (ShardedAdam steps flat slices, not rows)")

"""Loss and optimiser of the 500-iteration splat optimisation on HIP kernels.

  l1_ssim_loss : SplatfactoModel.get_loss_dict's main loss, (1-l)*L1 + l*(1-SSIM) with l = 0.2 (inherited by the reference via
                 /root/reference/gaussctrl/gc_pipeline.py:284-285), forward value AND gradient w.r.t. the render in two launches;
  FusedAdam    : the Adam groups of /root/reference/gaussctrl/gc_config.py:58-87 (eps 1e-15) as one fused read-modify-write per
                 tensor (torch.optim.Adam semantics, interface-compatible: param_groups / step / zero_grad / state_dict).
"""
from __future__ import annotations

import torch

from . import _lib as L


class _L1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, lam, valid):
        if not pred.is_cuda:
            raise L.GaussCtrlHipError("l1_ssim_loss needs GPU tensors (HIP path only; no CPU fallback)")
        H, W, Cc = pred.shape
        p = pred.detach().float().contiguous(); t = target.detach().float().contiguous()
        nbytes = L.call("gc_l1_ssim_workspace_bytes", H, W, Cc)
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=p.device)
        sums = torch.empty(2, dtype=torch.float32, device=p.device)
        v = torch.empty_like(p)
        L.call("gc_l1_ssim_fwd_bwd", p, t, H, W, Cc, lam, 1.0, int(valid), sums, v, ws, nbytes)
        ctx.save_for_backward(v)
        n = float(H * W * Cc)
        n_ssim = float((H - 10) * (W - 10) * Cc) if valid else n
        return (1.0 - lam) * sums[1] / n + lam * (1.0 - sums[0] / n_ssim)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return v * g, None, None, None


def l1_ssim_loss(pred, target, ssim_lambda: float = 0.2, valid_window: bool = True):
    """pred, target: [H,W,3] float32 on the GPU -> scalar loss tensor (differentiable w.r.t. pred).
    valid_window=True: SSIM as pytorch_msssim.SSIM(data_range=1, channel=3) computes it (unpadded 11x11 gaussian windows, mean over
    the (H-10) x (W-10) interior) -- the module splatfacto's get_loss_dict calls [recall nerfstudio 1.0.0 splatfacto.py]."""
    return _L1SSIM.apply(pred, target, float(ssim_lambda), bool(valid_window))


class _L1SSIMViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, lam, valid):
        if not pred.is_cuda:
            raise L.GaussCtrlHipError("l1_ssim_loss_views needs GPU tensors (HIP path only; no CPU fallback)")
        B, H, W, Cc = pred.shape
        p = pred.detach().float().contiguous(); t = target.detach().float().contiguous()
        nbytes = L.call("gc_l1_ssim_views_workspace_bytes", B, H, W, Cc)
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=p.device)
        sums = torch.empty(B, 2, dtype=torch.float32, device=p.device)
        v = torch.empty_like(p)
        L.call("gc_l1_ssim_fwd_bwd_views", B, p, t, H, W, Cc, lam, 1.0, int(valid), sums, v, ws, nbytes)
        ctx.save_for_backward(v)
        n = float(H * W * Cc)
        n_ssim = float((H - 10) * (W - 10) * Cc) if valid else n
        return (1.0 - lam) * sums[:, 1] / n + lam * (1.0 - sums[:, 0] / n_ssim)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return v * g.reshape(-1, 1, 1, 1), None, None, None


def l1_ssim_loss_views(pred, target, ssim_lambda: float = 0.2, valid_window: bool = True):
    """pred, target: [B,H,W,3] float32 -> [B] losses (each view's own l1_ssim_loss), one pair of launches for the batch."""
    return _L1SSIMViews.apply(pred, target, float(ssim_lambda), bool(valid_window))


class _DepthL1Views(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        if not pred.is_cuda:
            raise L.GaussCtrlHipError("depth_l1_loss needs GPU tensors (HIP path only; no CPU fallback)")
        if pred.dim() != 3 or pred.shape != target.shape:
            raise ValueError("depth_l1_loss_views: pred and target must both be [B,H,W]")
        B, H, W = pred.shape
        p = pred.detach().float().contiguous(); t = target.detach().to(p.device).float().contiguous()
        nbytes = L.call("gc_depth_l1_views_workspace_bytes", B, H, W)
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=p.device)
        sums = torch.empty(B, 2, dtype=torch.float32, device=p.device)
        v = torch.empty_like(p)
        L.call("gc_depth_l1_fwd_bwd_views", B, p, t, H, W, 1.0, sums, v, ws, nbytes)
        ctx.save_for_backward(v)
        return sums[:, 0] / sums[:, 1].clamp(min=1.0)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return v * g.reshape(-1, 1, 1), None


def depth_l1_loss_views(pred, target):
    """pred, target: [B,H,W] float32 depth images -> [B] losses: each view's mean |pred - target| over the pixels where both depths are
    real (neither is the 1000 of an empty pixel, both finite); 0 for a view without such a pixel.  Differentiable w.r.t. pred."""
    return _DepthL1Views.apply(pred, target)


def depth_l1_loss(pred, target):
    """depth_l1_loss_views for one [H,W] pair -> scalar loss tensor."""
    return _DepthL1Views.apply(pred[None], target[None])[0]


class FusedAdam(torch.optim.Optimizer):
    """row_select: None (every element steps: gc_adam_step), or a uint8 [rows] GPU tensor -- then a parameter whose first dimension has
    that many rows steps only in the rows with a non-zero byte (gc_adam_step_rows, include/gaussctrl_trace.h: every other row of the
    parameter and of both moments keeps its bits); parameters of another row count step whole."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-15):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self.row_select = None

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise L.GaussCtrlHipError("FusedAdam needs contiguous float32 GPU parameters")
                state = self.state[p]
                if not state:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                state["step"] += 1
                g = p.grad.contiguous()
                sel = getattr(self, "row_select", None)
                if sel is not None and p.dim() >= 1 and p.shape[0] == sel.numel():
                    if not sel.is_cuda or sel.dtype != torch.uint8 or not sel.is_contiguous():
                        raise L.GaussCtrlHipError("FusedAdam.row_select must be a contiguous uint8 GPU tensor")
                    rows = p.shape[0]
                    L.call("gc_adam_step_rows", p, g, state["exp_avg"], state["exp_avg_sq"], rows, p.numel() // rows if rows else 1, sel,
                           group["lr"], b1, b2, group["eps"], state["step"])
                    continue
                L.call("gc_adam_step", p, g, state["exp_avg"], state["exp_avg_sq"], p.numel(), group["lr"], b1, b2, group["eps"], state["step"])

"""Per-view camera pose refinement for training on edited views: what later splatfacto / gsplat 1.x call camera_optimizer, mode "SO3xR3".
The reference of this project (nerfstudio 1.0 splatfacto, gsplat 0.1.3) trains with constant poses; the conventions below are recalled from
later nerfstudio and were not checked against its source -- this docstring and include/gaussctrl_pose.h are the contract.

Every training view owns six numbers, a row of GaussCtrlModel.pose_adjustment: (tau, omega) = (row[:3], row[3:]).  The adjusted pose is

    c2w' = c2w @ [exp(omega) | tau]        (right-multiplication: the adjustment lives in the camera's own frame)

with exp the SO(3) exponential: R' = R exp(omega), t' = R tau + t.  It is composed on the host in float64, rounded to float32 and handed to
camera.camera_to_gsplat untouched, so an all-zero row gives the `cam` dict of the unadjusted camera bit for bit.  A sub-pixel shift or
rotation of one edited view's content against its camera lands in that view's row instead of in blur and floaters.

The gradient: the renderer leaves d loss / d viewmat[:3] of the view (RenderAux.pose_grad -> RenderAux.viewmat_grad, the kernels of
include/gaussctrl_pose.h), and `link` ties the row into the autograd graph: its backward chains that [3, 4] gradient through the float64
Jacobian of row -> viewmat (a few dozen flops and one 48-byte read-back per step: host code, not the hot path).  The SH view directions move
with the camera in the forward but pass no gradient to the pose, as they pass none to the means.

Opt-in: GaussCtrlModelConfig.camera_optimizer_mode = "SO3xR3" (stand-alone model, one GPU, gradients through autograd)."""
from __future__ import annotations

import numpy as np
import torch

MODES = ("off", "SO3xR3")
SMALL_ANGLE2 = 1e-4          # |omega|^2 below this: the series (their first neglected terms are below 1e-16 there)


def check_mode(mode) -> bool:
    """camera_optimizer_mode -> is it on; anything but the two names is a ValueError"""
    if mode not in MODES:
        raise ValueError(f"camera_optimizer_mode must be one of {MODES}, got {mode!r}")
    return mode != "off"


def check_config(config) -> bool:
    """camera_optimizer_mode with its three numbers checked; a wrong type or range is a ValueError"""
    on = check_mode(getattr(config, "camera_optimizer_mode", "off"))
    lr = getattr(config, "camera_opt_lr", None)
    if lr is not None and (isinstance(lr, bool) or not isinstance(lr, (int, float)) or not lr > 0 or lr == float("inf")):
        raise ValueError(f"camera_opt_lr must be None (the optimizer table's schedule) or a finite positive number, got {lr!r}")
    for name in ("camera_opt_trans_l2_penalty", "camera_opt_rot_l2_penalty"):
        v = getattr(config, name, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0 or v == float("inf"):
            raise ValueError(f"{name} must be a finite non-negative number, got {v!r}")
    return on


def refuse_unsupported(model_config, world_size: int = 1, train_mode: str = "single", have_nerfstudio: bool = False,
                       crop_in_training: bool = False) -> None:
    """camera_optimizer_mode "SO3xR3" refuses, rather than half-works, every combination in which the pose gradient would not reach its
    optimizer or the adjustment would not be applied"""
    if not check_mode(getattr(model_config, "camera_optimizer_mode", "off")):
        return
    if have_nerfstudio:
        raise ValueError("camera_optimizer_mode 'SO3xR3' is built for the stand-alone model only (under nerfstudio the inherited splatfacto "
                         "behaviour stays: leave the field 'off')")
    if world_size > 1:
        raise ValueError("camera_optimizer_mode 'SO3xR3' trains on one GPU only (world_size > 1: the pose gradient is not in the flat "
                         "gradient buffers of any train_mode)")
    if train_mode in ("throughput", "sharded"):
        raise ValueError(f"camera_optimizer_mode 'SO3xR3' needs the gradients to pass through autograd (train_mode {train_mode!r} writes them "
                         "into grad_into buffers)")
    if crop_in_training:
        raise ValueError("camera_optimizer_mode 'SO3xR3' does not train with a crop box")


def check_view(camera, V: int) -> int:
    """camera.metadata["cam_idx"] -> the row of pose_adjustment it names; a missing index or one outside [0, V) is a ValueError"""
    md = getattr(camera, "metadata", None)
    if not isinstance(md, dict) or md.get("cam_idx") is None:
        raise ValueError("camera_optimizer_mode 'SO3xR3': the training camera carries no metadata['cam_idx'] (the datamanager sets it)")
    idx = int(md["cam_idx"])
    if not 0 <= idx < V:
        raise ValueError(f"camera_optimizer_mode 'SO3xR3': cam_idx {idx} is outside [0, {V}): the model was built for {V} training views")
    return idx


def so3_exp(omega: torch.Tensor) -> torch.Tensor:
    """[3] float64 -> the rotation exp([omega]x) by Rodrigues' formula, I + A K + B K^2 with A = sin(a) / a, B = (1 - cos(a)) / a^2; below
    |omega|^2 = SMALL_ANGLE2 the two coefficients are their series in a^2 (no division by the angle, differentiable at 0).  omega = 0 gives
    the identity exactly."""
    omega = omega.to(torch.float64)
    t2 = (omega * omega).sum()
    if float(t2.detach()) < SMALL_ANGLE2:
        A = 1.0 - t2 / 6.0 + t2 * t2 / 120.0 - t2 * t2 * t2 / 5040.0
        B = 0.5 - t2 / 24.0 + t2 * t2 / 720.0 - t2 * t2 * t2 / 40320.0
    else:
        a = torch.sqrt(t2)
        A = torch.sin(a) / a
        B = (1.0 - torch.cos(a)) / t2
    z = torch.zeros((), dtype=torch.float64)
    K = torch.stack([torch.stack([z, -omega[2], omega[1]]), torch.stack([omega[2], z, -omega[0]]), torch.stack([-omega[1], omega[0], z])])
    return torch.eye(3, dtype=torch.float64) + A * K + B * (K @ K)


def compose(c2w, row: torch.Tensor) -> torch.Tensor:
    """c2w [3, 4] (or [4, 4]), row [6] = (tau, omega) -> c2w' = c2w @ [exp(omega) | tau], [3, 4] float64 (differentiable in row)"""
    c = torch.as_tensor(np.asarray(c2w, dtype=np.float64)[:3, :4])
    row = row.to(torch.float64)
    R, t = c[:, :3], c[:, 3]
    return torch.cat([R @ so3_exp(row[3:]), (R @ row[:3] + t)[:, None]], 1)


def viewmat_of(c2w: torch.Tensor) -> torch.Tensor:
    """[3, 4] float64 OpenGL camera-to-world -> the [3, 4] world-to-camera matrix camera_to_gsplat builds (y and z flipped, inverted)"""
    Rg = c2w[:, :3] * torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64)
    return torch.cat([Rg.T, -(Rg.T @ c2w[:, 3])[:, None]], 1)


def adjusted_c2w(c2w, row) -> np.ndarray:
    """the pose camera_to_gsplat is handed: compose in float64, rounded to float32 ([3, 4]).  An all-zero row returns c2w's own float32
    values untouched (the product R @ I would already do so up to the sign of a zero entry: -0 * 1 + 0 + 0 = +0)"""
    row = torch.as_tensor(row).detach().cpu()
    if not bool(row.any()):
        return np.asarray(c2w, dtype=np.float32)[:3, :4].copy()
    with torch.no_grad():
        return compose(c2w, row).numpy().astype(np.float32)


def jacobian(c2w, row) -> torch.Tensor:
    """d viewmat[:3] / d row of the composed pose, [3, 4, 6] float64: autograd through compose's own float64 operations (Rodrigues'
    formula or, at small angles, its series -- never a division by the angle)"""
    r = torch.as_tensor(row).detach().cpu().to(torch.float64)
    return torch.autograd.functional.jacobian(lambda x: viewmat_of(compose(c2w, x)), r)


class _Link(torch.autograd.Function):
    """means pass through unchanged; the backward runs after the render's (which produced the means' gradient) and so finds the view's
    RenderAux.viewmat_grad, which it chains to the row"""

    @staticmethod
    def forward(ctx, means, row, aux, c2w):
        ctx.aux, ctx.c2w = aux, c2w
        ctx.save_for_backward(row)
        return means.view_as(means)

    @staticmethod
    def backward(ctx, v_means):
        (row,) = ctx.saved_tensors
        g = ctx.aux.viewmat_grad
        if g is None:            # nothing was rendered (no Gaussian visible): no pose gradient either
            return v_means, torch.zeros_like(row), None, None
        J = jacobian(ctx.c2w, row)
        v = torch.einsum("rc,rcj->j", g.detach().reshape(-1, 3, 4)[0].to("cpu", torch.float64), J)
        return v_means, v.to(row.dtype).to(row.device), None, None


def link(means, row, aux, c2w):
    """ties pose row `row` ([6], requires grad) into the graph of a render of `means` under compose(c2w, row) with aux.pose_grad set:
    returns means (same values), whose use in ops.render_view makes backward() deliver d loss / d row"""
    return _Link.apply(means, row, aux, np.asarray(c2w, dtype=np.float64)[:3, :4].copy())


def regularizer(pose_adjustment, trans_l2_penalty: float, rot_l2_penalty: float):
    """trans_l2_penalty * mean |tau| + rot_l2_penalty * mean |omega| over the views (0 with zero gradient at an all-zero row)"""
    return trans_l2_penalty * row_norms(pose_adjustment[:, :3]).mean() + rot_l2_penalty * row_norms(pose_adjustment[:, 3:]).mean()


def row_norms(x):
    """|row|_2 with the subgradient 0 at a zero row (sqrt alone has none there)"""
    s = (x * x).sum(-1)
    live = s > 0
    return torch.where(live, torch.sqrt(torch.where(live, s, torch.ones_like(s))), torch.zeros_like(s))

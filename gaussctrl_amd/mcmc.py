"""MCMC densification of the stand-alone splat model on HIP kernels (csrc/train_mcmc.hip, include/gaussctrl_mcmc.h): the strategy of
"3D Gaussian Splatting as Markov Chain Monte Carlo" as gsplat 1.x's MCMCStrategy runs it.  The reference of this project (gsplat 0.1.3,
nerfstudio 1.0) has none of it; the formulas are recalled from the paper and gsplat 1.x and were not checked against their source -- the
header states them and is the contract.

  schedule(config, step)                 : is `step` a refinement step (pure Python);
  relocate(model, optimizers, sampled)   : dead Gaussians (sigmoid(opacity) <= mcmc_min_opacity) become copies of live ones drawn with
                                           probability proportional to their opacity; no tensor changes size or storage;
  add_new(model, optimizers, sampled)    : grow by 5 % towards mcmc_cap_max with copies drawn the same way (new tensors, optimizer state
                                           re-keyed by scene_rows.swap_rows);
  inject_noise(model, lr, noise)         : after every optimizer step, means += Cov noise * g(opacity) * lr * mcmc_noise_lr in ONE launch.

A relocation is  gc_mcmc_dead -> an 8-byte read-back of {n_dead, n_alive} (its only synchronisation) -> torch.multinomial on the device ->
gc_mcmc_relocate.  Under nerfstudio SplatfactoModel's own callbacks stay in charge; this module serves the stand-alone model
(GaussCtrlModelConfig.densify_strategy = "mcmc", gc_trainer.McmcCallback)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib as L
from .scene_rows import check_params, leaf_states, moment_ptrs, new_rows, ptr_array, rest_floats, swap_rows

MAX_CATEGORIES = 1 << 24          # torch.multinomial takes fewer categories than this


def schedule(config, step: int) -> bool:
    c = config
    return c.mcmc_refine_start_iter < step < c.mcmc_refine_stop_iter and step % c.mcmc_refine_every == 0


def _check_model(model, what: str) -> int:
    if not model.means.is_cuda:
        raise L.GaussCtrlHipError(f"mcmc.{what} needs GPU parameters (HIP path only; no CPU fallback)")
    check_params(model, f"mcmc.{what}")
    return int(model.means.shape[0])


def dead_rows(opacities: torch.Tensor, min_opacity: float):
    """gc_mcmc_dead on opacity logits [N, 1] -> (weights [N] float32, dead_idx [N] int32 of which the first n_dead are written, n_dead,
    n_alive); the two counts are read back (8 bytes: the one synchronisation)."""
    N = int(opacities.shape[0])
    dev = opacities.device
    weights = torch.empty(N, dtype=torch.float32, device=dev)
    dead_idx = torch.empty(N, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    nbytes = L.call("gc_mcmc_dead_workspace_bytes", N)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device=dev)
    L.call("gc_mcmc_dead", N, opacities, min_opacity, weights, dead_idx, counts, ws, nbytes)
    n_dead, n_alive = (int(v) for v in counts.cpu()) if N > 0 else (0, 0)
    return weights, dead_idx, n_dead, n_alive


def _draw(weights: torch.Tensor, n: int, sampled: Optional[torch.Tensor], what: str) -> torch.Tensor:
    """n source rows, int32 on the device: torch.multinomial over the weights, or the caller's draws after validation"""
    N = weights.shape[0]
    if sampled is None:
        return torch.multinomial(weights, n, replacement=True).to(torch.int32)
    if not torch.is_tensor(sampled) or not sampled.is_cuda:
        raise L.GaussCtrlHipError(f"mcmc.{what}: sampled must be a GPU tensor (HIP path only; no CPU fallback)")
    if sampled.dtype not in (torch.int32, torch.int64) or tuple(sampled.shape) != (n,):
        raise ValueError(f"mcmc.{what}: sampled must be int32 / int64 of shape [{n}], got {sampled.dtype} {tuple(sampled.shape)}")
    idx = sampled.to(weights.device, torch.int64)
    if bool(((idx < 0) | (idx >= N)).any()):                       # (one synchronisation at a refinement step)
        raise ValueError(f"mcmc.{what}: sampled holds rows outside [0, {N})")
    if bool((weights[idx] == 0).any()):
        raise ValueError(f"mcmc.{what}: sampled holds dead rows (sampling weight 0)")
    return idx.to(torch.int32).contiguous()


def _relocate_call(N, n, rest, sampled, dest, min_opacity, params, moments):
    mult = torch.empty(N, dtype=torch.int32, device=sampled.device)
    L.call("gc_mcmc_relocate", N, n, rest, sampled, dest, min_opacity, mult, ptr_array(params), moment_ptrs(moments, "exp_avg"),
           moment_ptrs(moments, "exp_avg_sq"))
    return mult


@torch.no_grad()
def relocate(model, optimizers, sampled: Optional[torch.Tensor] = None) -> int:
    """Every dead row (sigmoid(opacity) <= mcmc_min_opacity) becomes a copy of a live row drawn with probability proportional to its
    opacity; the drawn rows' opacity and scales are reduced so that the sum of the copies renders like the original (header), their Adam
    moments and the copies' are zero.  In place: N, every parameter's and moment's storage stay.  sampled: [n_dead] live rows instead of
    the draw (tests).  Returns the number of relocated rows."""
    N = _check_model(model, "relocate")
    if N == 0:
        return 0
    if N >= MAX_CATEGORIES:
        raise L.GaussCtrlHipError(f"mcmc.relocate: torch.multinomial takes fewer than 2^24 categories, the scene has {N} Gaussians")
    c = model.config
    weights, dead_idx, n_dead, n_alive = dead_rows(model.opacities.data, float(c.mcmc_min_opacity))
    if n_dead == 0 or n_alive == 0:
        return 0
    src = _draw(weights, n_dead, sampled, "relocate")
    states = leaf_states(model, optimizers, "mcmc.relocate", params_checked=True)
    _relocate_call(N, n_dead, rest_floats(model), src, dead_idx[:n_dead], float(c.mcmc_min_opacity), [p.data for _, p, _ in states],
                   [st for _, _, st in states])
    for _, p, _ in states:
        p.grad = None
    return n_dead


@torch.no_grad()
def add_new(model, optimizers, sampled: Optional[torch.Tensor] = None) -> int:
    """Grow the scene to min(mcmc_cap_max, int(1.05 N)) rows: the new rows are copies of rows drawn with probability proportional to their
    opacity, updated as in relocate().  New tensors for the six parameters and their Adam moments (state["step"] kept; the new rows'
    moments zero).  As after RefineState.refine, a loss graph of the previous step that the caller still holds keeps the old row count's gradient
    accumulators alive: drop it before the next forward (the trainers do).  sampled: [n_new] rows instead of the draw (tests).  Returns the
    number of rows added."""
    N = _check_model(model, "add_new")
    c = model.config
    n_new = min(int(c.mcmc_cap_max), int(1.05 * N)) - N
    if N == 0 or n_new <= 0:
        return 0
    if N >= MAX_CATEGORIES:
        raise L.GaussCtrlHipError(f"mcmc.add_new: torch.multinomial takes fewer than 2^24 categories, the scene has {N} Gaussians")
    weights, _, _, n_alive = dead_rows(model.opacities.data, 0.0)          # min_opacity 0: the weights are sigmoid(opacities) of all rows
    if n_alive == 0:
        return 0
    src = _draw(weights, n_new, sampled, "add_new")
    states = leaf_states(model, optimizers, "mcmc.add_new", params_checked=True)
    params, moments = new_rows(states, N + n_new, keep_old=True)
    _relocate_call(N, n_new, rest_floats(model), src, None, float(c.mcmc_min_opacity), params, moments)
    swap_rows(model, states, params, moments)
    return n_new


@torch.no_grad()
def inject_noise(model, lr: float, noise: Optional[torch.Tensor] = None) -> None:
    """means += Rot diag(exp(2 scales)) Rot^T noise * g(sigmoid(opacities)) * lr * mcmc_noise_lr, one launch.  noise: [N, 3] float32
    standard-normal draws (default: torch.randn on the model's device)."""
    N = _check_model(model, "inject_noise")
    dev = model.means.device
    if noise is None:
        noise = torch.randn(N, 3, device=dev)
    else:
        if not torch.is_tensor(noise) or not noise.is_cuda:
            raise L.GaussCtrlHipError("mcmc.inject_noise: noise must be a GPU tensor (HIP path only; no CPU fallback)")
        if noise.dtype != torch.float32 or tuple(noise.shape) != (N, 3):
            raise ValueError(f"mcmc.inject_noise: noise must be float32 of shape [{N}, 3], got {noise.dtype} {tuple(noise.shape)}")
        noise = noise.to(dev).contiguous()
    L.call("gc_mcmc_inject_noise", N, model.means.data, model.scales.data, model.quats.data, model.opacities.data, noise,
           float(lr) * float(model.config.mcmc_noise_lr))

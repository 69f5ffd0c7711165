"""Refinement (densification) of the stand-alone splat model on HIP kernels: splatfacto's after_train / refinement_after [recall
nerfstudio 1.0.0 splatfacto.py] -- screen-space gradient statistics, split / duplicate, cull, opacity reset (csrc/train_refine.hip).

  schedule(config, step, num_train_data) : which of densify / cull-only / opacity reset a trainer step runs (pure Python);
  RefineState                            : the three per-Gaussian statistics (lazily sized), accumulate() after every training step,
                                           refine() at a refinement step;
  accumulate(model) / refine(model, ...) : the same on the state kept at model._refine_state.

One refinement is  gc_refine_plan -> a 20-byte read-back of the counts (its only synchronisation) -> gc_refine_apply into NEW tensors for
the six parameters and their Adam moments [-> gc_refine_reset_opacity].  Under nerfstudio SplatfactoModel's own callbacks stay in charge;
this module serves the stand-alone model (GaussCtrlModelConfig.refine_on_device)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as L
from .scene_rows import NAMES, WIDTHS, leaf_states, moment_ptrs, new_rows, ptr_array, rest_floats, swap_rows      # noqa: F401  (NAMES, WIDTHS: importable from here)

# bits of the per-Gaussian action word (include/gaussctrl_refine.h GC_REFINE_*)
KEEP, SPLIT, DUP, EMIT_SPLIT, EMIT_DUP, BELOW_ALPHA, TOO_BIG, ON_SCREEN = 1, 2, 4, 8, 16, 32, 64, 128


@dataclass(frozen=True)
class Schedule:
    refine: bool          # a refinement step at all (step % refine_every == 0 and step > warmup_length)
    densify: bool         # split / duplicate, then cull
    cull_only: bool       # the cull after stop_split_at (what gc_trainer.CullCallback does)
    reset: bool           # the opacity reset, after the above
    cull_by_scale: bool   # step > refine_every * reset_alpha_every
    by_screen: bool       # step < stop_screen_size_at: the screen-size split test, and (with cull_by_scale) the screen-size cull of a densify step


def schedule(config, step: int, num_train_data: int) -> Schedule:
    c = config
    R, I = c.refine_every, c.refine_every * c.reset_alpha_every
    is_refine = step % R == 0 and step > c.warmup_length
    before_stop = step < c.stop_split_at
    densify = is_refine and before_stop and step % I > num_train_data + R
    cull_only = is_refine and not before_stop and bool(c.continue_cull_post_densification)
    reset = is_refine and before_stop and step % I == R
    return Schedule(is_refine, densify, cull_only, reset, step > I, step < c.stop_screen_size_at)


def reset_logit(cull_alpha_thresh: float) -> float:
    """logit(2 * cull_alpha_thresh) in float32: the value splatfacto clamps the opacities to."""
    return float(torch.logit(torch.tensor(2.0 * cull_alpha_thresh, dtype=torch.float32)))


class RefineState:
    """grad_norm_sum / vis_count / max_2dsize, float32 [N], created at the first accumulate() and dropped by every refinement step."""

    def __init__(self):
        self.grad_norm_sum = self.vis_count = self.max_2dsize = None
        self.last = None          # {"n_in", "n_out", "n_survivors", "n_split_src", "n_dup_src", "n_below_alpha"} of the last refine()

    def clear(self):
        self.grad_norm_sum = self.vis_count = self.max_2dsize = None

    def _ensure(self, N, device):
        if self.grad_norm_sum is None or self.grad_norm_sum.shape[0] != N:
            self.grad_norm_sum, self.vis_count, self.max_2dsize = (torch.zeros(N, dtype=torch.float32, device=device) for _ in range(3))

    @torch.no_grad()
    def accumulate_views(self, xys_grad, radii, height: int, width: int):
        """xys_grad [N,2] or [C,N,2], radii [N] or [C,N] int32 of one backward (one or C views of the scene)."""
        if not xys_grad.is_cuda:
            raise L.GaussCtrlHipError("refine.accumulate needs GPU tensors (HIP path only; no CPU fallback)")
        g = xys_grad.detach().float().contiguous()
        r = radii.detach().to(torch.int32).contiguous()
        N = g.shape[-2]
        Cv = 1 if g.dim() == 2 else g.shape[0]
        if r.numel() != Cv * N:
            raise ValueError("refine.accumulate: radii and xys_grad disagree")
        self._ensure(N, g.device)
        L.call("gc_refine_accumulate_views", N, Cv, g, r, 1.0 / max(height, width), self.grad_norm_sum, self.vis_count, self.max_2dsize)

    def accumulate(self, model):
        """after a training backward: model._aux.xys_grad -- with config.use_absgrad model._aux.xys_absgrad, the per-pixel absolute sums --
        model.radii, model.last_size (nothing to do when nothing was rendered)"""
        g = model._aux.xys_grad
        if g is None or model.radii is None or model.last_size is None:
            return
        if getattr(model.config, "use_absgrad", False):
            g = model._aux.xys_absgrad
            if g is None:
                raise L.GaussCtrlHipError("refine.accumulate: config.use_absgrad is set but the backward left no xys_absgrad "
                                          "(the render did not run with RenderAux.absgrad)")
        self.accumulate_views(g, model.radii, int(model.last_size[0]), int(model.last_size[1]))

    # ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def plan(self, model, sch: Schedule, max_dim: float):
        """gc_refine_plan for this step -> (action [N] int32, ranks [3,N] int32, counts: 5 host ints)"""
        c = model.config
        N = model.means.shape[0]
        dev = model.means.device
        action = torch.empty(N, dtype=torch.int32, device=dev)
        ranks = torch.empty(3, N, dtype=torch.int32, device=dev)
        counts = torch.zeros(5, dtype=torch.int32, device=dev)
        nbytes = L.call("gc_refine_plan_workspace_bytes", N)
        ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device=dev)
        densify = bool(sch.densify)
        cull_by_screen = densify and sch.cull_by_scale and sch.by_screen
        if densify or cull_by_screen:
            self._ensure(N, dev)          # (no view seen since the last refinement: zero statistics, nothing is high)
        stats = (self.grad_norm_sum, self.vis_count, self.max_2dsize) if densify else (None, None, None)
        L.call("gc_refine_plan", N, model.scales.data, model.opacities.data, stats[0], stats[1], stats[2], densify, c.n_split_samples, max_dim,
               c.densify_grad_thresh, c.densify_size_thresh, densify and sch.by_screen, c.split_screen_size, c.cull_alpha_thresh,
               sch.cull_by_scale, c.cull_scale_thresh, cull_by_screen, c.cull_screen_size, action, ranks, counts, ws, nbytes)
        host = [int(v) for v in counts.cpu()] if N > 0 else [0, 0, 0, 0, 0]       # the one synchronisation of a refinement
        return action, ranks, host

    @torch.no_grad()
    def refine(self, model, optimizers, step: int, num_train_data: int, samples: Optional[torch.Tensor] = None) -> Schedule:
        """What splatfacto's refinement_after does at `step`.  Swaps new tensors into the model's nn.Parameters, re-keys each optimizer's
        state (state["step"] kept; survivors' moments copied, children's zero), sets model._cull_keep to the row mask of a pure cull and to None when
        rows were added (scene_rows.swap_rows), and drops the statistics.  samples: [n_split_samples * n_split_src, 3] standard-normal draws for the split children (default:
        torch.randn on the model's device).  Returns the step's Schedule; self.last holds the counts."""
        sch = schedule(model.config, step, num_train_data)
        if not sch.refine:
            return sch
        if not model.means.is_cuda:
            raise L.GaussCtrlHipError("refine needs GPU parameters (HIP path only; no CPU fallback)")
        self.last = None
        if sch.densify or sch.cull_only:
            self._rebuild(model, optimizers, sch, samples)
        if sch.reset:
            st = leaf_states(model, optimizers, "refine")[NAMES.index("opacities")][2]
            m, v = (st["exp_avg"], st["exp_avg_sq"]) if st else (None, None)
            L.call("gc_refine_reset_opacity", model.opacities.numel(), reset_logit(model.config.cull_alpha_thresh), model.opacities.data, m, v)
        self.clear()
        return sch

    def _rebuild(self, model, optimizers, sch, samples):
        c = model.config
        N = model.means.shape[0]
        dev = model.means.device
        max_dim = float(max(model.last_size)) if model.last_size is not None else 1.0
        states = leaf_states(model, optimizers, "refine")
        action, ranks, (n_surv, n_split_src, n_dup_src, n_out, n_below) = self.plan(model, sch, max_dim)
        self.last = dict(n_in=N, n_out=n_out, n_survivors=n_surv, n_split_src=n_split_src, n_dup_src=n_dup_src, n_below_alpha=n_below)
        if N == 0 or (n_surv == N and n_split_src == 0 and n_dup_src == 0):
            return                                              # nothing to do: the tensors stay as they are
        ns = int(c.n_split_samples)
        if n_split_src > 0:
            if samples is None:
                samples = torch.randn(ns * n_split_src, 3, device=dev)
            if tuple(samples.shape) != (ns * n_split_src, 3):
                raise ValueError(f"refine: samples must be [{ns * n_split_src}, 3] (n_split_samples x n_split_src), got {tuple(samples.shape)}")
            samples = samples.to(dev, torch.float32).contiguous()
        else:
            samples = None
        moments = [st for _, _, st in states]
        p_out, m_out = new_rows(states, n_out)
        L.call("gc_refine_apply", N, ns, rest_floats(model), n_surv, n_split_src, n_dup_src, action, ranks, samples,
               ptr_array([p.data for _, p, _ in states]), moment_ptrs(moments, "exp_avg"), moment_ptrs(moments, "exp_avg_sq"),
               ptr_array(p_out), moment_ptrs(m_out, "exp_avg"), moment_ptrs(m_out, "exp_avg_sq"))
        # pure cull: train_mode "sharded" prunes its optimizer-state slices with the same mask
        keep = (action & KEEP) != 0 if n_split_src == 0 and n_dup_src == 0 else None
        swap_rows(model, states, p_out, m_out, keep)


def _state(model) -> RefineState:
    st = getattr(model, "_refine_state", None)
    if st is None:
        st = model._refine_state = RefineState()
    return st


def accumulate(model) -> None:
    """RefineState.accumulate on the state kept with the model."""
    _state(model).accumulate(model)


def refine(model, optimizers, step: int, num_train_data: int, samples: Optional[torch.Tensor] = None) -> Schedule:
    """RefineState.refine on the state kept with the model."""
    return _state(model).refine(model, optimizers, step, num_train_data, samples)

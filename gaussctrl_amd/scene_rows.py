"""The six leaf tensors of a splat scene and their Adam state, for every step that changes the scene's rows (gc_trainer.CullCallback,
refine.py, mcmc.py): who owns which parameter, what the kernels may be handed, and the ONE place (swap_rows) where new tensors replace
the old ones under the same nn.Parameter."""
import ctypes as C

import torch

from . import _lib as L

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")      # the order of the C ABI
WIDTHS = (3, 3, 4, 1, 3)
MOMENTS = ("exp_avg", "exp_avg_sq")


def ptr_array(tensors):
    return (C.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in tensors])


def rest_floats(model) -> int:
    """floats of features_rest per Gaussian (0 for an empty scene)"""
    return int(model.features_rest[0].numel()) if model.features_rest.shape[0] > 0 else 0


def owners(model, optimizers) -> dict:
    """parameter name -> (optimizer | None, nn.Parameter) through the model's param groups"""
    out = {}
    by_id = {id(getattr(model, n)): n for n in NAMES}
    for gname, params in model.get_param_groups().items():
        for p in params:
            if id(p) in by_id:
                out[by_id[id(p)]] = ((optimizers or {}).get(gname), p)
    return out


def check_params(model, what: str) -> None:
    for n in NAMES:
        t = getattr(model, n).data
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise L.GaussCtrlHipError(f"{what} needs contiguous float32 parameters")


def leaf_states(model, optimizers, what: str, params_checked: bool = False) -> list:
    """per tensor of NAMES: (optimizer | None, parameter, state dict with both moments | None), fit for the kernels: float32 contiguous
    parameters (unless the caller has just made check_params), moments likewise and shaped like their parameter.  what: the error prefix."""
    if not params_checked:
        check_params(model, what)
    own = owners(model, optimizers)
    out = []
    for n in NAMES:
        opt, p = own.get(n, (None, getattr(model, n)))
        st = opt.state.get(p) if opt is not None else None
        st = st if st and "exp_avg" in st and "exp_avg_sq" in st else None
        if st is not None:
            for t in (st["exp_avg"], st["exp_avg_sq"]):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape:
                    raise L.GaussCtrlHipError(f"{what} needs contiguous float32 Adam moments shaped like their parameter")
        out.append((opt, p, st))
    return out


def moment_ptrs(moments, key: str):
    """one moment of the six tensors as the C ABI's pointer array; moments: per tensor a dict with both moments, or None"""
    return ptr_array([m[key] if m else None for m in moments])


def new_rows(states, n: int, keep_old: bool = False):
    """new n-row tensors for leaf_states' result: (parameters, per tensor {exp_avg, exp_avg_sq} or None, as swap_rows takes them);
    keep_old: the old rows are copied into the first rows"""
    def new(t):
        out = torch.empty((n,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
        if keep_old:
            out[:t.shape[0]].copy_(t)
        return out
    return [new(p.data) for _, p, _ in states], [{k: new(st[k]) for k in MOMENTS} if st else None for _, _, st in states]


def swap_rows(model, states, new_params, new_moments, keep=None) -> None:
    """The scene's rows changed: new_params[k] becomes the data of states[k]'s parameter, its gradient goes, and the optimizer state is
    re-keyed under the same nn.Parameter with the entries of new_moments[k] ({key: tensor} or None) replaced and every other key ("step")
    kept.  keep: the row mask of a pure cull, with which train_mode "sharded" prunes its optimizer-state slices
    (GaussCtrlPipeline._sharded_adam); None when rows were added or moved, so that no older mask outlives this step."""
    for (opt, p, _), data, moments in zip(states, new_params, new_moments):
        full = opt.state.pop(p, None) if opt is not None else None
        p.data = data
        p.grad = None
        if full:
            full.update(moments or {})
            opt.state[p] = full
    model._cull_keep = keep

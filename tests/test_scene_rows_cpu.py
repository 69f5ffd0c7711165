"""CPU: gaussctrl_amd/scene_rows.py, the one owner of "the scene's rows changed" -- swap_rows under the same nn.Parameter, leaf_states' validation,
and gc_trainer.CullCallback on top of them.  A six-tensor stub model with N = 5 and torch.optim.Adam per group after one real step; no library
is loaded."""
import types

import pytest
import torch

from gaussctrl_amd import scene_rows as SR
from gaussctrl_amd._lib import GaussCtrlHipError
from gaussctrl_amd.gc_trainer import CullCallback

N = 5
_SHAPES = {"means": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N, 1), "features_dc": (N, 3), "features_rest": (N, 15, 3)}
_GROUPS = {"xyz": "means", "features_dc": "features_dc", "features_rest": "features_rest", "opacity": "opacities", "scaling": "scales",
           "rotation": "quats"}
_CONFIG = dict(continue_cull_post_densification=True, stop_split_at=10, refine_every=5, reset_alpha_every=30, cull_alpha_thresh=0.1,
               cull_scale_thresh=0.5)


class Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        for k, s in _SHAPES.items():
            setattr(self, k, torch.nn.Parameter(torch.randn(*s, generator=g)))
        self.config = types.SimpleNamespace(**_CONFIG)

    def get_param_groups(self):
        return {g: [getattr(self, n)] for g, n in _GROUPS.items()}


def _stepped(without=(), unstepped=()):
    """the model and one Adam per group after one real step (groups in `without` have no optimizer, those in `unstepped` no state yet)"""
    model = Model()
    opts = {g: torch.optim.Adam(ps, lr=1e-3) for g, ps in model.get_param_groups().items() if g not in without}
    g = torch.Generator().manual_seed(1)
    for gname, opt in opts.items():
        if gname in unstepped:
            continue
        for p in opt.param_groups[0]["params"]:
            p.grad = torch.randn(*p.shape, generator=g)
        opt.step()
    return model, opts


def _rows(states, n, seed):
    g = torch.Generator().manual_seed(seed)
    new = lambda p: torch.randn(n, *p.shape[1:], generator=g)
    return [new(p) for _, p, _ in states], [{k: new(p) for k in SR.MOMENTS} if st else None for _, p, st in states]


def test_names_stay_importable_from_refine():
    from gaussctrl_amd import refine
    assert refine.NAMES is SR.NAMES and refine.WIDTHS is SR.WIDTHS == (3, 3, 4, 1, 3)
    assert (refine.KEEP, refine.SPLIT, refine.DUP, refine.EMIT_SPLIT, refine.EMIT_DUP) == (1, 2, 4, 8, 16)
    assert (refine.BELOW_ALPHA, refine.TOO_BIG, refine.ON_SCREEN) == (32, 64, 128)


def test_swap_rows_cull():
    model, opts = _stepped()
    states = SR.leaf_states(model, opts, "test")
    assert [p is getattr(model, n) for (_, p, _), n in zip(states, SR.NAMES)] == [True] * 6
    group_of = {n: g for g, n in _GROUPS.items()}
    assert [opt for opt, _, _ in states] == [opts[group_of[n]] for n in SR.NAMES]
    steps = [st["step"].clone() for _, _, st in states]
    for _, p, _ in states:
        p.grad = torch.ones_like(p)
    keep = torch.tensor([True, False, True, True, False])
    params, moments = _rows(states, 3, seed=2)
    SR.swap_rows(model, states, params, moments, keep)
    for k, (opt, p, _) in enumerate(states):
        assert p is getattr(model, SR.NAMES[k]) and p.data.data_ptr() == params[k].data_ptr() and p.shape == params[k].shape and p.grad is None
        assert list(opt.state.keys()) == [p]                                   # the parameter object is still the state's key
        st = opt.state[p]
        assert torch.equal(st["step"], steps[k])
        assert st["exp_avg"] is moments[k]["exp_avg"] and st["exp_avg_sq"] is moments[k]["exp_avg_sq"]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
    assert model._cull_keep is keep


def test_swap_rows_growth_clears_a_stale_mask():
    model, opts = _stepped()
    model._cull_keep = torch.tensor([True, False, True, True, True])             # left by an earlier cull that nobody consumed
    states = SR.leaf_states(model, opts, "test")
    params, moments = _rows(states, 7, seed=3)
    SR.swap_rows(model, states, params, moments)
    assert model._cull_keep is None
    assert all(getattr(model, n).shape[0] == 7 for n in SR.NAMES)
    assert all(opt.state[p]["exp_avg"].shape == p.shape for opt, p, _ in states)


def test_no_state_and_no_optimizer():
    model, opts = _stepped(without=("rotation",), unstepped=("opacity",))
    states = SR.leaf_states(model, opts, "test")
    by_name = dict(zip(SR.NAMES, states))
    assert by_name["quats"][0] is None and by_name["quats"][2] is None
    assert by_name["opacities"][0] is opts["opacity"] and by_name["opacities"][2] is None
    params, moments = _rows(states, 3, seed=4)
    assert moments[SR.NAMES.index("quats")] is None and moments[SR.NAMES.index("opacities")] is None
    SR.swap_rows(model, states, params, moments, torch.tensor([True, True, False, True, False]))
    assert len(opts["opacity"].state) == 0                                     # no state entry appears
    assert model.quats.shape == (3, 4) and model.opacities.shape == (3, 1)
    assert len(opts["xyz"].state) == 1


def test_state_with_one_moment():
    """CullCallback prunes whichever moment exists; the kernel paths (leaf_states) take both or nothing"""
    model, opts = _stepped()
    with torch.no_grad():
        model.opacities.data = torch.tensor([[3.0], [-5.0], [3.0], [3.0], [-5.0]])       # rows 1 and 4: sigmoid < 0.1
        model.scales.data.fill_(-3.0)
    del opts["xyz"].state[model.means]["exp_avg_sq"]
    m0 = opts["xyz"].state[model.means]["exp_avg"].clone()
    assert SR.leaf_states(model, opts, "test")[0][2] is None
    assert SR.moment_ptrs([st for _, _, st in SR.leaf_states(model, opts, "test")], "exp_avg")[0] is None
    cb = CullCallback(model, opts)
    cb.run(10)
    st = opts["xyz"].state[model.means]
    assert set(st) == {"step", "exp_avg"}
    assert torch.equal(st["exp_avg"], m0[[0, 2, 3]])
    assert model.means.shape == (3, 3) and cb.n_culled == 2


def test_cull_callback():
    model, opts = _stepped()
    with torch.no_grad():
        model.opacities.data = torch.tensor([[3.0], [-5.0], [3.0], [3.0], [-5.0]])
        model.scales.data.fill_(-3.0)
    keep = torch.tensor([True, False, True, True, False])
    before = {n: getattr(model, n).detach().clone() for n in SR.NAMES}
    owners = SR.owners(model, opts)
    mom = {n: {k: owners[n][0].state[owners[n][1]][k].clone() for k in ("step",) + SR.MOMENTS} for n in SR.NAMES}
    cb = CullCallback(model, opts)
    cb.run(7)                                                                    # not a culling step
    assert cb.n_culled == 0 and model.means.shape[0] == N
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    cb.run(10)
    assert cb.n_culled == 2
    for n in SR.NAMES:
        opt, p = owners[n]
        assert p is getattr(model, n) and p.grad is None and p.data.is_contiguous()
        assert torch.equal(p.data, before[n][keep])
        st = opt.state[p]
        assert torch.equal(st["step"], mom[n]["step"])
        for k in SR.MOMENTS:
            assert torch.equal(st[k], mom[n][k][keep]) and st[k].is_contiguous()
    assert torch.equal(model._cull_keep, keep)
    cb.run(15)                                                                   # nothing left to cull: nothing changes
    assert cb.n_culled == 2 and model.means.shape[0] == 3


@pytest.mark.parametrize("what", ["refine", "mcmc.relocate"])
def test_leaf_states_refuses(what):
    model, opts = _stepped()
    with torch.no_grad():
        model.scales.data = torch.randn(3, N).t()                                # [N, 3], not contiguous
    with pytest.raises(GaussCtrlHipError, match=rf"^{what} needs contiguous float32 parameters"):
        SR.leaf_states(model, opts, what)
    model, opts = _stepped()
    opts["rotation"].state[model.quats]["exp_avg_sq"] = torch.zeros(N + 1, 4)
    with pytest.raises(GaussCtrlHipError, match=rf"^{what} needs contiguous float32 Adam moments shaped like their parameter"):
        SR.leaf_states(model, opts, what)
    model, opts = _stepped()
    opts["xyz"].state[model.means]["exp_avg"] = torch.zeros(N, 3, dtype=torch.float64)
    with pytest.raises(GaussCtrlHipError, match=rf"^{what} needs contiguous float32 Adam moments"):
        SR.leaf_states(model, opts, what)


def test_ptr_array_and_rest_floats():
    model, _ = _stepped()
    arr = SR.ptr_array([model.means.data, None, model.quats.data, None, None, None])
    assert len(arr) == 6 and arr[0] == model.means.data_ptr() and arr[1] is None and arr[2] == model.quats.data_ptr()
    assert SR.rest_floats(model) == 45
    with torch.no_grad():
        model.features_rest.data = torch.zeros(0, 15, 3)
    assert SR.rest_floats(model) == 0

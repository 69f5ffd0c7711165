"""GPU tests of the bilateral-grid colour compensation (include/gaussctrl_bilagrid.h; csrc/train_bilagrid.hip; gaussctrl_amd/bilagrid.py;
GaussCtrlModelConfig.use_bilateral_grid).

The slice and the total variation are checked against the float64 restatement of tests/_bilagrid_ref.py (F.grid_sample on 5-D input,
autograd).  Each quantity is compared as maximum error over maximum |reference|, and its bar is 16 x the error the SAME restatement shows
when it is evaluated in float32 on the same inputs (computed here, recorded through _margins.within): the kernels differ from that
float32 form only in summation order, atomics and FMA contraction, while a missing z term, a wrong pixel-centre convention or a wrong
corner weight is off by 1e-3 and more.  References are computed once per case and shared, the guarded re-runs included.

Every device input is made with _redzone.on_device or a torch factory with an explicit device, so that the red-zone re-runs at the end of
the file carve them from the arena."""
import sys

import pytest
import torch

import _bilagrid_ref as R
from _margins import within
from _redzone import guard, on_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP1 = 2.0 ** -23

# name: (C, H, W, GW, GH, L, V, view_idx) and the path of csrc/train_bilagrid.hip the shape takes
CASES = {
    "a": (1, 16, 16, 16, 16, 8, 1, [0]),            # one 16 x 16 tile reaches the whole grid: a 96 KB slab
    "b": (3, 37, 53, 16, 16, 8, 4, [2, 0, 2]),      # ragged tiles; two images add into grid 2; grids 1 and 3 receive exactly zero
    "c": (2, 20, 33, 7, 5, 4, 2, [1, 0]),           # other grid dimensions
    "d": (1, 272, 272, 16, 16, 8, 1, [0]),          # a cell (18 pixels) wider than a tile: slabs of 2 and 3 vertices per axis
    "e": (1, 1, 1, 2, 2, 2, 1, [0]),                # smallest shapes
    "f": (2, 19, 21, 64, 48, 8, 2, [1, 1]),         # a 704 KB slab: the global-atomic fallback (both images into one grid)
    "g": (2, 512, 512, 16, 16, 8, 2, [1, 0]),       # 512 workgroups of 32 x 32 pixels: the large-tile policy
}


def _case(name):
    return R.slice_case(name, *CASES[name], seed=7)


def _slice_on_device(c):
    from gaussctrl_amd import bilagrid
    g = on_device(c["grids"], DEV).requires_grad_(True)
    x = on_device(c["rgb"], DEV).requires_grad_(True)
    out = bilagrid.bilagrid_apply(g, x, c["view_idx"])
    out.backward(on_device(c["v_out"], DEV))
    return out.detach(), g.grad, x.grad


# ------------------------------------------------------------------------------------------------------------------ 1. slice vs float64
@pytest.mark.parametrize("name", sorted(CASES))
def test_slice_vs_fp64(name):
    c = _case(name)
    got = _slice_on_device(c)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    for what, t, ref, e32 in zip(("out", "v_grids", "v_rgb"), got, c["ref"], c["f32_err"]):
        err = R.rel_err(t, ref)
        print(f"case {name} {what}: kernel {err:.3e}, float32 restatement {e32:.3e}, bar {16 * e32:.3e}")
    for what, t, ref, e32 in zip(("out", "v_grids", "v_rgb"), got, c["ref"], c["f32_err"]):
        within(f"case {name} {what}: max |kernel - fp64| / max |fp64|", R.rel_err(t, ref), 16 * e32)
    V, idx = CASES[name][6], set(c["view_idx"])
    for v in range(V):
        if v not in idx:                                   # a grid no image names is not touched
            assert int(torch.count_nonzero(got[1][v])) == 0, v


# ------------------------------------------------------------------------------------------------------------------ 2. identity
def test_identity_grid_changes_nothing():
    """the identity grid returns its input, and v_rgb = v_out, within 4 ulp of 1.0 (|rgb| <= 1.15, |v_out| <= 1: the interpolation weights
    sum to 1 in float32 only up to rounding, so it is not bit-exact); dA/dz of a constant grid is exactly zero"""
    from gaussctrl_amd import bilagrid
    g = torch.Generator().manual_seed(11)
    rgb = torch.rand(2, 37, 53, 3, generator=g) * 1.3 - 0.15
    v_out = torch.rand(2, 37, 53, 3, generator=g) * 2 - 1
    grids = bilagrid.identity_grids(3, 16, 16, 8, DEV).requires_grad_(True)
    assert grids.shape == (3, 12, 8, 16, 16) and torch.equal(grids[1, :, 3, 5, 7].cpu(), torch.tensor(R.IDENTITY))
    x = on_device(rgb, DEV).requires_grad_(True)
    out = bilagrid.bilagrid_apply(grids, x, [2, 0])
    out.backward(on_device(v_out, DEV))
    within("identity: max |out - rgb|", float((out.detach().cpu() - rgb).abs().max()), 4 * ULP1)
    within("identity: max |v_rgb - v_out|", float((x.grad.cpu() - v_out).abs().max()), 4 * ULP1)
    assert int(torch.count_nonzero(grids.grad[1])) == 0 and float(grids.grad[2].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 3. total variation
@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("shape", [(16, 16, 8), (7, 5, 4)], ids=["16x16x8", "7x5x4"])
def test_tv_vs_fp64(V, shape):
    """the value, and the weight-scaled gradient ADDED onto a non-zero buffer, through the C ABI; then the host layer's value and gradient"""
    import ctypes as C
    from gaussctrl_amd import _lib as L, bilagrid
    GW, GH, Lz = shape
    c = R.tv_case(V, GW, GH, Lz, seed=3)
    tv_ref, grad_ref = c["ref"]
    e_val, e_grad = c["f32_err"]
    g = on_device(c["grids"], DEV)
    weight = 0.37
    gen = torch.Generator().manual_seed(5)
    base = torch.randn(c["grids"].shape, generator=gen) * float(grad_ref.abs().max()) * weight
    v = on_device(base, DEV)
    tv = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    lib = L.lib()
    nbytes = lib.gcx_bilagrid_tv_workspace_bytes(L.i32(V), L.i32(GW), L.i32(GH), L.i32(Lz))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    L.check(lib.gcx_bilagrid_tv_fwd_bwd(L.i32(V), L.i32(GW), L.i32(GH), L.i32(Lz), L.ptr(g), L.f32(weight), L.ptr(tv), L.ptr(v), L.ptr(ws),
                                        C.c_size_t(nbytes), L.stream_ptr()), "gcx_bilagrid_tv_fwd_bwd")
    want = base.double() + weight * grad_ref
    err_v = float(abs(float(tv[0]) - float(tv_ref)) / abs(float(tv_ref)))
    err_g = float((v.double().cpu() - want).abs().max() / (weight * grad_ref.abs().max()))
    print(f"tv V={V} {shape}: value {err_v:.3e} (float32 restatement {e_val:.3e}), gradient {err_g:.3e} (float32 restatement {e_grad:.3e})")
    within(f"tv V={V} {shape}: |value - fp64| / fp64", err_v, 16 * e_val)
    within(f"tv V={V} {shape}: max |buffer - (buffer + weight * fp64 gradient)| / max", err_g, 16 * e_grad)
    gl = on_device(c["grids"], DEV).requires_grad_(True)
    loss = bilagrid.bilagrid_tv_loss(gl)
    (3.0 * loss).backward()
    within(f"tv V={V} {shape}: host layer value", abs(float(loss) - float(tv_ref)) / abs(float(tv_ref)), 16 * e_val)
    within(f"tv V={V} {shape}: host layer gradient", R.rel_err(gl.grad / 3.0, grad_ref), 16 * e_grad)


# ------------------------------------------------------------------------------------------------------------------ 4. autograd wiring
def test_autograd_through_the_loss_accumulates():
    """bilagrid_apply -> l1_ssim_loss, backward to the grid and to a leaf image; a second backward doubles .grad (float atomics: to 1e-5)"""
    from gaussctrl_amd import bilagrid
    from gaussctrl_amd.train_ops import l1_ssim_loss
    grids, rgb, _ = R.make_inputs(1, 24, 40, 16, 16, 8, 2, seed=21)
    target = torch.rand(24, 40, 3, generator=torch.Generator().manual_seed(22))
    g = on_device(grids, DEV).requires_grad_(True)
    x = on_device(rgb, DEV).requires_grad_(True)
    t = on_device(target, DEV)
    loss = l1_ssim_loss(bilagrid.bilagrid_apply(g, x, [1])[0], t, 0.2)
    loss.backward()
    g1, x1 = g.grad.clone(), x.grad.clone()
    assert float(g1[1].abs().max()) > 0 and int(torch.count_nonzero(g1[0])) == 0 and float(x1.abs().max()) > 0
    l1_ssim_loss(bilagrid.bilagrid_apply(g, x, [1])[0], t, 0.2).backward()
    within("second backward: max |grad - 2 grad| / max (grid)", float((g.grad - 2 * g1).abs().max()), 1e-5 * float(g1.abs().max()))
    within("second backward: max |grad - 2 grad| / max (image)", float((x.grad - 2 * x1).abs().max()), 1e-5 * float(x1.abs().max()))
    # what arrives is the loss's own gradient: the same slice, cut from the loss and fed that gradient by hand, gives the same two results
    # (the same additions, the float atomics in another order: 1e-5 of the maximum)
    g2 = on_device(grids, DEV).requires_grad_(True)
    x2 = on_device(rgb, DEV).requires_grad_(True)
    o2 = bilagrid.bilagrid_apply(g2, x2, [1])
    od = o2.detach().requires_grad_(True)
    l1_ssim_loss(od[0], t, 0.2).backward()
    o2.backward(od.grad)
    within("cut at the loss: max |grid gradient - chained| / max", float((g2.grad - g1).abs().max()), 1e-5 * float(g1.abs().max()))
    within("cut at the loss: max |image gradient - chained| / max", float((x2.grad - x1).abs().max()), 1e-5 * float(x1.abs().max()))


def test_host_layer_refuses_bad_arguments():
    from gaussctrl_amd import bilagrid
    from gaussctrl_amd._lib import GaussCtrlHipError
    g = bilagrid.identity_grids(2, 4, 4, 4, DEV)
    x = torch.zeros(1, 8, 8, 3, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="outside"):
        bilagrid.bilagrid_apply(g, x, [2])
    with pytest.raises(ValueError, match="view indices"):
        bilagrid.bilagrid_apply(g, x, [0, 1])
    with pytest.raises(ValueError, match="rgb must be"):
        bilagrid.bilagrid_apply(g, x[0], [0])
    with pytest.raises(GaussCtrlHipError):
        bilagrid.bilagrid_apply(g, x.cpu(), [0])
    assert float(bilagrid.bilagrid_tv_loss(bilagrid.identity_grids(0, 4, 4, 4, DEV))) == 0.0            # no grid: nothing launched, 0
    assert float(bilagrid.bilagrid_tv_loss(g)) == 0.0                                                   # constant grids: exactly 0


# ------------------------------------------------------------------------------------------------------------------ 5. model, end to end
GAINS = ((1.20, 0.04), (1.32, -0.02), (1.10, 0.06), (1.26, 0.01))          # (gain, offset) of the four views: all brighter, each differently
STEPS = 60


def _train(P, cams, targets, use_grid):
    from gaussctrl_amd.gc_config import build_optimizers
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    torch.manual_seed(0)
    # bilagrid_lr 2e-2, not the default 2e-3: Adam moves a parameter by about its learning rate per step, and a view's grid is stepped
    # only when that view is drawn -- 15 of the 60 steps.  At 2e-3 a gain entry could move by about 0.03, against gains of 1.10 to 1.32
    # to absorb, while features_dc (2.5e-3, stepped every time) would do nearly all of the work in both runs: the default rate is
    # meant for the thousands of steps of a real run and is not what this short run examines
    cfg = GaussCtrlModelConfig(background_color="black", use_bilateral_grid=use_grid, bilagrid_lr=2e-2)
    model = GaussCtrlModel(cfg, params={k: v.copy() for k, v in P.items()}, device=DEV, num_train_data=len(targets))
    opts = build_optimizers(model)
    dc0 = model.features_dc.detach().clone()
    keys = None
    for step in range(STEPS):
        view = step % len(targets)
        for o in opts.values():
            o.zero_grad(set_to_none=True)
        outputs = model(cams[view])
        loss = model.get_loss_dict(outputs, {"image": targets[view], "image_idx": view})
        keys = set(loss)
        sum(loss.values()).backward()
        for o in opts.values():
            o.step()
    final = 0.0
    with torch.no_grad():
        for view in range(len(targets)):
            final += float(model.get_loss_dict(model(cams[view]), {"image": targets[view], "image_idx": view})["main_loss"]) / len(targets)
    drift = float((model.features_dc.detach() - dc0).abs().mean())
    return model, opts, keys, final, drift


def test_model_end_to_end():
    """2000 Gaussians, 4 views of 64 x 64 whose targets are the scene's own renders, each through its own gain and offset; 60 steps with
    the switch on and off from the same seeds.  Directions only: with the grids the final main loss (mean over the views) is lower, the DC
    colours moved less (the tone drift went into the grids), the grids left the identity, and evaluation does not see them."""
    from gaussctrl_amd import bilagrid, synthetic as syn
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.ns_compat import Cameras
    P = syn.make_gaussians(2000, seed=4, scale_mean=0.05)
    cams = Cameras(syn.make_cameras(4, seed=12), 60.0, 60.0, 32.0, 32.0, 64, 64)
    clean = GaussCtrlModel(GaussCtrlModelConfig(background_color="black"), params={k: v.copy() for k, v in P.items()}, device=DEV)
    targets = [clean.get_outputs_for_camera(cams[i])["rgb"] * gain + off for i, (gain, off) in enumerate(GAINS)]
    on, opts_on, keys_on, loss_on, drift_on = _train(P, cams, targets, True)
    off, opts_off, keys_off, loss_off, drift_off = _train(P, cams, targets, False)
    print(f"end to end: main loss {loss_on:.5f} (grids) vs {loss_off:.5f}; mean |features_dc - initial| {drift_on:.5f} (grids) vs {drift_off:.5f}")
    # switch off: nothing new
    assert keys_off == {"main_loss"} and set(opts_off) == {"xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation"}
    assert not hasattr(off, "bilateral_grid") and "bilateral_grid" not in off.state_dict()
    # switch on
    assert keys_on == {"main_loss", "tv_loss"} and set(opts_on) == set(opts_off) | {"bilateral_grid"}
    assert opts_on["bilateral_grid"].param_groups[0]["lr"] == 2e-2 and opts_on["bilateral_grid"].param_groups[0]["eps"] == 1e-15
    assert "bilateral_grid" in on.state_dict() and on.bilateral_grid.shape == (4, 12, 8, 16, 16)
    assert loss_on < loss_off
    assert drift_on < drift_off
    moved = float((on.bilateral_grid.detach() - bilagrid.identity_grids(4, 16, 16, 8, DEV)).abs().max())
    print(f"end to end: max |grid - identity| {moved:.4f}")
    assert moved > 1e-3
    # evaluation never sees the grids: the same parameters without the switch render the same bits
    plain = GaussCtrlModel(GaussCtrlModelConfig(background_color="black"),
                           params={k: getattr(on, k).detach().cpu().numpy() for k in P}, device=DEV)
    for i in range(4):
        a, b = on.get_outputs_for_camera(cams[i]), plain.get_outputs_for_camera(cams[i])
        assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["depth"], b["depth"])
    many = on.get_outputs_for_cameras([cams[i] for i in range(4)])
    assert all(torch.equal(m["rgb"], plain.get_outputs_for_camera(cams[i])["rgb"]) for i, m in enumerate(many))
    # training-mode outputs are un-gridded too: the grid acts inside the loss only
    on.train(); plain.train()
    assert torch.equal(on(cams[0])["rgb"], plain(cams[0])["rgb"])
    with pytest.raises(ValueError, match="image_idx"):
        on.get_loss_dict(on(cams[0]), {"image": targets[0], "image_idx": 4})


# ------------------------------------------------------------------------------------------------------------------ 6. red zones
def _guarded(fn, nbytes, **kw):
    from gaussctrl_amd import bilagrid
    with guard(bilagrid, sys.modules[__name__], nbytes=nbytes):
        fn(**kw)


@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_guarded_slice(name):
    """test 1 again with the grids, the images, both gradients and the output inside a red-zone arena: the NaN-poisoned zones catch a
    weight-zero read of the vertex past a border, the zone check a store past an image or a grid"""
    _guarded(test_slice_vs_fp64, 64 << 20, name=name)


def test_guarded_tv():
    _guarded(test_tv_vs_fp64, 64 << 20, V=4, shape=(7, 5, 4))

"""GPU: render_view(cam) against render_views([cam]) over every combination of the four switches of the fused render -- depth_grad, absgrad,
antialiased and grad_into (with grad_accumulate).  Both go through ONE compositing backward and ONE projection backward on the host
(gsplat_ops._composite_bwd / _project_bwd) and the same tile walk on the device (csrc/raster_tile.h); the single-view call is the C = 1 case.

Scene: (a) of tests/test_raster_depth_gpu.py (3000 Gaussians, 72 x 40: 5 x 3 tiles, partial in both directions, lists longer than one
256-record staging batch).  Forward outputs are compared bit for bit (the forward is deterministic).  Gradients pass through float atomics,
whose order differs from run to run, so they are held to the project's bar for such sums: 1e-3 of the tensor's largest magnitude
(DESIGN.md section 2)."""
import itertools

import numpy as np
import pytest
import torch

from test_raster_depth_gpu import BG, KEYS, _cotangents, _leaves, _scene, _t

pytestmark = pytest.mark.gpu
INTO = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def _run(batched, depth_grad, absgrad, antialiased, into):
    """one forward + backward; returns (forward outputs, gradients) as dicts of CPU arrays"""
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.camera import camera_to_gsplat
    P, c2w, K = _scene("a")
    H, W = K["H"], K["W"]
    cam = camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], W, H)
    tp = _leaves(P)
    aux = ops.RenderAux()
    aux.depth_grad, aux.absgrad, aux.antialiased = depth_grad, absgrad, antialiased
    if into:        # the backward ADDS into buffers that already hold something
        aux.grad_into = {k: torch.full(tp[k].shape if k != "opacities" else (tp[k].shape[0],), 0.25, device=tp[k].device) for k in INTO}
        aux.grad_accumulate = True
    if batched:
        rgb, alpha, depth = (t[0] for t in ops.render_views(*(tp[k] for k in KEYS), [cam], _t(BG), True, 3, aux))
    else:
        rgb, alpha, depth = ops.render_view(*(tp[k] for k in KEYS), cam, _t(BG), True, 3, aux)
    assert aux.xys_grad is None and aux.xys_absgrad is None and depth.requires_grad == depth_grad
    bins = aux.tile_bins.reshape(-1, 2).cpu().numpy()
    assert bins.shape[0] == 15 and W % 16 and H % 16 and (bins[:, 1] - bins[:, 0]).max() > 256      # multi-batch staging, partial tiles
    fwd = dict(rgb=rgb, alpha=alpha, depth=depth, final_index=aux.final_index.reshape(H, W))
    if antialiased:
        fwd["compensation"] = aux.compensation.reshape(-1)
    fwd = {k: v.detach().cpu().numpy() for k, v in fwd.items()}
    v_rgb, v_a, v_d = (_t(c) for c in _cotangents(H, W, 7))
    loss = (rgb * v_rgb).sum() + (alpha * v_a).sum()
    if depth_grad:
        loss = loss + (torch.where(depth != 1000.0, depth, torch.zeros_like(depth)) * v_d).sum()
    loss.backward()
    if into:
        assert all(tp[k].grad is None for k in KEYS)
        grads = {k: aux.grad_into[k].reshape(tp[k].shape) for k in INTO}
    else:
        grads = {k: tp[k].grad for k in KEYS}
    grads["xys_grad"] = aux.xys_grad.reshape(-1, 2)
    assert (aux.xys_absgrad is not None) == absgrad
    if absgrad:
        grads["xys_absgrad"] = aux.xys_absgrad.reshape(-1, 2)
    return fwd, {k: v.detach().cpu().numpy() for k, v in grads.items()}


@pytest.mark.parametrize("depth_grad,absgrad,antialiased,into", list(itertools.product((False, True), repeat=4)))
def test_render_view_is_render_views_of_one_camera(depth_grad, absgrad, antialiased, into):
    f1, g1 = _run(False, depth_grad, absgrad, antialiased, into)
    fC, gC = _run(True, depth_grad, absgrad, antialiased, into)
    assert sorted(f1) == sorted(fC) and sorted(g1) == sorted(gC)
    for k in f1:
        assert f1[k].shape == fC[k].shape and np.array_equal(f1[k], fC[k]), k
    assert (f1["depth"] == 1000.0).any() and (f1["depth"] != 1000.0).any()
    for k in g1:
        top = np.abs(gC[k]).max()
        assert top > 0, k
        err = np.abs(g1[k] - gC[k]).max()
        print(f"{k}: max |render_view - render_views| = {err:.3e}, bar {1e-3 * top:.3e}")
        assert err <= 1e-3 * top, k

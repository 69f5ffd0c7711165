"""CPU side of the projection / SH backward tests with the camera inside the cloud (tests/_inside_scene.py; GPU side:
tests/test_project_vjp_gpu.py).  Nothing here needs a GPU: it shows that the populations the GPU tests rely on exist, that the reference is
decided (float32 and float64 make the same discrete choices), where the bars come from, that the C oracle's hand-derived backward holds
them, and that they would catch a wrong frustum-clamp branch.

Census (float64; x- / x+ = visible rows clamped at -lim / +lim, lim = 1.3 * half-fov; dark = colour channels of visible rows at 0):

    scene        visible  x- / x+   y- / y+    both  behind  tz < 0.2  full-image boxes  dark  max radius
    in3            759    66 / 54   64 / 104    61    923       25           22           136     1658
    in7            990    63 / 57   98 / 120    63    569       33           23           173      630
    tiny            98     9 / 30   20 / 33     22     76        5           16           154      262
    views9 (min)   596    51 / 45   64 / 91     54    526       18           16           119      579
    views9 (max)  1033    69 / 68   95 / 141    63   1165       33           32           205     2312

(seeds 3 and 7 meet every floor of test_census_floors; no replacement seed was needed)

float32 against float64 front_ref, worst e_row over every scene, view, SH mode and cotangent set (aa off) -- BARS is four times these:

    means 1.16e-4   log-scales 8.24e-6   quaternions (floored) 2.75e-6   opacity logits 3.12e-5   features_dc 1.93e-7   features_rest 3.09e-7
    forward (FWD_BARS; two CPUs, see _inside_scene.py): xys 1.59e-6 / 1.65e-6   depths 1.65e-6 / 2.65e-6   conics 2.89e-6 / 5.35e-6
                                                        rgbs 9.19e-8   opac 4.35e-8

The means figure comes from the conic-only set, where the mean's gradient is the frustum path alone and cancels on a few large Gaussians
(99 % of the rows are below 2.1e-6; with every cotangent at once the worst row is 1.2e-6).  Both precisions take the float32 camera
matrices the kernels are handed, so the distance is arithmetic alone (with a float64 camera: quaternions 4.24e-6, depths 4.34e-6).
On a second CPU the backward figures are the same to three digits except log-scales, 7.99e-6.

Sensitivity (float64 reference with a straight-through frustum clamp against the true one, conic-only cotangents, means): every clamped row
exceeds the means bar -- in3 227 of 227, in7 275 of 275 -- and no unclamped row moves at all.  The whole-tensor bar of test_raster_gpu.
_grad_close (1e-3 of the tensor's max) catches 210 / 238 of them under the conic-only set and 0 / 0 under the mixed set (a), which is what a
render's gradients look like; under (a) the row metric still catches 33 / 58 at the means bar.
"""
import numpy as np
import pytest
import torch

import _inside_scene as S
from _margins import within

INSIDE = ("in3", "in7")


@pytest.mark.parametrize("name", INSIDE)
def test_census_floors(name):
    """a GPU test cannot pass on an empty population: the inside scenes hold every kind of row, with margin"""
    c, = S.census(name)
    assert min(c["clamp_x"]) >= 10 and sum(c["clamp_x"]) >= 50, c
    assert min(c["clamp_y"]) >= 10 and sum(c["clamp_y"]) >= 50, c
    assert c["clamp_both"] >= 20 and c["behind"] >= 300 and c["near"] >= 10 and c["full_boxes"] >= 5 and c["dark_channels"] >= 30, c
    assert c["visible"] >= 500 and c["max_radius"] > 500, c


@pytest.mark.parametrize("name", ["tiny", "views9"])
def test_census_nonempty(name):
    """every view of the small and of the batched scene has rows of each kind"""
    rows = S.census(name)
    assert len(rows) == (9 if name == "views9" else 1)
    for c in rows:
        assert min(c["clamp_x"]) > 0 and min(c["clamp_y"]) > 0 and c["clamp_both"] > 0 and c["behind"] > 0 and c["near"] > 0, c
        assert c["full_boxes"] > 0 and c["dark_channels"] > 0 and c["visible"] > 0, c
    if name == "tiny":
        assert rows[0]["visible"] == 98 and S.scene("tiny")[0]["means"].shape[0] == 299


@pytest.mark.parametrize("name", list(S.SCENES))
def test_float32_and_float64_reference_make_the_same_choices(name):
    """radii, num_tiles_hit and the colour mask rgbs > 0 of front_ref do not depend on its precision, in any view and SH mode"""
    P, c2ws, K = S.scene(name)
    for c2w in c2ws:
        for deg, n_use in S.SH_MODES:
            o32, _ = S.front_ref(P, c2w, K, deg, n_use, False, None, torch.float32)
            o64, _ = S.front_ref(P, c2w, K, deg, n_use, False, None, torch.float64)
            assert np.array_equal(o32["radii"], o64["radii"]) and np.array_equal(o32["num_tiles_hit"], o64["num_tiles_hit"]), (deg, n_use)
            assert np.array_equal(o32["rgbs"] > 0, o64["rgbs"] > 0), (deg, n_use)


@pytest.mark.parametrize("name,views", [("in3", (0,)), ("in7", (0,)), ("views9", S.RENDER_VIEWS)])
def test_render_scenes_are_decided(name, views):
    """the whole-render scenes of test_project_vjp_gpu.py: rt.get_outputs in float32 and float64 agrees on radii, sorted ids, tile bins,
    final_index and the far mask, and max |rgb32 - rgb64| <= 1e-5 (the convention of the antialias and depth test files)"""
    from oracle import raster_torch as rt
    P, c2ws, K = S.scene(name)
    for v in views:
        o = [rt.get_outputs({k: torch.tensor(x) for k, x in P.items()}, torch.tensor(c2ws[v]), K["fx"], K["fy"], K["cx"], K["cy"], K["W"],
                            K["H"], torch.tensor([0.1, 0.2, 0.3]), training=False, dtype=dt) for dt in (torch.float32, torch.float64)]
        for k in ("radii", "gaussian_ids_sorted", "tile_bins", "final_index"):
            assert torch.equal(o[0][k], o[1][k]), (v, k)
        assert torch.equal(o[0]["depth"] == 1000.0, o[1]["depth"] == 1000.0), v
        within("max |rgb32 - rgb64|", float((o[0]["rgb"].double() - o[1]["rgb"]).abs().max()), 1e-5)
        tiles = (o[1]["tile_bins"][:, 1] - o[1]["tile_bins"][:, 0])
        assert int(tiles.max()) > 150 and int(o[1]["radii"].max()) > 400                # lists from Gaussians hundreds of pixels wide


@pytest.mark.parametrize("name", INSIDE)
def test_c_oracle_projection_backward_vs_float64(oracle_c, name):
    """oracle_c.project_gaussians_bwd (hand-derived; the kernels' project_one_bwd mirrors it) against float64 autograd of
    rt.project_gaussians on the SAME float32 inputs (exp'd scales, normalised quaternions, camera matrices), per row at BARS, for the
    cotangent sets a to d and once without a depth cotangent.  The scale gradient is compared as the log-scale one (v_s * s)."""
    from oracle import raster_torch as rt
    P, c2ws, K = S.scene(name)
    W, H = K["W"], K["H"]
    V, full = oracle_c.camera_glue(c2ws[0], K["fx"], K["fy"], W, H)
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    scales = np.exp(P["scales"]).astype(np.float32)
    qn = (P["quats"] / np.linalg.norm(P["quats"], axis=-1, keepdims=True)).astype(np.float32)
    cam = (K["fx"], K["fy"], K["cx"], K["cy"], H, W)
    xys, depths, radii, conics, nth, _ = oracle_c.project_gaussians(P["means"], scales, 1.0, qn, V[:3], full, *cam, tb)
    m, s, q = (torch.tensor(a, dtype=torch.float64).requires_grad_(True) for a in (P["means"], scales, qn))
    out = rt.project_gaussians(m, s, 1.0, q, torch.tensor(V[:3], dtype=torch.float64), torch.tensor(full, dtype=torch.float64), *cam, tb)
    assert np.array_equal(out[2].numpy(), radii) and np.array_equal(out[4].numpy(), nth)
    for cset, depth in (("a", True), ("a", False), ("b", False), ("c", False), ("d", False)):
        cot = {k: c[0] for k, c in S.cotangents(name, cset, depth).items() if k in ("xys", "depths", "conics")}
        loss = sum((o * torch.tensor(cot[k], dtype=torch.float64)).sum() for k, o in (("xys", out[0]), ("depths", out[1]), ("conics", out[3]))
                   if k in cot)
        ref = [np.zeros(t.shape) if g is None else g.numpy()
               for t, g in zip((m, s, q), torch.autograd.grad(loss, (m, s, q), retain_graph=True, allow_unused=True))]
        zero = lambda k, *sh: cot.get(k, np.zeros((radii.shape[0],) + sh, np.float32))
        vm, vs, vq = oracle_c.project_gaussians_bwd(P["means"], scales, 1.0, qn, V[:3], full, *cam, radii, conics, zero("xys", 2),
                                                    cot.get("depths"), zero("conics", 3))
        ls_den = S.row_norms(ref[1] * scales)
        for k, got, want, den in (("means", vm, ref[0], S.row_norms(ref[0])), ("scales", vs * scales, ref[1] * scales, ls_den),
                                  ("quats", vq, ref[2], S.row_norms(ref[2]) + ls_den)):
            within(f"C oracle, set {cset}{'+depth' if depth else ''}: {k} worst row error", S.row_errors(got, want, den)[0], S.BARS[k])


def test_bars_are_four_times_the_reference_distance():
    """BARS can neither be exceeded by the reference itself nor be set loose: bar / 8 <= worst float32-vs-float64 e_row <= bar / 3"""
    worst = S.reference_distances()
    print("float32 vs float64 front_ref, worst e_row:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k in S.KEYS:
        assert S.BARS[k] / 8 <= worst[k] <= S.BARS[k] / 3, (k, worst[k], S.BARS[k])


@pytest.mark.parametrize("name", INSIDE)
def test_a_wrong_clamp_branch_would_be_caught(name):
    """The float64 reference with a straight-through frustum clamp (what a wrong clx / cly routing at the end of project_one_bwd computes)
    against the true one, conic-only cotangents: it exceeds the means bar on at least half of the clamped rows and on no unclamped row."""
    clamped, unclamped = S.clamped_rows(name)
    true, wrong = S.ref_views(name, cset="b"), S.ref_views(name, cset="b", straight_through=True)
    d = S.row_norms(wrong["sum"]["means"] - true["sum"]["means"])
    den = true["den"]["means"]
    assert np.all(den[clamped | unclamped] > 0)
    e = d / np.where(den > 0, den, 1.0)
    caught = int((e[clamped] > S.BARS["means"]).sum())
    old = np.abs(wrong["sum"]["means"] - true["sum"]["means"]).max(axis=1) > 1e-3 * np.abs(true["sum"]["means"]).max()
    print(f"{name}: {caught} of {int(clamped.sum())} clamped rows beyond the means bar; the whole-tensor 1e-3 bar catches {int(old[clamped].sum())}")
    assert 2 * caught >= int(clamped.sum()) > 100
    assert float(e[unclamped].max()) <= S.BARS["means"] and int(unclamped.sum()) > 300
    for k in S.KEYS[1:]:                                      # the clamp is on the mean's path alone
        assert np.abs(wrong["sum"][k] - true["sum"][k]).max() <= 1e-12 * max(1.0, np.abs(true["sum"][k]).max()), k


def test_forward_bars_are_four_times_the_reference_distance():
    """the per-row bars of the forward outputs (_inside_scene.FWD_BARS) are four times the larger of the distances measured on two CPUs
    (the float32 matmul's summation order is the BLAS's): the upper edge of the window is BARS' own, the lower one leaves room for that"""
    worst = S.forward_distances()
    print("float32 vs float64 front_ref, forward, worst e_row:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k in S.FWD_BARS:
        assert S.FWD_BARS[k] / 16 <= worst[k] <= S.FWD_BARS[k] / 3, (k, worst[k], S.FWD_BARS[k])


def test_reference_camera_is_the_product_camera():
    """front_ref hands both precisions the float32 matrices of oracle.raster_c.camera_glue: the product's camera_to_gsplat bit for bit"""
    from gaussctrl_amd.camera import camera_to_gsplat
    from oracle import raster_c
    for name in S.SCENES:
        _, c2ws, K = S.scene(name)
        for c2w in c2ws:
            cam = camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], K["W"], K["H"])
            V, full = raster_c.camera_glue(c2w, K["fx"], K["fy"], K["W"], K["H"])
            assert V.dtype == np.float32 and np.array_equal(V[:3].reshape(-1), np.asarray(cam["viewmat"], np.float32))
            assert full.dtype == np.float32 and np.array_equal(full.reshape(-1), np.asarray(cam["fullproj"], np.float32))
            assert np.array_equal(np.asarray(c2w, np.float32)[:3, 3], np.asarray(cam["origin"], np.float32))

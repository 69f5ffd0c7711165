"""The crafted compositing scenes of tests/_composite_scene.py and their float64 closed form, checked on the CPU: census floors, no knife
edge, the closed form against float64 autograd of oracle.raster_torch.rasterize on the same lists, xy_abs against the per-pixel construction
of _absgrad_ref.py, the C oracle (float32) against the closed form per row, the bars against what they are eight times of, and the
sensitivity of the row metric to five faults the whole-tensor bar of test_raster_gpu._grad_close does not see."""
import numpy as np
import pytest
import torch

import _composite_scene as cs
from _margins import within

F32, F64 = np.float32, np.float64
VARIANTS = [(0, False), (1, False), (2, False), (1, True), (2, True)]          # every (view, own_opac) the GPU tests use


def _tb(sc):
    return (sc["tiles"][0], sc["tiles"][1], 1)


@pytest.mark.parametrize("name", cs.SCENES)
def test_census_floors(name):
    c = cs.census(name)
    print(name, c)
    if name == "deep":
        assert c["stopped"] == 0 and c["above_one"] == 0 and c["two_batch_tiles"] >= 3 and c["valid_per_pixel"] > 50
    if name == "stop":
        assert c["stopped"] >= 0.30 and c["kmax_before_end"] >= 64 and c["wmax_span"] >= 64 and c["two_batch_tiles"] >= 1
    if name == "opaque":
        assert c["faint"] >= 50 and c["capped"] >= 5 and c["ra_over_100"] >= 5 and c["above_one"] > 0 and c["alpha_zero"] > 0
        assert c["above_one"] < 3 * c["pixels"]
    if name == "tiny":
        assert c["pixels"] == 17 * 9


@pytest.mark.parametrize("name", cs.SCENES)
def test_no_knife_edge(name):
    """no (pixel, entry) and no pixel is inside 16 x the float32-float64 difference of its quantity, in any variant of the scene; then both
    precisions decide alike: final_index and the clamp mask are identical"""
    for view, own in VARIANTS:
        sc = cs.scene(name, view, own)
        k = cs.knife_edges(sc)
        print(name, view, own, "redrawn", sc["redrawn"], {q: f"{k['dist'][q]:.3g} >= {k['margin'][q]:.3g}" for q in k["margin"]}, f"far {k['far']:.3g}")
        assert not k["owners"]
        for q in k["margin"]:
            assert k["dist"][q] >= k["margin"][q], (q, k["dist"][q], k["margin"][q])
        assert k["far"] < 0.5                     # a pair further than 1 from its threshold moves by less than half its distance
        f64, f32 = cs.forward(sc, F64), cs.forward(sc, F32)
        assert np.array_equal(f64["final_index"], f32["final_index"])
        assert np.array_equal(f64["image"] > 1, f32["image"] > 1)
        a = 1 - f64["final_Ts"]
        assert np.all((a == 0) | (a >= float(cs.ALPHA_MIN) * (1 - 1e-12)))


def _kernel_constants(monkeypatch):
    """the oracle with the float32 constants the kernels (and the closed form, in both precisions) compare against"""
    from oracle import raster_torch as rt
    monkeypatch.setattr(rt, "ALPHA_CAP", float(cs.ALPHA_CAP))
    monkeypatch.setattr(rt, "ALPHA_MIN", float(cs.ALPHA_MIN))
    monkeypatch.setattr(rt, "T_STOP", float(cs.T_STOP))
    return rt


def _autograd(rt, sc, cot, C, depth, clamp):
    col, bg = cs.colors_nd(sc, C)
    leaves = [torch.tensor(np.asarray(a, F64), requires_grad=True) for a in (sc["xys"], sc["conics"], col, sc["opac"], sc["extra"])]
    out, alpha, fidx, E = rt.rasterize(leaves[0], leaves[1], leaves[2], leaves[3], torch.tensor(sc["ids_sorted"]), torch.tensor(sc["tile_bins"]),
                                       sc["H"], sc["W"], _tb(sc), torch.tensor(np.asarray(bg, F64)), extra=leaves[4])
    if clamp:
        out = torch.clamp(out, max=1.0)
    loss = (out * torch.tensor(cot["v_out"].astype(F64))).sum()
    if cot["v_alpha"] is not None:
        loss = loss + (alpha * torch.tensor(cot["v_alpha"].astype(F64))).sum()
    if depth and cot["v_depth"] is not None:
        pos = alpha > 0
        dep = torch.where(pos, E / torch.where(pos, alpha, torch.ones_like(alpha)), torch.full_like(E, 1000.0))
        loss = loss + (dep * torch.tensor(cot["v_depth"].astype(F64))).sum()
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    g = [np.zeros(l.shape) if x is None else x.numpy() for l, x in zip(leaves, gs)]
    return {"v_xy": g[0], "v_conic": g[1], "v_colors": g[2], "v_opacity": g[3], "v_extra": g[4]}, fidx.numpy()


@pytest.mark.parametrize("name", cs.SCENES)
def test_closed_form_is_the_oracles_autograd(name, monkeypatch):
    rt = _kernel_constants(monkeypatch)
    sc = cs.scene(name)
    for C, cset, depth, clamp in ((3, "a", True, False), (3, "a", False, True), (3, "d", True, False), (5, "a", False, False), (5, "c", False, False)):
        col, bg = cs.colors_nd(sc, C)
        cot = cs.cotangents(sc, cset, C, depth)
        ref = cs.pair_backward(sc, cot, F64, depth, col, bg, clamp)
        auto, fidx = _autograd(rt, sc, cot, C, depth, clamp)
        assert np.array_equal(fidx, cs.forward(sc, F64, col, bg)["final_index"])
        for k in ref:
            if k != "xy_abs":
                within(f"{name} C={C} {cset}: {k} closed form vs autograd", cs.row_errors(auto[k], ref[k][0], ref[k][1])[0], 1e-12)


def test_xy_abs_is_the_per_pixel_construction_on_tiny(monkeypatch):
    """tests/_absgrad_ref.py's construction: every pixel composites from its own copy of the tile's centres, |g_p| summed over the pixels"""
    rt = _kernel_constants(monkeypatch)
    sc = cs.scene("tiny")
    cot = cs.cotangents(sc, "a", 3, True)
    t = {k: torch.tensor(np.asarray(sc[k], F64)) for k in ("xys", "conics", "colors", "opac", "extra", "background")}
    v = {k: torch.tensor(a.astype(F64)) for k, a in cot.items()}
    want = np.zeros((sc["N"], 2))
    for tile, (s, e) in enumerate(sc["tile_bins"].tolist()):
        gid = torch.tensor(sc["ids_sorted"][s:e].astype(np.int64))
        py, px = cs._tile_pixels(sc, tile)
        leaves, total = [], 0.0
        for i, j in zip(py.tolist(), px.tolist()):
            X = t["xys"][gid].clone().requires_grad_(True)
            img, Tfin, _, E = rt.composite_tile(X, t["conics"][gid], t["colors"][gid], t["opac"][gid], torch.arange(len(gid)), s, i, i + 1, j, j + 1,
                                                extra=t["extra"][gid])
            alpha = 1 - Tfin[0]
            L = ((img[0] + Tfin[0] * t["background"]) * v["v_out"][i, j]).sum() + alpha * v["v_alpha"][i, j]
            if float(alpha.detach()) > 0:
                L = L + E[0] / alpha * v["v_depth"][i, j]
            leaves.append(X)
            total = total + L
        g = torch.stack(torch.autograd.grad(total, leaves))
        np.add.at(want, gid.numpy(), g.abs().sum(0).numpy())
    ref = cs.pair_backward(sc, cot, F64, True)
    within("tiny: xy_abs vs per-pixel autograd", cs.row_errors(ref["xy_abs"], want, ref["v_xy"][1])[0], 1e-12)


@pytest.mark.parametrize("name", cs.SCENES)
def test_c_oracle_per_row(name, oracle_c):
    sc = cs.scene(name)
    f64 = cs.forward(sc, F64)
    img, E, fT, fi = oracle_c.rasterize_fwd(sc["xys"], sc["conics"], sc["colors"], sc["opac"], sc["ids_sorted"], sc["tile_bins"], sc["H"], sc["W"],
                                            _tb(sc), sc["background"], extra=sc["extra"])
    assert np.array_equal(fi, f64["final_index"])
    for k, v in cs.forward_errors(dict(image=img, extra=E, final_Ts=fT), f64).items():
        within(f"{name}: C oracle forward {k}", v, cs.FWD_BARS[k])
    for cset in "abc":
        cot = cs.cotangents(sc, cset)
        got = oracle_c.rasterize_bwd(sc["xys"], sc["conics"], sc["colors"], sc["opac"], sc["ids_sorted"], sc["tile_bins"], sc["H"], sc["W"], _tb(sc),
                                     sc["background"], fT, fi, cot["v_out"], cot["v_alpha"])
        ref = cs.reference(sc, cset)
        for k, g in zip(cs.KEYS, got):
            within(f"{name} {cset}: C oracle {k}", cs.row_errors(g, ref[k][0], ref[k][1])[0], cs.BARS[k])


def test_bar_window():
    d, fd = cs.reference_distances(), cs.forward_distances()
    print("backward float32-vs-float64 distances:", {k: f"{v:.3g}" for k, v in d.items()})
    print("forward  float32-vs-float64 distances:", {k: f"{v:.3g}" for k, v in fd.items()})
    for k in cs.KEYS:
        assert 2 * d[k] <= cs.BARS[k] <= 8 * d[k], (k, d[k], cs.BARS[k])
    assert cs.BARS["v_extra"] == cs.BARS["v_colors"] and cs.BARS["xy_abs"] == cs.BARS["v_xy"]
    assert d["xy_abs"] <= cs.BARS["xy_abs"] / 2 and d["v_extra"] <= cs.BARS["v_extra"] / 2
    for k in cs.FWD_BARS:
        assert 2 * fd[k] <= cs.FWD_BARS[k] <= 8 * fd[k], (k, fd[k], cs.FWD_BARS[k])


def _old_bar_rows(got, ref):
    """rows test_raster_gpu._grad_close would flag: |diff| > 1e-3 max|ref of the tensor| + 1e-6 max|ref of all four|"""
    scale = max(np.abs(ref[k][0]).max() for k in cs.KEYS)
    n = 0
    for k in cs.KEYS:
        d = np.abs(got[k][0] - ref[k][0]).reshape(ref[k][0].shape[0], -1).max(1)
        n += int((d > 1e-3 * np.abs(ref[k][0]).max() + 1e-6 * scale).sum())
    return n


def test_sensitivity():
    """each fault, injected into the float64 closed form, moves rows beyond the new bars; the whole-tensor bar sees none of faults (i), (iv)"""
    table = {}
    # fault (i) is one block of one tile, taken in `stop`, whose rows span five orders of magnitude.  (In `deep` every row is within two
    # orders of the largest one -- v_opacity does not even scale with the opacity -- and the whole-tensor bar sees such a loss as well.)
    edge_scene = "stop"
    print("fault (i):", edge_scene, cs.batch_edge_target(cs.scene(edge_scene)))
    for fault in cs.FAULTS:
        new = old = 0
        for name in cs.SCENES:
            sc = cs.scene(name)
            if fault == "batch_edge" and name != edge_scene:
                continue
            for cset in "abc":
                ref = cs.reference(sc, cset)
                bad = cs.pair_backward(sc, cs.cotangents(sc, cset), F64, fault=fault)
                for k in cs.KEYS:
                    d = np.linalg.norm(cs._rows(bad[k][0]) - cs._rows(ref[k][0]), axis=1)
                    den = np.linalg.norm(cs._rows(ref[k][1]), axis=1)
                    new += int((d[den > 0] > cs.BARS[k] * den[den > 0]).sum())
                old += _old_bar_rows(bad, ref)
        table[fault] = (new, old)
    print("fault: rows beyond the new bars / rows the whole-tensor bar flags (all scenes, sets a b c):")
    for fault, (new, old) in table.items():
        print(f"  {fault:11s} {new:6d} {old:6d}")
    for fault, (new, old) in table.items():
        assert new > 0, fault
    assert table["batch_edge"][1] == 0 and table["t_drift"][1] == 0

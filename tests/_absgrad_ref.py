"""float64 reference of absgrad densification (RenderAux.absgrad / gc_rasterize_bwd_abs_views), built from the oracle's own composite_tile on
1 x 1 pixel blocks.  A helper, not a test module.

With the oracle's projected centres detached as a leaf X, every pixel p has its own loss

    L_p = sum_c min(rgb_p, 1)_c v_rgb[p, c] + alpha_p v_a[p] + [alpha_p > 0] (E_p / alpha_p) v_d[p]

composited over that pixel's tile list (get_outputs(...)["tile_bins"], extra = the projected depths), and g_p = dL_p/dX by autograd.  Then

    abs_ref = sum_p |g_p|          signed = sum_p g_p

both for the three-term L_p ("abs", "signed") and for L_p without its depth term ("abs_nodepth", "signed_nodepth": the render whose depth image
carries no gradient), from one pass over the pixels.

`signed` is the oracle's full-image xys gradient (tests/test_absgrad_cpu.py holds that to 1e-12), `abs_ref` is gsplat's absgrad: rgb, alpha
and depth of ONE pixel combine before the absolute value, different pixels do not.

Autograd runs once per tile, not once per pixel: every pixel composites from a private copy of the tile's centres (a leaf of its own), so the
gradient of sum_p L_p with respect to pixel p's copy is exactly g_p."""
import numpy as np
import torch

TILE = 16


def absgrad_reference(P, c2w, K, background, cotangents, dtype=torch.float64):
    """P: the six parameter arrays; c2w [3,4]; K: dict(fx, fy, cx, cy, W, H); cotangents (v_rgb [H,W,3], v_a [H,W], v_d [H,W]).
    Returns dict(abs, signed, abs_nodepth, signed_nodepth: [N,2]; radii [N]) as numpy arrays (float64 for dtype = float64)."""
    from oracle import raster_torch as rt
    H, W = K["H"], K["W"]
    p = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in P.items()}
    c2w = torch.tensor(np.asarray(c2w))
    bg = torch.tensor(np.asarray(background), dtype=dtype)
    with torch.no_grad():
        o = rt.get_outputs(p, c2w, K["fx"], K["fy"], K["cx"], K["cy"], W, H, bg, training=False, dtype=dtype)
        # the per-Gaussian inputs of the compositing, as get_outputs forms them
        viewmat, _, full = rt.camera_to_gsplat(c2w, K["fx"], K["fy"], W, H, dtype)
        tb = ((W + TILE - 1) // TILE, (H + TILE - 1) // TILE, 1)
        quats = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
        xys, depths, radii, conics, _, _ = rt.project_gaussians(p["means"], torch.exp(p["scales"]), 1.0, quats, viewmat[:3, :], full, K["fx"],
                                                                K["fy"], K["cx"], K["cy"], H, W, tb)
        assert torch.equal(xys, o["xys"]) and torch.equal(radii, o["radii"])
        viewdirs = p["means"] - c2w[:3, 3].to(dtype)
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        colors = torch.cat([p["features_dc"][:, None, :], p["features_rest"]], 1)
        rgbs = torch.clamp(rt.spherical_harmonics(3, viewdirs, colors) + 0.5, min=0.0)
        opac = torch.sigmoid(p["opacities"])[:, 0]
    ids, bins = o["gaussian_ids_sorted"], o["tile_bins"]
    v_rgb, v_a, v_d = (torch.tensor(np.asarray(c), dtype=dtype) for c in cotangents)
    N = xys.shape[0]
    out = {k: torch.zeros(N, 2, dtype=dtype) for k in ("abs", "signed", "abs_nodepth", "signed_nodepth")}
    for ty in range(tb[1]):
        for tx in range(tb[0]):
            s, e = int(bins[ty * tb[0] + tx, 0]), int(bins[ty * tb[0] + tx, 1])
            if e <= s:
                continue
            gid = ids[s:e].to(torch.int64)
            n = gid.numel()
            loc = torch.arange(n)
            cn, col, op, ex = conics[gid], rgbs[gid], opac[gid], depths[gid]
            leaves, total, total_nodepth = [], 0.0, 0.0
            for i in range(ty * TILE, min(ty * TILE + TILE, H)):
                for j in range(tx * TILE, min(tx * TILE + TILE, W)):
                    X = xys[gid].clone().requires_grad_(True)           # this pixel's own copy of the centres
                    img, Tfin, _, E = rt.composite_tile(X, cn, col, op, loc, s, i, i + 1, j, j + 1, extra=ex)
                    rgb = torch.clamp(img[0] + Tfin[0] * bg, max=1.0)
                    alpha = 1 - Tfin[0]
                    L = (rgb * v_rgb[i, j]).sum() + alpha * v_a[i, j]
                    leaves.append(X)
                    total_nodepth = total_nodepth + L
                    if float(alpha.detach()) > 0:
                        L = L + E[0] / alpha * v_d[i, j]
                    total = total + L
            for sfx, loss in (("", total), ("_nodepth", total_nodepth)):
                g = torch.stack(torch.autograd.grad(loss, leaves, retain_graph=True))       # [pixels, n, 2]
                out["abs" + sfx].index_add_(0, gid, g.abs().sum(0))
                out["signed" + sfx].index_add_(0, gid, g.sum(0))
    res = {k: v.numpy() for k, v in out.items()}
    res["radii"] = radii.numpy()
    return res

"""GPU tests of rasterize_gaussians for colors[N, C] with C != 3 (gsplat's nd_rasterize_forward / _backward; HIP kernels of
gaussctrl_amd/csrc/raster_composite_nd.hip): forward and backward against the fp64 oracle (oracle/raster_torch.py::rasterize, fed the
same tile lists), the N-channel op against the 3-channel one on channel triples at full size, RGB + depth in one call against the
reference's two calls, and the edge cases of the operator surface and the C ABI."""
import numpy as np
import pytest
import torch

from _margins import within
from test_raster_gpu import BG, DEV, _grad_close, _img_close, _scene, _t

pytestmark = pytest.mark.gpu


def _projected(N, W, H, fx, sm, seed=3):
    """the scene of tests/test_raster_gpu.py projected by the product: (xys, depths, radii, conics, num_tiles_hit, opacity[N,1])"""
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.camera import camera_to_gsplat
    P, c2w, K = _scene(N, W, H, fx, seed=seed, scale_mean=sm)
    cam = camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], W, H)
    q = P["quats"] / np.linalg.norm(P["quats"], axis=-1, keepdims=True)
    V4 = _t(cam["viewmat4"]); full = _t(np.asarray(cam["fullproj"], np.float32).reshape(4, 4))
    with torch.no_grad():
        xys, depths, radii, conics, nth, _ = ops.project_gaussians(_t(P["means"]), torch.exp(_t(P["scales"])), 1, _t(q), V4[:3], full,
                                                                   K["fx"], K["fy"], K["cx"], K["cy"], H, W, cam["tile_bounds"])
        opac = torch.sigmoid(_t(P["opacities"]))
    return xys, depths, radii, conics, nth, opac


def _lists(xys, depths, radii, nth, W, H):
    from gaussctrl_amd import gsplat_ops as ops
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    _, _, ids, bins, _ = ops.bin_and_sort_gaussians(xys.shape[0], xys, depths, radii, nth, tb)
    return tb, ids, bins


def _colors(N, C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(N, C, device=DEV, generator=g) * 1.5 - 0.25        # some negative, some above 1: nothing is clamped


def _oracle(xys, conics, colors, opac, ids, bins, H, W, tb, bg):
    from oracle import raster_torch as rt
    with torch.device(DEV):
        return rt.rasterize(xys.double(), conics.double(), colors.double(), opac.reshape(-1).double(), ids, bins.cpu(), H, W, tb, bg.double())


SMALL = [(5000, 200, 136, 180.0, 0.03), (3, 40, 24, 50.0, 0.2)]
BIG = (100000, 512, 512, 540.0, 0.01)


@pytest.mark.parametrize("scene,C", [(s, c) for s in SMALL for c in (1, 2, 4, 5, 8, 16, 31, 32, 33, 64, 100)] + [(BIG, 4), (BIG, 33)])
def test_forward_vs_fp64_oracle(scene, C):
    from gaussctrl_amd import gsplat_ops as ops
    N, W, H, fx, sm = scene
    xys, depths, radii, conics, nth, opac = _projected(N, W, H, fx, sm)
    tb, ids, bins = _lists(xys, depths, radii, nth, W, H)
    colors = _colors(N, C, seed=C)
    bg = torch.linspace(0.1, 0.9, C, device=DEV)
    img, alpha = ops.rasterize_gaussians(xys, depths, radii, conics, nth, colors, opac, H, W, background=bg, return_alpha=True)
    assert img.shape == (H, W, C) and alpha.shape == (H, W)
    ref_img, ref_alpha, ref_idx, _ = _oracle(xys, conics, colors, opac, ids, bins, H, W, tb, bg)
    _img_close(img.cpu().numpy(), ref_img.cpu().numpy())
    _img_close(alpha.cpu().numpy(), ref_alpha.cpu().numpy())
    # final_Ts / final_index: bit-identical to the 3-channel kernel's on the same lists
    out_nd, fT_nd, fi_nd = ops._rasterize_nd_fwd(H, W, tb, ids, bins, xys, conics, colors.contiguous(), opac.reshape(-1), bg)
    col3 = torch.zeros(N, 3, device=DEV); col3[:, :min(3, C)] = colors[:, :3]
    _, _, fT3, fi3 = ops._rasterize_fwd(H, W, tb, ids, bins, xys, conics, col3, opac.reshape(-1).contiguous(), None, torch.ones(3, device=DEV))
    assert torch.equal(fT_nd, fT3) and torch.equal(fi_nd, fi3)
    assert torch.equal(alpha, 1 - fT3)
    assert torch.equal(out_nd, img)


@pytest.mark.parametrize("scene,C", [(s, c) for s in SMALL for c in (1, 4, 8, 33)])
def test_backward_vs_fp64_autograd(scene, C):
    from gaussctrl_amd import gsplat_ops as ops
    N, W, H, fx, sm = scene
    xys, depths, radii, conics, nth, opac = _projected(N, W, H, fx, sm)
    tb, ids, bins = _lists(xys, depths, radii, nth, W, H)
    colors = _colors(N, C, seed=100 + C)
    bg = torch.linspace(0.9, 0.1, C, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(7 + C)
    v_out = torch.randn(H, W, C, device=DEV, generator=g); v_alpha = torch.randn(H, W, device=DEV, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (xys, conics, colors, opac)]
    img, alpha = ops.rasterize_gaussians(leaves[0], depths, radii, leaves[1], nth, leaves[2], leaves[3], H, W, background=bg,
                                         return_alpha=True)
    ((img * v_out).sum() + (alpha * v_alpha).sum()).backward()
    ref = [t.detach().double().requires_grad_(True) for t in (xys, conics, colors, opac)]
    from oracle import raster_torch as rt
    with torch.device(DEV):
        r_img, r_alpha, _, _ = rt.rasterize(ref[0], ref[1], ref[2], ref[3].reshape(-1), ids, bins.cpu(), H, W, tb, bg.double())
        ((r_img * v_out.double()).sum() + (r_alpha * v_alpha.double()).sum()).backward()
    scale = max(float(r.grad.abs().max()) for r in ref)
    for name, got, r in zip(("xys", "conics", "colors", "opacity"), leaves, ref):
        assert got.grad.shape == r.grad.shape, name
        _grad_close(got.grad.cpu().numpy(), r.grad.cpu().numpy(), scale)


_FULL = {}


def _full_inputs():
    """1 M Gaussians at 512 x 512 (the synthetic scene of tests/test_raster_gpu.py), projected and binned once for the module"""
    if not _FULL:
        W = H = 512
        xys, depths, radii, conics, nth, opac = _projected(1_000_000, W, H, 540.0, 0.01)
        tb, ids, bins = _lists(xys, depths, radii, nth, W, H)
        _FULL.update(xys=xys, conics=conics, opac=opac.reshape(-1).contiguous(), tb=tb, ids=ids, bins=bins, W=W, H=H)
    return _FULL


@pytest.mark.parametrize("C", [7, 32])
def test_full_size_matches_channel_triples(C):
    """The N-channel op against what a caller would otherwise write: the 3-channel op once per channel triple."""
    from gaussctrl_amd import gsplat_ops as ops
    f = _full_inputs()
    H, W, tb, ids, bins, xys, conics, opac = f["H"], f["W"], f["tb"], f["ids"], f["bins"], f["xys"], f["conics"], f["opac"]
    N = xys.shape[0]
    colors = _colors(N, C, seed=200 + C)
    bg = torch.linspace(0.2, 0.7, C, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(300 + C)
    v_out = torch.randn(H, W, C, device=DEV, generator=g); v_alpha = torch.randn(H, W, device=DEV, generator=g)
    img, fT, fi = ops._rasterize_nd_fwd(H, W, tb, ids, bins, xys, conics, colors, opac, bg)
    v_xy, v_conic, v_col, v_op = ops._rasterize_nd_bwd(H, W, tb, N, ids, bins, xys, conics, colors, opac, bg, fT, fi, v_out.contiguous(),
                                                      v_alpha)
    P = -(-C // 3) * 3                                                  # channels padded to whole triples
    pad = lambda t: torch.nn.functional.pad(t, (0, P - C)).contiguous()
    colp, bgp, vop = pad(colors), pad(bg), pad(v_out)
    s_xy, s_conic, s_op = torch.zeros_like(v_xy), torch.zeros_like(v_conic), torch.zeros_like(v_op)
    s_col = torch.zeros(N, P, device=DEV)
    for k in range(0, P, 3):
        img3, _, fT3, fi3 = ops._rasterize_fwd(H, W, tb, ids, bins, xys, conics, colp[:, k:k + 3].contiguous(), opac, None,
                                               bgp[k:k + 3].contiguous())
        assert torch.equal(fT3, fT) and torch.equal(fi3, fi)
        ref = img3[..., :min(3, C - k)]
        within(f"C={C} channels {k}..: max |nd - triple| / max", float((img[..., k:k + ref.shape[-1]] - ref).abs().max()),
               1e-6 * float(ref.abs().max()))
        g_xy, g_conic, g_col, g_op = ops._rasterize_bwd(H, W, tb, N, ids, bins, xys, conics, colp[:, k:k + 3].contiguous(), opac,
                                                        bgp[k:k + 3].contiguous(), fT3, fi3, vop[..., k:k + 3].contiguous(),
                                                        v_alpha if k == 0 else None)
        s_xy += g_xy; s_conic += g_conic; s_op += g_op; s_col[:, k:k + 3] = g_col
    scale = max(float(t.abs().max()) for t in (s_xy, s_conic, s_op, s_col))
    for got, ref in ((v_xy, s_xy), (v_conic, s_conic), (v_op, s_op), (v_col, s_col[:, :C])):
        _grad_close(got.cpu().numpy(), ref.cpu().numpy(), scale)


def test_rgb_and_depth_in_one_call():
    """project -> SH -> rasterize with colors = [rgb | depth] (C = 4) against the reference's two calls, RGB then depth repeated into
    three channels (gaussctrl/gc_model.py:174-202), both through the gsplat surface."""
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.camera import camera_to_gsplat
    N, W, H, fx = 5000, 200, 136, 180.0
    P, c2w, K = _scene(N, W, H, fx)
    cam = camera_to_gsplat(c2w, K["fx"], K["fy"], K["cx"], K["cy"], W, H)
    V4 = _t(cam["viewmat4"]); full = _t(np.asarray(cam["fullproj"], np.float32).reshape(4, 4))
    rng = np.random.default_rng(11)
    v_rgb, v_d, v_a = (_t(rng.normal(size=s).astype(np.float32)) for s in ((H, W, 3), (H, W), (H, W)))

    def run(one_call):
        tp = {k: _t(v).requires_grad_(True) for k, v in P.items()}
        colors = torch.cat([tp["features_dc"][:, None, :], tp["features_rest"]], 1)
        q = tp["quats"] / tp["quats"].norm(dim=-1, keepdim=True)
        xys, depths, radii, conics, nth, _ = ops.project_gaussians(tp["means"], torch.exp(tp["scales"]), 1, q, V4[:3], full,
                                                                   K["fx"], K["fy"], K["cx"], K["cy"], H, W, cam["tile_bounds"])
        vd = tp["means"].detach() - _t(c2w[:3, 3]); vd = vd / vd.norm(dim=-1, keepdim=True)
        rgbs = torch.clamp(ops.spherical_harmonics(3, vd, colors) + 0.5, min=0.0)
        op = torch.sigmoid(tp["opacities"])
        if one_call:
            out, alpha = ops.rasterize_gaussians(xys, depths, radii, conics, nth, torch.cat([rgbs, depths[:, None]], 1), op, H, W,
                                                 background=torch.cat([_t(BG), torch.zeros(1, device=DEV)]), return_alpha=True)
            rgb, dep = out[..., :3], out[..., 3]
        else:
            rgb, alpha = ops.rasterize_gaussians(xys, depths, radii, conics, nth, rgbs, op, H, W, background=_t(BG), return_alpha=True)
            dep = ops.rasterize_gaussians(xys, depths, radii, conics, nth, depths[:, None].repeat(1, 3), op, H, W,
                                          background=torch.zeros(3, device=DEV))[..., 0]
        ((rgb * v_rgb).sum() + (dep * v_d).sum() + (alpha * v_a).sum()).backward()
        return rgb.detach(), dep.detach(), alpha.detach(), {k: t.grad for k, t in tp.items()}

    rgb1, dep1, a1, g1 = run(True)
    rgb2, dep2, a2, g2 = run(False)
    _img_close(rgb1.cpu().numpy(), rgb2.cpu().numpy())
    _img_close(dep1.cpu().numpy(), dep2.cpu().numpy())
    assert torch.equal(a1, a2)
    scale = max(float(g.abs().max()) for g in g2.values())
    for k in P:
        _grad_close(g1[k].cpu().numpy(), g2[k].cpu().numpy(), scale)


# ---------------------------------------------------------------------------------------------------------------- edge cases
def test_nothing_visible_gives_background_and_zero_gradients():
    from gaussctrl_amd import gsplat_ops as ops
    N, W, H, C = 50, 40, 24, 5
    xys, depths, radii, conics, nth, opac = _projected(N, W, H, 50.0, 0.2)
    for culled in (torch.zeros_like(radii), None):                     # nothing binned / binned but every alpha below 1/255
        r = culled if culled is not None else radii
        n = torch.zeros_like(nth) if culled is not None else nth
        o = opac if culled is not None else torch.full_like(opac, 1e-4)
        x, cn, col, o = (t.clone().requires_grad_(True) for t in (xys, conics, _colors(N, C, 1), o))
        bg = torch.arange(C, device=DEV, dtype=torch.float32) / C
        img, alpha = ops.rasterize_gaussians(x, depths, r, cn, n, col, o, H, W, background=bg, return_alpha=True)
        assert torch.equal(img, bg.expand(H, W, C)) and float(alpha.abs().max()) == 0.0
        (img.sum() + alpha.sum()).backward()
        for t in (x, cn, col, o):
            assert float(t.grad.abs().max()) == 0.0


def test_background_default_length_and_dtype():
    from gaussctrl_amd import gsplat_ops as ops
    N, W, H, fx, sm = SMALL[0]
    xys, depths, radii, conics, nth, opac = _projected(N, W, H, fx, sm)
    args = (xys, depths, radii, conics, nth)
    for C in (1, 6):
        col = _colors(N, C, 5)
        a = ops.rasterize_gaussians(*args, col, opac, H, W)
        b = ops.rasterize_gaussians(*args, col, opac, H, W, background=torch.ones(C, device=DEV))
        assert torch.equal(a, b)
        with pytest.raises(ValueError):
            ops.rasterize_gaussians(*args, col, opac, H, W, background=torch.ones(C + 1, device=DEV))
        # uint8 colours are divided by 255
        c8 = (torch.rand(N, C, device=DEV) * 255).to(torch.uint8)
        assert torch.equal(ops.rasterize_gaussians(*args, c8, opac, H, W), ops.rasterize_gaussians(*args, c8.float() / 255, opac, H, W))
        # non-contiguous colours
        wide = _colors(N, 2 * C, 6)
        nc = wide[:, ::2]
        assert not nc.is_contiguous()
        assert torch.equal(ops.rasterize_gaussians(*args, nc, opac, H, W), ops.rasterize_gaussians(*args, nc.contiguous(), opac, H, W))


@pytest.mark.parametrize("W,H", [(37, 29), (200, 136), (17, 100)])
def test_image_size_not_a_multiple_of_16(W, H):
    from gaussctrl_amd import gsplat_ops as ops
    N, C = 2000, 6
    xys, depths, radii, conics, nth, opac = _projected(N, W, H, 0.9 * max(W, H), 0.05)
    tb, ids, bins = _lists(xys, depths, radii, nth, W, H)
    colors = _colors(N, C, 9)
    bg = torch.linspace(0.3, 0.6, C, device=DEV)
    img, alpha = ops.rasterize_gaussians(xys, depths, radii, conics, nth, colors, opac, H, W, background=bg, return_alpha=True)
    ref_img, ref_alpha, _, _ = _oracle(xys, conics, colors, opac, ids, bins, H, W, tb, bg)
    _img_close(img.cpu().numpy(), ref_img.cpu().numpy())
    _img_close(alpha.cpu().numpy(), ref_alpha.cpu().numpy())


def test_abi_refuses_bad_channel_counts_and_sizes():
    """argument checks run before any launch: small dummy buffers are never touched"""
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    d = torch.zeros(64, device=DEV)
    p = L.ptr(d)

    def fwd(H, W, C):
        return lib.gc_rasterize_nd_fwd(L.i32(H), L.i32(W), L.i32((W + 15) // 16), L.i32((H + 15) // 16), L.i32(C), p, p, p, p, p, p, p, p,
                                       p, p, L.stream_ptr())

    def bwd(H, W, N, C):
        return lib.gc_rasterize_nd_bwd(L.i32(H), L.i32(W), L.i32((W + 15) // 16), L.i32((H + 15) // 16), L.i64(N), L.i32(C), p, p, p, p, p,
                                       p, p, p, p, p, p, p, p, p, p, L.stream_ptr())

    EINVAL = -1
    assert fwd(16, 16, 0) == EINVAL and bwd(16, 16, 4, 0) == EINVAL
    assert fwd(16, 16, -3) == EINVAL
    assert fwd(16384, 16384, 8) == EINVAL and bwd(16384, 16384, 4, 8) == EINVAL          # H W C = 2^31
    assert bwd(16, 16, 1 << 28, 8) == EINVAL                                            # N C = 2^31
    assert b"channels" in lib.gc_last_error_string()
    torch.cuda.synchronize()

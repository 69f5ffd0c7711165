"""Operator surface of the rasterizer: drop-in for the three gsplat 0.1.3 functions the reference calls.

    project_gaussians    /root/reference/gaussctrl/gc_model.py:140-154  (import :35)
    spherical_harmonics  /root/reference/gaussctrl/gc_model.py:166      (import :32)
    rasterize_gaussians  /root/reference/gaussctrl/gc_model.py:174-186,191-202 (import :36)

Same names, argument order, tuple arity (6-tuple from project_gaussians, gsplat <= 0.1.3) and
autograd behaviour; every call goes through the C ABI of include/gaussctrl_hip.h (hand-written HIP
kernels for gfx950).  There is no CPU / eager fallback: tensors must live on the GPU.

`render_view` is the fused product path used by gaussctrl_amd.gc_model.GaussCtrlModel.get_outputs:
one launch over the 59-float parameter record (exp/normalise/project/SH/sigmoid), one sort, one
compositing sweep for RGB + depth + alpha, and a fused backward to the six leaf tensors.
"""
from __future__ import annotations

import collections

import torch

from . import _lib as L

TILE = 16


def num_sh_bases(degree: int) -> int:
    """gsplat.sh.num_sh_bases"""
    if degree == 0:
        return 1
    if degree == 1:
        return 4
    if degree == 2:
        return 9
    if degree == 3:
        return 16
    return 25


_need_gpu = L.need_gpu


def _c(t, dtype=torch.float32):
    return t.detach().to(dtype).contiguous()


def _host_mat(m, n):
    """small camera matrix (device or host tensor / array) -> ctypes float array of n entries."""
    if isinstance(m, torch.Tensor):
        m = m.detach().to("cpu", torch.float32).reshape(-1)
    else:
        import numpy as np
        m = torch.from_numpy(np.asarray(m, dtype="float32").reshape(-1))
    if m.numel() < n:
        raise ValueError(f"camera matrix needs >= {n} entries")
    return L.host_floats(m[:n].tolist())


# --------------------------------------------------------------------------------------------- project
class _ProjectGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, H, W, tile_bounds, clip):
        _need_gpu(means3d, scales, quats)
        N = means3d.shape[0]
        dev = means3d.device
        m, s, q = _c(means3d), _c(scales), _c(quats)
        V, P = _host_mat(viewmat, 12), _host_mat(projmat, 16)
        cov3d = torch.empty(N, 6, device=dev); xys = torch.empty(N, 2, device=dev); depths = torch.empty(N, device=dev)
        radii = torch.empty(N, dtype=torch.int32, device=dev); conics = torch.empty(N, 3, device=dev)
        nth = torch.empty(N, dtype=torch.int32, device=dev)
        L.call("gc_project_gaussians_fwd", N, m, s, glob_scale, q, V, P, fx, fy, cx, cy, H, W, tile_bounds[0], tile_bounds[1], clip,
               cov3d, xys, depths, radii, conics, nth)
        ctx.save_for_backward(m, s, q, radii, conics)
        ctx.cam = (V, P, float(glob_scale), float(fx), float(fy), float(cx), float(cy), int(H), int(W))
        ctx.mark_non_differentiable(radii, nth)
        return xys, depths, radii, conics, nth, cov3d

    @staticmethod
    def backward(ctx, v_xys, v_depths, v_radii, v_conics, v_nth, v_cov3d):
        m, s, q, radii, conics = ctx.saved_tensors
        V, P, glob, fx, fy, cx, cy, H, W = ctx.cam
        N = m.shape[0]
        dev = m.device
        v_xy = _c(v_xys) if v_xys is not None else torch.zeros(N, 2, device=dev)
        v_con = _c(v_conics) if v_conics is not None else torch.zeros(N, 3, device=dev)
        v_dep = _c(v_depths) if v_depths is not None else None
        vm = torch.empty(N, 3, device=dev); vs = torch.empty(N, 3, device=dev); vq = torch.empty(N, 4, device=dev)
        L.call("gc_project_gaussians_bwd", N, m, s, glob, q, V, P, fx, fy, cx, cy, H, W, radii, conics, v_xy, v_dep, v_con, vm, vs, vq)
        return (vm, vs, None, vq) + (None,) * 10


def project_gaussians(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
                      tile_bounds, clip_thresh=0.01):
    """gsplat 0.1.3 signature; returns (xys, depths, radii, conics, num_tiles_hit, cov3d)."""
    return _ProjectGaussians.apply(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
                                   img_height, img_width, tile_bounds, clip_thresh)


# --------------------------------------------------------------------------------------------- SH
class _SphericalHarmonics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degrees_to_use, viewdirs, coeffs):
        _need_gpu(viewdirs, coeffs)
        N, K = coeffs.shape[0], coeffs.shape[1]
        degree = {1: 0, 4: 1, 9: 2, 16: 3}[K]
        d, c = _c(viewdirs), _c(coeffs)
        out = torch.empty(N, 3, device=coeffs.device)
        L.call("gc_sh_fwd", N, degree, degrees_to_use, d, c, out)
        ctx.save_for_backward(d)
        ctx.meta = (degree, int(degrees_to_use), K)
        return out

    @staticmethod
    def backward(ctx, v_colors):
        (d,) = ctx.saved_tensors
        degree, n, K = ctx.meta
        N = d.shape[0]
        vc = _c(v_colors)
        out = torch.empty(N, K, 3, device=d.device)
        L.call("gc_sh_bwd", N, degree, n, d, vc, out)
        return None, None, out


def spherical_harmonics(degrees_to_use, viewdirs, coeffs):
    """gsplat.sh.spherical_harmonics(degrees_to_use, viewdirs[N,3], coeffs[N,K,3]) -> colors[N,3]"""
    return _SphericalHarmonics.apply(degrees_to_use, viewdirs, coeffs)


# --------------------------------------------------------------------------------------------- binning
def bin_and_sort_gaussians(N, xys, depths, radii, num_tiles_hit, tile_bounds, want_keys=False, m_cap=None, tile_boxes=None):
    """Two-level binning (csrc/raster_sort.hip): depth-sort the Gaussians, emit (tile, id) in depth order, stable radix
    passes over the tile id, tile bins.  Same gaussian_ids_sorted / tile_bins as gsplat's bin_and_sort_gaussians
    (reference call sites gc_model.py:174-202).  Returns (M, isect_ids_sorted | None, gaussian_ids_sorted, tile_bins,
    cum_tiles_hit_in_depth_order).  One 4-byte readback (M).
    tile_boxes: the packed tight boxes of gc_project_sh_fwd_boxes (num_tiles_hit must be the counts it wrote): the emission walks
    them instead of the boxes recomputed from xys / radii -- fewer pairs, bit-identical images (fused product path)."""
    dev = xys.device
    T = tile_bounds[0] * tile_bounds[1]
    order = torch.empty(N, dtype=torch.int32, device=dev)
    cum = torch.empty(N, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    wb = L.call("gc_raster_depth_order_workspace_bytes", N)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    L.call("gc_raster_depth_order", N, depths, radii, num_tiles_hit, order, cum, cnt, ws, wb)
    bins = torch.empty(T, 2, dtype=torch.int32, device=dev)
    if m_cap is not None:
        # sync-free: buffers sized for the caller's capacity, count and overflow flag stay on the device.
        # Returns M = (count tensor, overflow tensor) instead of a host int.
        M = int(m_cap)
        ovf = torch.empty(1, dtype=torch.int32, device=dev)
        dev_cnt = ret_M = (cnt, ovf)
    else:
        M = _read_count(cnt)
        dev_cnt, ret_M = (None, None), M
    ids_s = torch.empty(M, dtype=torch.int32, device=dev)
    keys_s = torch.empty(M, dtype=torch.int64, device=dev) if want_keys else None
    bb = L.call("gc_raster_bin_workspace_bytes", M)
    bws = torch.empty(bb, dtype=torch.uint8, device=dev)
    lead, out = (N, M), (tile_bounds[0], tile_bounds[1], ids_s, bins, keys_s, bws, bb)
    if tile_boxes is not None:
        L.call("gc_raster_bin_tiles_boxes", *lead, *dev_cnt, order, cum, tile_boxes, depths, *out)
    elif m_cap is not None:
        L.call("gc_raster_bin_tiles_dev", *lead, *dev_cnt, order, cum, xys, depths, radii, *out)
    else:
        L.call("gc_raster_bin_tiles", *lead, order, cum, xys, depths, radii, *out)
    return ret_M, keys_s, ids_s, bins, cum


def _read_count(cnt):
    """the one blocking 4-byte read-back (gc_raster_read_count) of a device counter, as a host int"""
    m_host = L.C.c_int32(0)
    L.call("gc_raster_read_count", cnt, L.C.byref(m_host))
    return int(m_host.value)


def bin_and_sort_gaussians_keys64(N, xys, depths, radii, num_tiles_hit, tile_bounds):
    """gsplat-shaped chain: cumsum -> map -> 64-bit key sort -> tile bins (kept for API parity / cross-checks).
    Returns (M, isect_ids_sorted, gaussian_ids_sorted, tile_bins, cum_tiles_hit)."""
    dev = xys.device
    T = tile_bounds[0] * tile_bounds[1]
    cum = torch.empty(N, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = L.call("gc_raster_scan_workspace_bytes", N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    L.call("gc_raster_scan_tiles", N, num_tiles_hit, cum, cnt, ws, ws_bytes)
    M = _read_count(cnt)
    bins = torch.empty(T, 2, dtype=torch.int32, device=dev)
    keys = torch.empty(M, dtype=torch.int64, device=dev); ids = torch.empty(M, dtype=torch.int32, device=dev)
    keys_s = torch.empty(M, dtype=torch.int64, device=dev); ids_s = torch.empty(M, dtype=torch.int32, device=dev)
    if M > 0:
        L.call("gc_raster_map_intersects", N, M, xys, depths, radii, cum, tile_bounds[0], tile_bounds[1], keys, ids)
        sb = L.call("gc_raster_sort_workspace_bytes", M, T)
        sws = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
        L.call("gc_raster_sort_intersects", M, T, keys, ids, keys_s, ids_s, sws, sb)
    L.call("gc_raster_tile_bins", M, T, keys_s, bins)
    return M, keys_s, ids_s, bins, cum


def _rasterize_fwd(H, W, tb, ids_s, bins, xys, conics, colors, opac, extra, background):
    dev = xys.device
    out = torch.empty(H, W, 3, device=dev)
    out_e = torch.empty(H, W, device=dev) if extra is not None else None
    fT = torch.empty(H, W, device=dev)
    fi = torch.empty(H, W, dtype=torch.int32, device=dev)
    L.call("gc_rasterize_fwd", H, W, tb[0], tb[1], ids_s, bins, xys, conics, colors, opac, extra, background, out, out_e, fT, fi)
    return out, out_e, fT, fi


def _rasterize_bwd(H, W, tb, N, ids_s, bins, xys, conics, colors, opac, background, fT, fi, v_out, v_alpha):
    dev = xys.device
    v_xy = torch.zeros(N, 2, device=dev); v_conic = torch.zeros(N, 3, device=dev)
    v_col = torch.zeros(N, 3, device=dev); v_op = torch.zeros(N, device=dev)
    L.call("gc_rasterize_bwd", H, W, tb[0], tb[1], N, ids_s, bins, xys, conics, colors, opac, background, fT, fi, v_out, v_alpha,
           v_xy, v_conic, v_col, v_op)
    return v_xy, v_conic, v_col, v_op


def _rasterize_nd_fwd(H, W, tb, ids_s, bins, xys, conics, colors, opac, background):
    """colors[N,C] for any C (gc_rasterize_nd_fwd) -> out_img[H,W,C], final_Ts, final_index"""
    dev = xys.device
    C = colors.shape[1]
    out = torch.empty(H, W, C, device=dev)
    fT = torch.empty(H, W, device=dev)
    fi = torch.empty(H, W, dtype=torch.int32, device=dev)
    L.call("gc_rasterize_nd_fwd", H, W, tb[0], tb[1], C, ids_s, bins, xys, conics, colors, opac, background, out, fT, fi)
    return out, fT, fi


def _rasterize_nd_bwd(H, W, tb, N, ids_s, bins, xys, conics, colors, opac, background, fT, fi, v_out, v_alpha):
    dev = xys.device
    C = colors.shape[1]
    v_xy = torch.zeros(N, 2, device=dev); v_conic = torch.zeros(N, 3, device=dev)
    v_col = torch.zeros(N, C, device=dev); v_op = torch.zeros(N, device=dev)
    L.call("gc_rasterize_nd_bwd", H, W, tb[0], tb[1], N, C, ids_s, bins, xys, conics, colors, opac, background, fT, fi, v_out, v_alpha,
           v_xy, v_conic, v_col, v_op)
    return v_xy, v_conic, v_col, v_op


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity, H, W, background, return_alpha):
        _need_gpu(xys, colors)
        if colors.dim() != 2 or colors.shape[1] < 1:
            raise ValueError("rasterize_gaussians: colors must be [N,C] with C >= 1")
        N, C = xys.shape[0], colors.shape[1]
        if background is not None and background.numel() != C:
            raise ValueError(f"rasterize_gaussians: background has {background.numel()} values, colors has {C} channels")
        dev = xys.device
        tb = ((W + TILE - 1) // TILE, (H + TILE - 1) // TILE, 1)
        x, d, r, c, nth = _c(xys), _c(depths), _c(radii, torch.int32), _c(conics), _c(num_tiles_hit, torch.int32)
        col, op = _c(colors), _c(opacity).reshape(-1)
        bg = _c(background).reshape(-1) if background is not None else torch.ones(C, device=dev)
        M, keys_s, ids_s, bins, _ = bin_and_sort_gaussians(N, x, d, r, nth, tb)
        if C == 3:
            out, _, fT, fi = _rasterize_fwd(H, W, tb, ids_s, bins, x, c, col, op, None, bg)
        else:                                   # gsplat's nd_rasterize_forward
            out, fT, fi = _rasterize_nd_fwd(H, W, tb, ids_s, bins, x, c, col, op, bg)
        ctx.save_for_backward(ids_s, bins, x, c, col, op, bg, fT, fi)
        ctx.meta = (H, W, tb, N)
        if return_alpha:
            return out, 1 - fT
        return out

    @staticmethod
    def backward(ctx, v_out, v_alpha=None):
        ids_s, bins, x, c, col, op, bg, fT, fi = ctx.saved_tensors
        H, W, tb, N = ctx.meta
        vo = _c(v_out)
        va = _c(v_alpha) if v_alpha is not None else None
        bwd = _rasterize_bwd if col.shape[1] == 3 else _rasterize_nd_bwd
        v_xy, v_conic, v_col, v_op = bwd(H, W, tb, N, ids_s, bins, x, c, col, op, bg, fT, fi, vo, va)
        return v_xy, None, None, v_conic, None, v_col, v_op[:, None], None, None, None, None


def rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, colors, opacity, img_height, img_width,
                        background=None, return_alpha=False):
    """gsplat 0.1.3 signature; colors[N,C] for any C >= 1 -> out_img[H,W,C] (, out_alpha[H,W]).  C == 3 runs the RGB kernels
    (gc_rasterize_fwd / _bwd), every other C the N-channel ones (gc_rasterize_nd_fwd / _bwd), as gsplat dispatches.  background[C]
    defaults to ones(C); uint8 colours are divided by 255."""
    if colors.dtype == torch.uint8:
        colors = colors.float() / 255
    return _RasterizeGaussians.apply(xys, depths, radii, conics, num_tiles_hit, colors, opacity, img_height, img_width,
                                     background, return_alpha)


# --------------------------------------------------------------------------------------------- fused path
TIGHT_BOXES = True          # default of RenderAux.tight_boxes for the fused render_view path


class RenderAux:
    """Side outputs of render_view (non-differentiable state the model keeps, gc_model.py:140,159-160)."""
    xys = None
    radii = None
    num_tiles_hit = None
    depths = None
    xys_grad = None
    M = 0
    gaussian_ids_sorted = None
    tile_bins = None
    final_index = None
    isect_ids_sorted = None
    m_cap = None          # set to an intersection capacity for the sync-free path: M then is (count, overflow) device tensors
    # Gradient accumulation inside the backward kernel: grad_into = {"means", "scales", "quats", "opacities", "features_dc",
    # "features_rest"} -> fp32 tensors shaped like the parameters.  The backward then writes (grad_accumulate = False) or adds
    # (True) the six leaf gradients there and hands autograd None for them -- no separate read-add-write pass per tensor and view.
    grad_into = None
    grad_accumulate = False
    # Tight tile boxes (round 3): bin a Gaussian only into the tiles of the bounding box of its alpha >= 1/255 ellipse (inside gsplat's
    # 3-sigma box): ~31 % fewer (tile, Gaussian) pairs, images and gradients bit-identical.  num_tiles_hit / M / gaussian_ids_sorted /
    # tile_bins then describe the SHORTER lists; set False for the lists gsplat would build (the gsplat-shaped operators always do).
    tight_boxes = None            # None: module default TIGHT_BOXES
    tile_boxes = None
    # render_views (round 6): True = the gather-free depth order (gc_raster_order_boxes_views + gc_raster_bin_sorted_views: the packed boxes ride
    # through the radix passes, culled Gaussians drop out in the first pass); False = the round-5 chain (same lists bit for bit; A/B and cross-checks)
    sorted_boxes = True
    # Depth supervision: True (with want_depth and parameters that require grad) makes the depth image differentiable -- the backward then
    # runs gc_rasterize_bwd_depth_views / gc_project_sh_bwd_depth_views.  False: depth is marked non-differentiable, as it always was.
    depth_grad = False
    # rasterize_mode "antialiased" of later splatfacto / gsplat versions (include/gaussctrl_antialias.h): every view multiplies the opacity by
    # rho = sqrt(max(0, det(cov2d) / det(cov2d + 0.3 I))), so that the 0.3 px^2 blur does not brighten splats thinner than a pixel.  False: the
    # classic mode, gsplat 0.1.3's (the reference has no other).  `compensation` is rho after an antialiased render: [N] from render_view,
    # [C, N] from render_views (0 where the view culls the Gaussian); None after a classic one.
    antialiased = False
    compensation = None
    # absgrad densification (AbsGS; use_absgrad of later splatfacto, include/gaussctrl_absgrad.h): True makes the compositing backward also sum
    # |dL_p/dx|, |dL_p/dy| over the pixels p of every Gaussian (rgb, alpha and depth combined per pixel, then abs) into `xys_absgrad`: [N, 2]
    # from render_view, [C, N, 2] from render_views; None until a backward with the switch has run.  xys_grad and the leaf gradients are what
    # they are without it.  Combines freely with depth_grad, antialiased and grad_into (the projection backward is not involved).
    absgrad = False
    xys_absgrad = None
    # camera pose refinement (include/gaussctrl_pose.h): True makes the projection backward also sum, over the Gaussians of every view, the
    # gradient with respect to the view's camera matrices (gcx_pose_bwd_views, on the same v_xy / v_conic / v_opac / v_depths the leaf backward
    # takes) and leave `viewmat_grad`: device float32 [C, 3, 4] (C = 1 from render_view), d loss / d viewmat[:3] of each `cam` dict, chained as
    # v_V + (projmat4^T v_P)[:3] because camera_to_gsplat forms fullproj = projmat4 @ viewmat4.  None until a backward with the switch has run.
    # The SH view directions move with the camera in the forward (cam["origin"]) but pass no gradient to the pose; they pass none to the means
    # either.  With the switch off nothing new runs; on, every output and leaf gradient is computed by the same launches as without it.
    pose_grad = False
    viewmat_grad = None
    # distortion loss (include/ext/gaussctrl_distort.h; the formulas are recalled from Mip-NeRF 360 / 2DGS and the header is the contract):
    # True (with parameters that require grad) makes the render also leave `distort_map`, per pixel the weighted spread in mapped depth of
    # the splats composited there: [H, W] from render_view, [C, H, W] from render_views, a differentiable output of the same autograd node.
    # distort_depth_map "linear" (t = z) or "ndc" (t = far (z - near) / ((far - near) z) with distort_near / distort_far).  When the map
    # received a cotangent, gcx_distort_bwd_views runs after the compositing backward and adds into its v_xy / v_conic / v_opacity and the
    # depth slice of the same zeroed buffer (there whether or not depth_grad is set); the projection backward then takes its depth form.
    # So grad_into, antialiased and pose_grad work as they are, aux.xys_grad includes the distortion's pull, and xys_absgrad (per-pixel
    # magnitudes of the image losses) does not.  False: nothing new is allocated or launched, every launch gets the arguments it always got.
    distort = False
    distort_depth_map = "linear"
    distort_near = 0.2
    distort_far = 100.0
    distort_map = None


DISTORT_DEPTH_MAPS = ("linear", "ndc")


def distort_depth_mode(name) -> int:
    """RenderAux.distort_depth_map -> depth_map of gcx_distort_*_views; anything but the two names is a ValueError"""
    if name not in DISTORT_DEPTH_MAPS:
        raise ValueError(f"distort_depth_map must be one of {DISTORT_DEPTH_MAPS}, got {name!r}")
    return DISTORT_DEPTH_MAPS.index(name)


def _finalize(ctx, npix, img, dep, fT):
    """alpha = 1 - T, depth / alpha, clamp(max=1).  Differentiable: the raw image stays for the clamp's backward (pre_clamp), no copy pass.
    Returns (img, alpha, pre_clamp | None)."""
    alpha = torch.empty_like(fT)
    if any(ctx.needs_input_grad[:6]):
        pre_clamp, img = img, torch.empty_like(img)
        L.call("gc_raster_finalize_into", npix, pre_clamp, img, dep, fT, alpha)
        return img, alpha, pre_clamp
    L.call("gc_raster_finalize", npix, img, dep, fT, alpha)
    return img, alpha, None


def _leaf_grad_buffers(aux, m, ls, q, dc, rest):
    """The six leaf-gradient tensors the projection backward fills: RenderAux.grad_into's (validated) or fresh ones.
    Returns (vm, vls, vq, vop, vdc, vrest), into (the caller's dict or None), acc (add to the buffers' contents)."""
    N, dev = m.shape[0], m.device
    into = aux.grad_into if aux is not None else None
    if into is None:
        return tuple(torch.empty(s, device=dev) for s in (m.shape, ls.shape, q.shape, (N,), dc.shape, rest.shape)), None, False
    bufs = tuple(into[k] for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest"))
    vm, vls, vq, vop, vdc, vrest = bufs
    for t, ref in ((vm, m), (vls, ls), (vq, q), (vdc, dc), (vrest, rest)):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.shape == ref.shape and t.device == dev
    assert vop.is_contiguous() and vop.dtype == torch.float32 and vop.numel() == N and vop.device == dev
    return bufs, into, bool(aux.grad_accumulate)


def _cams_host(cams: list):
    """list of `cam` dicts (camera_to_gsplat) -> ctypes float array [C][GC_VIEW_CAM_FLOATS = 35]"""
    flat = []
    for cam in cams:
        flat += list(cam["viewmat"])[:12] + list(cam["fullproj"])[:16] + list(cam["origin"])[:3] + [cam["fx"], cam["fy"], cam["cx"], cam["cy"]]
    return L.host_floats(flat)


def _leaf_params(means, log_scales, quats, opacities, features_dc, features_rest):
    """the six leaf tensors as the kernels read them (detached, fp32, contiguous, opacities flat) and the SH degree of features_rest"""
    sh_degree = {1: 0, 4: 1, 9: 2, 16: 3}[features_rest.shape[1] + 1]
    return (_c(means), _c(log_scales), _c(quats), _c(opacities).reshape(-1), _c(features_dc), _c(features_rest)), sh_degree


# what a fused backward needs next to the saved tensors; cams_host None: built when a batched entry point needs it; single: render_view
_RenderMeta = collections.namedtuple("_RenderMeta", "C N M_cap shared_op shared_bg H W tb sh_degree n_use cams cams_host single")


def _distort_fwd(ctx, aux, C, N, M_cap, shared_op, H, W, tb, ids_s, bins, xys, conics, opac, depths, single):
    """RenderAux.distort: the distortion map of the lists the compositing forward just walked.  Returns (map, wt, (depth_map, near, far)),
    or (None, None, None) with the switch off or nothing to differentiate.  Empty lists (a view that sees no Gaussian: ids_sorted has no
    element and no address) composite nothing: the map is zero without a launch, as the entry point leaves it for an empty scene"""
    if aux is None or not aux.distort or not any(ctx.needs_input_grad[:6]):
        return None, None, None
    how = (distort_depth_mode(aux.distort_depth_map), float(aux.distort_near), float(aux.distort_far))
    shape = (H, W) if single else (C, H, W)
    if ids_s.numel() == 0:
        return torch.zeros(shape, device=xys.device), torch.zeros(shape, device=xys.device), how
    dmap = torch.empty(shape, device=xys.device)
    wt = torch.empty_like(dmap)
    L.call("gcx_distort_fwd_views", C, N, M_cap, shared_op, H, W, tb[0], tb[1], ids_s, bins, xys, conics, opac, depths, *how, dmap, wt)
    return dmap, wt, how


def _end_forward(ctx, aux, want_depth, meta, comp, saved, depths, dep, nth, M, boxes, keys_s, wt=None, how=None):
    """What both fused forwards do last: fill `aux` (the gradients of an earlier backward are dropped), keep the backward's bookkeeping on
    ctx and save the tensors -- with the two depth tensors when the depth image is differentiable (RenderAux.depth_grad); otherwise depth
    is marked non-differentiable.  Returns the depth output (empty when there is none)."""
    m, ls, q, op, dc, rest, radii, conics, xys, rgbs, opac, ids_s, bins, bg, fT, fi, pre_clamp = saved
    if aux is not None:
        aux.xys, aux.radii, aux.num_tiles_hit, aux.M, aux.depths, aux.tile_boxes = xys, radii, nth, M, depths, boxes
        aux.gaussian_ids_sorted, aux.tile_bins, aux.final_index, aux.isect_ids_sorted = ids_s, bins, fi, keys_s
        aux.xys_grad = aux.xys_absgrad = aux.viewmat_grad = aux.distort_map = None
        aux.compensation = comp
    ctx.meta, ctx.aux = meta, aux
    ctx.comp = comp          # (not an input or output of the function: kept as an attribute)
    ctx.depth_grad = bool(want_depth and aux is not None and aux.depth_grad and any(ctx.needs_input_grad[:6]))
    ctx.distort = how        # RenderAux.distort: (depth_map, near, far); the backward's two tensors come last among the saved ones
    tail = (depths, wt) if how is not None else ()
    if ctx.depth_grad or how is not None:
        ctx.set_materialize_grads(False)     # an unused depth or distortion map arrives as None in backward, which then takes the path without it
    if ctx.depth_grad:
        ctx.save_for_backward(*saved, depths, dep, *tail)
    else:
        ctx.save_for_backward(*saved, *tail)
        if dep is not None:
            ctx.mark_non_differentiable(dep)
    return dep if dep is not None else torch.empty(0, device=m.device)


def _composite_bwd(ctx, v_img, v_alpha, v_dep, want_ex=False):
    """The compositing backward of render_view (C = 1, the batched entry points' single-view case) and render_views: ONE zeroed buffer for
    every output, the entry point picked by the switches; want_ex: the buffer has the v_ex slice even without a depth cotangent (the distortion
    backward adds into it).  Returns (v_xy, v_conic, v_col, v_op, v_ex | None, v_abs | None), shaped [N, ..]
    for render_view and [C, N, ..] for render_views, and leaves aux.xys_grad / aux.xys_absgrad (views of the buffer)."""
    conics, xys, rgbs, opac, ids_s, bins, bg, fT, fi, pre_clamp = ctx.saved_tensors[7:17]
    mt = ctx.meta
    C, N, M_cap, shared_op, shared_bg, H, W, tb = mt.C, mt.N, mt.M_cap, mt.shared_op, mt.shared_bg, mt.H, mt.W, mt.tb
    lead = (N,) if mt.single else (C, N)
    dev = xys.device
    vo = _c(v_img) if v_img is not None else torch.zeros(C, H, W, 3, device=dev)
    va = _c(v_alpha) if v_alpha is not None else None
    absgrad = ctx.aux is not None and ctx.aux.absgrad
    depths, dep, vd = (ctx.saved_tensors[17], ctx.saved_tensors[18], _c(v_dep)) if ctx.depth_grad and v_dep is not None else (None, None, None)
    parts = [("v_xy", 2), ("v_conic", 3), ("v_col", 3), ("v_op", 1)] + ([("v_ex", 1)] if vd is not None or want_ex else []) + ([("v_abs", 2)] if absgrad else [])
    vbuf = torch.zeros(C * N * sum(w for _, w in parts), device=dev)
    v = {k: t.view(*lead, *((w,) if w > 1 else ())) for (k, w), t in zip(parts, vbuf.split([C * N * w for _, w in parts]))}
    v_xy, v_conic, v_col, v_op, v_ex, v_abs = (v.get(k) for k in ("v_xy", "v_conic", "v_col", "v_op", "v_ex", "v_abs"))
    # (clamp(max=1) backward, gc_model.py:188: applied by the kernel when it loads the pixel's gradient)
    plain = (C, N, M_cap, shared_op, shared_bg, H, W, tb[0], tb[1], ids_s, bins, xys, conics, rgbs, opac, bg, fT, fi, vo, va, pre_clamp,
             v_xy, v_conic, v_col, v_op)
    if absgrad:                 # one entry point for both depth forms (NULL quartet = no depth)
        L.call("gc_rasterize_bwd_abs_views", *plain, depths, dep, vd, v_ex if vd is not None else None, v_abs)
    elif vd is not None:
        L.call("gc_rasterize_bwd_depth_views", *plain, depths, dep, vd, v_ex)
    else:
        L.call("gc_rasterize_bwd_views", *plain)
    if ctx.aux is not None:
        ctx.aux.xys_grad = v_xy
        if absgrad:
            ctx.aux.xys_absgrad = v_abs
    return v_xy, v_conic, v_col, v_op, v_ex, v_abs


def _project_bwd(ctx, v_xy, v_conic, v_col, v_op, v_ex):
    """The projection / SH backward to the six leaf tensors (or into RenderAux.grad_into: then autograd gets None for them).  The plain form
    of render_view launches the single-view kernel (its own memory schedule); everything else is a batched entry point, C = 1 included."""
    m, ls, q, op, dc, rest, radii, conics, _, rgbs = ctx.saved_tensors[:10]
    mt = ctx.meta
    C, N, H, W, sh_degree, n_use = mt.C, mt.N, mt.H, mt.W, mt.sh_degree, mt.n_use
    (vm, vls, vq, vop, vdc, vrest), into, acc = _leaf_grad_buffers(ctx.aux, m, ls, q, dc, rest)
    grads = (v_xy, v_conic, v_col, v_op, vm, vls, vq, vop, vdc, vrest)
    if mt.single and ctx.comp is None and v_ex is None:
        cam = mt.cams[0]
        L.call("gc_project_sh_bwd_accumulate" if acc else "gc_project_sh_bwd", N, m, ls, q, op, rgbs, sh_degree, n_use,
               L.host_floats(cam["viewmat"]), L.host_floats(cam["fullproj"]), L.host_floats(cam["origin"]), cam["fx"], cam["fy"], cam["cx"],
               cam["cy"], H, W, radii, conics, *grads)
    else:
        CH = mt.cams_host if mt.cams_host is not None else _cams_host(mt.cams)
        lead = (N, C, int(acc), m, ls, q, op, rgbs, sh_degree, n_use, CH, H, W, radii, conics)
        if ctx.comp is not None:    # antialiased: v_op is of the per-view effective opacities; v_depths may be NULL
            L.call("gc_project_sh_bwd_aa_views", *lead, ctx.comp, *grads, v_ex)
        elif v_ex is not None:      # the compositing's v_extra is the projection's v_depths
            L.call("gc_project_sh_bwd_depth_views", *lead, *grads, v_ex)
        else:
            L.call("gc_project_sh_bwd_views", *lead, *grads)
    if ctx.aux is not None and ctx.aux.pose_grad:
        ctx.aux.viewmat_grad = _pose_bwd(ctx, v_xy, v_conic, v_op, v_ex)
    if into is not None:
        return (None,) * 11
    return vm, vls, vq, vop[:, None], vdc, vrest, None, None, None, None, None


def pose_bwd_views(means, log_scales, quats, opacity_logits, cams, radii, conics, v_xy, v_conic, v_opac=None, v_depths=None, antialiased=False):
    """gcx_pose_bwd_views (include/gaussctrl_pose.h) on device tensors laid out as the fused render keeps them: radii [C, N] (or [N] for one
    camera), conics, v_xy, v_conic, v_opac, v_depths alike; cams: the list of `cam` dicts.  Returns the raw sums, float32 [C, 2, 3, 4]:
    [:, 0] = v_V, [:, 1] = rows 0, 1, 3 of v_P (row 2 is identically zero)."""
    _need_gpu(means, radii)
    N, C = means.shape[0], len(cams)
    H, W = cams[0]["H"], cams[0]["W"]
    nbytes = L.call("gcx_pose_bwd_views_workspace_bytes", N, C)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=means.device)
    out = torch.empty(C, 2, 3, 4, dtype=torch.float32, device=means.device)
    L.call("gcx_pose_bwd_views", N, C, 1 if antialiased else 0, means, log_scales, quats, opacity_logits, _cams_host(cams), H, W, radii, conics,
           v_xy, v_conic, v_opac, v_depths, ws, out)
    return out


def chain_viewmat_grad(raw, cams):
    """raw [C, 2, 3, 4] of pose_bwd_views -> d / d viewmat[:3] per view, float32 [C, 3, 4]: v_V + (projmat4^T v_P4)[:3] with v_P4 = v_P and a zero
    row 2 (camera_to_gsplat: fullproj = projmat4 @ viewmat4).  Sixteen multiply-adds per entry, taken in float64."""
    import numpy as np
    # [C, 3, 3]: rows 0..2 of projmat4^T, columns 0, 1, 3 (the rows of v_P that exist).  Kept on the device per set of projection matrices:
    # a training run has one or a few, and an upload per backward would make the host wait for the stream
    proj = [np.asarray(c["projmat4"], dtype=np.float64) for c in cams]
    key = (str(raw.device),) + tuple(p.tobytes() for p in proj)
    PT = _proj_t_cache.get(key)
    if PT is None:
        if len(_proj_t_cache) >= 16:
            _proj_t_cache.clear()
        PT = _proj_t_cache[key] = torch.from_numpy(np.stack([p.T[:3][:, [0, 1, 3]] for p in proj])).to(raw.device)
    r = raw.double()
    return (r[:, 0] + PT @ r[:, 1]).float()


_proj_t_cache = {}


def _pose_bwd(ctx, v_xy, v_conic, v_op, v_ex):
    """RenderAux.pose_grad: the camera gradient of the views of this render, from the cotangents the projection backward was just handed"""
    m, ls, q, op, _, _, radii, conics = ctx.saved_tensors[:8]
    aa = ctx.comp is not None
    raw = pose_bwd_views(m, ls, q, op, ctx.meta.cams, radii, conics, v_xy, v_conic, v_op if aa else None, v_ex, aa)
    return chain_viewmat_grad(raw, ctx.meta.cams)


def _distort_bwd(ctx, v_dist, v_xy, v_conic, v_op, v_ex):
    """RenderAux.distort: the distortion map's cotangent, added into the compositing backward's four arrays"""
    conics, xys, _, opac, ids_s, bins, _, fT, fi = ctx.saved_tensors[7:16]
    depths, wt = ctx.saved_tensors[-2:]
    mt = ctx.meta
    if ids_s.numel() == 0:          # empty lists: the map is identically zero, nothing to add
        return
    depth_map, near, far = ctx.distort
    L.call("gcx_distort_bwd_views", mt.C, mt.N, mt.M_cap, mt.shared_op, mt.H, mt.W, mt.tb[0], mt.tb[1], ids_s, bins, xys, conics, opac, depths,
           depth_map, near, far, fT, fi, wt, _c(v_dist), v_xy, v_conic, v_op, v_ex)


def _render_bwd(ctx, v_img, v_alpha, v_dep, v_dist=None):
    distort = ctx.distort is not None and v_dist is not None
    v_xy, v_conic, v_col, v_op, v_ex, _ = _composite_bwd(ctx, v_img, v_alpha, v_dep, distort)
    if distort:
        _distort_bwd(ctx, v_dist, v_xy, v_conic, v_op, v_ex)
    return _project_bwd(ctx, v_xy, v_conic, v_col, v_op, v_ex)


class _RenderView(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, log_scales, quats, opacities, features_dc, features_rest, cam, background, want_depth,
                sh_degree_to_use, aux):
        _need_gpu(means)
        N = means.shape[0]
        dev = means.device
        H, W = cam["H"], cam["W"]
        tb = ((W + TILE - 1) // TILE, (H + TILE - 1) // TILE, 1)
        (m, ls, q, op, dc, rest), sh_degree = _leaf_params(means, log_scales, quats, opacities, features_dc, features_rest)
        V, P, O = L.host_floats(cam["viewmat"]), L.host_floats(cam["fullproj"]), L.host_floats(cam["origin"])
        xys = torch.empty(N, 2, device=dev); depths = torch.empty(N, device=dev)
        radii = torch.empty(N, dtype=torch.int32, device=dev); conics = torch.empty(N, 3, device=dev)
        nth = torch.empty(N, dtype=torch.int32, device=dev)
        rgbs = torch.empty(N, 3, device=dev); opac = torch.empty(N, device=dev)
        tight = TIGHT_BOXES if (aux is None or aux.tight_boxes is None) else bool(aux.tight_boxes)
        tight = tight and tb[0] <= 255 and tb[1] <= 255
        boxes = torch.empty(N, dtype=torch.int32, device=dev) if tight else None
        aa = bool(aux is not None and aux.antialiased)
        comp = torch.empty(N, device=dev) if aa else None
        if aa:         # opac is this view's sigmoid(logit) * rho: what the compositing kernels and the tight boxes see
            L.call("gc_project_sh_fwd_aa_views", N, 1, m, ls, q, op, dc, rest, sh_degree, sh_degree_to_use, _cams_host([cam]), H, W, tb[0], tb[1],
                   0.01, xys, depths, radii, conics, nth, rgbs, opac, comp, boxes, None)
        else:
            plain = (N, m, ls, q, op, dc, rest, sh_degree, sh_degree_to_use, V, P, O, cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, tb[0], tb[1],
                     0.01, xys, depths, radii, conics, nth, rgbs, opac)
            if tight:
                L.call("gc_project_sh_fwd_boxes", *plain, boxes)
            else:
                L.call("gc_project_sh_fwd", *plain)
        M, keys_s, ids_s, bins, _ = bin_and_sort_gaussians(N, xys, depths, radii, nth, tb, m_cap=None if aux is None else aux.m_cap,
                                                           tile_boxes=boxes)
        bg = _c(background)
        extra = depths if want_depth else None
        img, dep, fT, fi = _rasterize_fwd(H, W, tb, ids_s, bins, xys, conics, rgbs, opac, extra, bg)
        img, alpha, pre_clamp = _finalize(ctx, H * W, img, dep, fT)
        meta = _RenderMeta(1, N, ids_s.numel(), 1, 1, H, W, tb, sh_degree, int(sh_degree_to_use), [cam], None, True)
        dmap, wt, how = _distort_fwd(ctx, aux, 1, N, ids_s.numel(), 1, H, W, tb, ids_s, bins, xys, conics, opac, depths, True)
        dep = _end_forward(ctx, aux, want_depth, meta, comp, (m, ls, q, op, dc, rest, radii, conics, xys, rgbs, opac, ids_s, bins, bg, fT, fi, pre_clamp),
                           depths, dep, nth, M, boxes, keys_s, wt, how)
        return img, alpha, dep, dmap

    backward = staticmethod(_render_bwd)


def render_view(means, log_scales, quats, opacities, features_dc, features_rest, cam: dict, background, want_depth: bool,
                sh_degree_to_use: int = 3, aux: RenderAux | None = None):
    """Fused get_outputs core.  cam: dict(viewmat[12], fullproj[16], origin[3], fx, fy, cx, cy, H, W) of HOST floats.
    Returns (rgb[H,W,3] clamped to <=1, alpha[H,W], depth[H,W] (normalised, 1000 where alpha==0) or empty).  depth carries no gradient
    unless aux.depth_grad is set (RenderAux)."""
    img, alpha, dep, dmap = _RenderView.apply(means, log_scales, quats, opacities, features_dc, features_rest, cam, background, want_depth,
                                              sh_degree_to_use, aux)
    if dmap is not None:          # RenderAux.distort: the fourth output of the node lives on aux
        aux.distort_map = dmap
    return img, alpha, dep


# --------------------------------------------------------------------------------------------- batched views
# what the front half of a batched launch set leaves for its compositing stage (render_views: the forward; trace_masks_views: the trace)
_ViewsFront = collections.namedtuple("_ViewsFront", "N C H W tb leaves sh_degree CH xys depths radii conics nth rgbs boxes opac comp shared_op "
                                                    "cnt ovf M_cap ids_s bins")


def _views_front(means, log_scales, quats, opacities, features_dc, features_rest, cams, sh_degree_to_use, aux):
    """Projection / SH, depth order and binning of C cameras of one scene: tight boxes, the sorted-boxes chain (or the pair chain with
    aux.sorted_boxes = False), the antialiased per-view opacities when aux.antialiased."""
    _need_gpu(means)
    N = means.shape[0]
    dev = means.device
    C = len(cams)
    H, W = cams[0]["H"], cams[0]["W"]
    assert all(c["H"] == H and c["W"] == W for c in cams), "the views of a batch share one image size"
    tb = ((W + TILE - 1) // TILE, (H + TILE - 1) // TILE, 1)
    T = tb[0] * tb[1]
    if tb[0] > 255 or tb[1] > 255:
        raise ValueError("render_views: at most 255 x 255 tiles (packed tile boxes)")
    (m, ls, q, op, dc, rest), sh_degree = _leaf_params(means, log_scales, quats, opacities, features_dc, features_rest)
    CH = _cams_host(cams)
    f32 = dict(device=dev, dtype=torch.float32); i32 = dict(device=dev, dtype=torch.int32)
    xys = torch.empty(C, N, 2, **f32); depths = torch.empty(C, N, **f32); radii = torch.empty(C, N, **i32)
    conics = torch.empty(C, N, 3, **f32); nth = torch.empty(C, N, **i32); rgbs = torch.empty(C, N, 3, **f32)
    boxes = torch.empty(C, N, **i32); pairs = torch.empty(C, N, 2, **i32)
    aa = bool(aux is not None and aux.antialiased)
    shared_op = 0 if aa else 1          # antialiased: per-view effective opacities [C][N], the compositing kernels' shared_opacities = 0
    if aa:
        opac = torch.empty(C, N, **f32); comp = torch.empty(C, N, **f32)
        L.call("gc_project_sh_fwd_aa_views", N, C, m, ls, q, op, dc, rest, sh_degree, sh_degree_to_use, CH, H, W, tb[0], tb[1], 0.01,
               xys, depths, radii, conics, nth, rgbs, opac, comp, boxes, pairs)
    else:
        opac = torch.empty(N, **f32); comp = None
        L.call("gc_project_sh_fwd_views", N, C, m, ls, q, op, dc, rest, sh_degree, sh_degree_to_use, CH, H, W, tb[0], tb[1], 0.01,
               xys, depths, radii, conics, nth, rgbs, opac, boxes, pairs)
    order = torch.empty(C, N, **i32); cum = torch.empty(C, N, **i32); cnt = torch.empty(C, **i32)
    sorted_boxes = bool(getattr(aux, "sorted_boxes", True)) if aux is not None else True
    if sorted_boxes:      # round 6: the boxes ride through the depth sort, culled Gaussians drop out in its first pass -- no per-Gaussian gathers
        bxs = torch.empty(C, N, **i32); nvis = torch.empty(C, **i32)
        wb = L.call("gc_raster_order_boxes_views_workspace_bytes", N, C)
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        L.call("gc_raster_order_boxes_views", N, C, pairs, boxes, order, bxs, cum, cnt, nvis, ws, wb)
    else:                 # the round-5 chain (A/B, cross-check tests)
        wb = L.call("gc_raster_depth_order_views_workspace_bytes", N, C)
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        L.call("gc_raster_depth_order_views", N, C, None, None, pairs, nth, order, cum, cnt, ws, wb)
    del pairs
    m_cap = None if aux is None else aux.m_cap
    if m_cap is None:                     # one readback of the C counts sizes the lists exactly (the sync-free form passes a capacity)
        M_cap = max(int(cnt.max().item()), 1)
    else:
        M_cap = int(m_cap)
    ids_s = torch.empty(C, M_cap, **i32); bins = torch.empty(C, T, 2, **i32); ovf = torch.empty(C, **i32)
    bb = L.call("gc_raster_bin_views_workspace_bytes", M_cap, C)
    del ws
    bws = torch.empty(bb, dtype=torch.uint8, device=dev)
    if sorted_boxes:
        L.call("gc_raster_bin_sorted_views", N, C, M_cap, cnt, ovf, nvis, order, bxs, cum, tb[0], tb[1], ids_s, bins, bws, bb)
        del bxs
    else:
        L.call("gc_raster_bin_tiles_views", N, C, M_cap, cnt, ovf, order, cum, boxes, depths, tb[0], tb[1], ids_s, bins, None, bws, bb)
    del bws
    return _ViewsFront(N, C, H, W, tb, (m, ls, q, op, dc, rest), sh_degree, CH, xys, depths, radii, conics, nth, rgbs, boxes, opac, comp, shared_op,
                       cnt, ovf, M_cap, ids_s, bins)


class _RenderViews(torch.autograd.Function):
    """C cameras of one scene through ONE set of launches (include/gaussctrl_hip.h "Batched views"): the parameter record is read once
    per batch by the projection / SH kernel and once by its backward, the sort / binning / compositing kernels run with the view as a
    grid dimension.  Per view the result is bit-identical to _RenderView (same device code); the leaf gradients are the sum over the
    views.  The reference has no such call: it renders one camera per get_outputs (gc_pipeline.py:124-130, gc_trainer.py:186-201)."""

    @staticmethod
    def forward(ctx, means, log_scales, quats, opacities, features_dc, features_rest, cams, backgrounds, want_depth, sh_degree_to_use, aux):
        fr = _views_front(means, log_scales, quats, opacities, features_dc, features_rest, cams, sh_degree_to_use, aux)
        N, C, H, W, tb, (m, ls, q, op, dc, rest), sh_degree, CH = fr[:8]
        xys, depths, radii, conics, nth, rgbs, boxes, opac, comp, shared_op, cnt, ovf, M_cap, ids_s, bins = fr[8:]
        del fr
        f32 = dict(device=means.device, dtype=torch.float32); i32 = dict(device=means.device, dtype=torch.int32)
        bg = _c(backgrounds)
        shared_bg = 1 if bg.dim() == 1 else 0
        assert bg.numel() == (3 if shared_bg else 3 * C)
        img = torch.empty(C, H, W, 3, **f32); fT = torch.empty(C, H, W, **f32); fi = torch.empty(C, H, W, **i32)
        dep = torch.empty(C, H, W, **f32) if want_depth else None
        L.call("gc_rasterize_fwd_views", C, N, M_cap, shared_op, shared_bg, H, W, tb[0], tb[1], ids_s, bins, xys, conics, rgbs, opac,
               depths if want_depth else None, bg, img, dep, fT, fi)
        img, alpha, pre_clamp = _finalize(ctx, C * H * W, img, dep, fT)
        meta = _RenderMeta(C, N, M_cap, shared_op, shared_bg, H, W, tb, sh_degree, int(sh_degree_to_use), cams, CH, False)
        # aux.M: per-view device counts / overflow flags ([C] each)
        dmap, wt, how = _distort_fwd(ctx, aux, C, N, M_cap, shared_op, H, W, tb, ids_s, bins, xys, conics, opac, depths, False)
        dep = _end_forward(ctx, aux, want_depth, meta, comp, (m, ls, q, op, dc, rest, radii, conics, xys, rgbs, opac, ids_s, bins, bg, fT, fi, pre_clamp),
                           depths, dep, nth, (cnt, ovf), boxes, None, wt, how)
        return img, alpha, dep, dmap

    backward = staticmethod(_render_bwd)


def render_views(means, log_scales, quats, opacities, features_dc, features_rest, cams: list, backgrounds, want_depth: bool,
                 sh_degree_to_use: int = 3, aux: RenderAux | None = None):
    """render_view for a LIST of cameras of one scene in one set of launches.  backgrounds: [3] (shared) or [C,3].
    Returns (rgb [C,H,W,3] clamped to <= 1, alpha [C,H,W], depth [C,H,W] or empty).  aux.M = (count [C], overflow [C]) device tensors;
    aux.m_cap = per-view intersection capacity for the sync-free form (else the C counts are read back once to size the lists)."""
    img, alpha, dep, dmap = _RenderViews.apply(means, log_scales, quats, opacities, features_dc, features_rest, list(cams), backgrounds, want_depth,
                                               sh_degree_to_use, aux)
    if dmap is not None:          # RenderAux.distort: the fourth output of the node lives on aux
        aux.distort_map = dmap
    return img, alpha, dep


# --------------------------------------------------------------------------------------------- edit-region tracing
@torch.no_grad()
def trace_masks_views(means, log_scales, quats, opacities, features_dc, features_rest, cams: list, masks, w_in, w_all, aux: RenderAux | None = None):
    """Lift the 2D masks of a LIST of cameras onto the Gaussians (include/gaussctrl_trace.h): the front half of render_views (projection,
    depth order, binning -- the same lists, bit for bit), then gc_trace_mask_views in place of the compositing forward.  masks [C,H,W]
    float32; w_in / w_all: float32 [N], ADDED into (w_in += sum vis * mask, w_all += sum vis over the views' pixels): zero them once, then
    call per batch of views.  aux: tight_boxes is not read (batched views always bin tight boxes); sorted_boxes, antialiased and m_cap act
    as in render_views; aux.M = (count [C], overflow [C]) afterwards.  No gradient."""
    _need_gpu(means, masks, w_in, w_all)
    N, C = means.shape[0], len(cams)
    for t, name in ((w_in, "w_in"), (w_all, "w_all")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != N:
            raise ValueError(f"trace_masks_views: {name} must be a contiguous float32 tensor of N = {N} elements")
    if C == 0 or N == 0:
        return
    H, W = cams[0]["H"], cams[0]["W"]
    if tuple(masks.shape) != (C, H, W):
        raise ValueError(f"trace_masks_views: masks must be [C, H, W] = {(C, H, W)}, got {tuple(masks.shape)}")
    mk = _c(masks)
    fr = _views_front(means, log_scales, quats, opacities, features_dc, features_rest, list(cams), 0, aux)
    if aux is not None:
        aux.M = (fr.cnt, fr.ovf)
    L.call("gc_trace_mask_views", C, N, fr.M_cap, fr.shared_op, H, W, fr.tb[0], fr.tb[1], fr.ids_s, fr.bins, fr.xys, fr.conics, fr.opac,
           mk, w_in, w_all)

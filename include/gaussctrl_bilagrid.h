/*
 * gaussctrl_bilagrid.h -- C ABI of libgaussctrl_hip.so, extension set: per-view bilateral grids of 3x4 colour transforms, sliced at
 * (x, y, luma) and applied to a render before the loss, and their total-variation regulariser.  Same conventions as gaussctrl_hip.h
 * (error codes, the last-error string, caller-owned memory, launches on `stream` only, no hidden synchronisation, GC_EINVAL before any
 * launch).  The four functions carry the prefix gcx_: they are an extension set beside the library's counted entry points, resolved by
 * the loader from its own list (gaussctrl_amd/_lib.py EXT_SYMBOLS).
 */
#ifndef GAUSSCTRL_BILAGRID_H
#define GAUSSCTRL_BILAGRID_H

#include "gaussctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- What later splatfacto / gsplat versions call use_bilateral_grid ("Bilateral Guided Radiance Field Processing"; gsplat 1.x
 * lib_bilagrid.py).  The reference of this project has none of it, and the formulas are recalled, not checked against their source: what
 * is written here is the contract.  Opt-in: nothing in gaussctrl_hip.h calls these.
 *
 * Layouts, all float32 and contiguous: grids [V][12][L][GH][GW] (channel k = 4 i + j is entry (i, j) of the 3x4 transform), images
 * [C][H][W][3]; view_idx is a HOST int32 [C] with every value in [0, V): image c is sliced from grid view_idx[c].
 *
 * Per pixel (c, y, x) with input r, g, b:
 *     u = (x + 0.5) / W * (GW - 1),  v = (y + 0.5) / H * (GH - 1),  z = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) * (L - 1)
 *     A[0..11] = the trilinear interpolation of grid view_idx[c] at (u, v, z), per channel: the cell on each axis is
 *                min(floor(.), size - 2), so the upper vertex is never outside the grid (and is never read outside it, whatever its
 *                weight) -- grid_sample with align_corners = True, padding_mode = "border"
 *     out_i   = A[4 i] r + A[4 i + 1] g + A[4 i + 2] b + A[4 i + 3]
 * GC_EINVAL (both slice functions, before anything is launched): a NULL pointer, C < 1, H < 1, W < 1, V < 1, GW / GH / L < 2, a view_idx
 * value outside [0, V), C H W 3 >= 2^31 or V 12 L GH GW >= 2^31, H > 16 * 65535.  (No empty call exists: an image needs a grid.) */
int gcx_bilagrid_slice_fwd_views(int C, int H, int W, int V, int GW, int GH, int L, const float *grids, const float *rgb,
                                 const int32_t *view_idx, float *out, void *stream);

/* The backward of the slice from v_out [C][H][W][3].  The call ADDS into v_grids [V][12][L][GH][GW] (the caller zeroes it; images that
 * share a view index add into one grid, a grid no image names is not touched):
 *     v_grids[view_idx[c]][k] at each of the 8 vertices += (its trilinear weight) * v_out_i * {r, g, b, 1}[j],   k = 4 i + j
 * and WRITES v_rgb [C][H][W][3]:
 *     v_rgb_j = sum_i A[4 i + j] v_out_i  +  {0.299, 0.587, 0.114}[j] * (L - 1) * sum_k v_A[k] * dA[k]/dz
 * where v_A[4 i + j] = v_out_i * {r, g, b, 1}[j] and dA[k]/dz is the difference of the two z levels of the cell, interpolated in x and
 * y; the second term is zero where the clamp of z is active (luma <= 0 or >= 1).
 * A workgroup sums the contributions of its pixel tile in LDS, over the slab of grid vertices the tile can reach (lanes of a wave that
 * share a grid cell are summed in registers first), and leaves one float atomic per touched grid element; where that slab does not fit
 * the LDS the same per-wave, per-cell sums are global float atomics themselves.  Float atomics: the sums can differ in their last bits
 * from run to run. */
int gcx_bilagrid_slice_bwd_views(int C, int H, int W, int V, int GW, int GH, int L, const float *grids, const float *rgb,
                                 const int32_t *view_idx, const float *v_out, float *v_grids, float *v_rgb, void *stream);

/* Total variation over all V grids: for each of the three spatial axes the mean of the squared forward differences over that axis's
 * [V][12][...] difference tensor; tv = the sum of the three means.  tv: device float32 [1], WRITTEN.  v_grids [V][12][L][GH][GW]:
 * weight * d tv / d grids is ADDED to it (one owner per element: no atomics, the same bits every run).  workspace: at least
 * gcx_bilagrid_tv_workspace_bytes(V, GW, GH, L) bytes, 8-byte aligned.
 * GC_EINVAL: V < 0, GW / GH / L < 2, V 12 L GH GW >= 2^31; with V > 0 also a NULL pointer, a workspace smaller than the query's answer
 * and a weight that is NaN.  V = 0 returns GC_OK and launches nothing (tv is not written). */
size_t gcx_bilagrid_tv_workspace_bytes(int V, int GW, int GH, int L);
int gcx_bilagrid_tv_fwd_bwd(int V, int GW, int GH, int L, const float *grids, float weight, float *tv, float *v_grids, void *workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GAUSSCTRL_BILAGRID_H */

/*
 * gaussctrl_distort.h -- C ABI of libgaussctrl_hip.so, distortion loss: per pixel, the weighted spread in depth of the splats composited
 * there, and its backward to the compositing inputs and the projected depths.  Same conventions as gaussctrl_hip.h (error codes,
 * caller-owned memory, launches on `stream` only, no hidden synchronisation, GC_EINVAL before any launch).
 */
#ifndef GAUSSCTRL_DISTORT_H
#define GAUSSCTRL_DISTORT_H

#include "../gaussctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The distortion regulariser of Mip-NeRF 360 / 2DGS (gsplat 1.x returns it as render_distort).  The reference of this project (gsplat
 * 0.1.3, nerfstudio 1.0) has none of this, and the formulas are recalled from the papers, not checked against their source: what is written
 * here is the contract.  Opt-in: nothing in gaussctrl_hip.h calls these.
 *
 * For one view and one pixel let i = 0 .. K-1 be the list entries the compositing forward composites there, front to back -- the same alpha
 * cap (0.999), the same 1/255 cull and the same stop at T <= 1e-4 as gc_rasterize_fwd_views, on the same lists.  Per entry: alpha_i, T_i the
 * transmittance in front of it, w_i = alpha_i T_i, z_i = depths[gid], t_i = m(z_i) with
 *     depth_map 0 ("linear")   m(z) = z
 *     depth_map 1 ("ndc")      m(z) = far (z - near) / ((far - near) z),   m'(z) = far near / ((far - near) z^2),   0 < near < far
 * (a composited Gaussian has z > 0: the projection culls the others).  With A_i = 1 - T_i (= sum_{j<i} w_j) and B_i = sum_{j<i} w_j t_j
 *     distort = 2 sum_i w_i (t_i A_i - B_i)          wt = sum_i w_i t_i
 * For non-decreasing t this is sum_i sum_j w_i w_j |t_i - t_j|; the prefix form is the definition, so ties and the quantised keys of the
 * depth order need no special case.  A pixel with nothing composited has distort = wt = 0.
 *
 * gcx_distort_fwd_views writes distort and wt, float32 [C][H][W].  depths [C][N]; gaussian_ids_sorted [C][M_cap], tile_bins [C][T][2], xys
 * [C][N][2], conics [C][N][3], opacities [N] (shared_opacities = 1) or [C][N]: the view strides of gc_rasterize_fwd_views.  No colour and
 * no image is read or written.
 * GC_EINVAL, as gc_trace_mask_views: C outside 1..65535, N < 0, M_cap < 0, tile bounds that do not match the image size; and a depth_map
 * outside {0, 1}; depth_map 1 without 0 < near_plane < far_plane < infinity (a NaN included; depth_map 0 does not read the two); any NULL array when
 * N > 0.  N = 0 returns GC_OK without a launch, after zeroing the two images (those that are not NULL). */
int gcx_distort_fwd_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int img_h, int img_w, int tiles_x, int tiles_y,
                          const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                          const float *opacities, const float *depths, int depth_map, float near_plane, float far_plane,
                          float *distort, float *wt, void *stream);

/* The backward for an upstream v_distort [C][H][W] (nothing flows through wt).  final_Ts / final_index [C][H][W]: what gc_rasterize_fwd_views
 * left on the same lists; wt: what gcx_distort_fwd_views left.  With the suffix sums S_i = sum_{k>i} w_k, Bs_i = sum_{k>i} w_k t_k and
 * R_i = sum_{k>i} w_k dD/dw_k
 *     dD/dw_i     = 2 [ (t_i A_i - B_i) + (Bs_i - t_i S_i) ]
 *     dD/dt_i     = 2 w_i (A_i - S_i)
 *     dD/dalpha_i = T_i dD/dw_i - R_i / (1 - alpha_i)
 * and g = v_distort[pixel]: g dD/dalpha_i takes the path of every compositing backward to v_xy [C][N][2], v_conic [C][N][3] and v_opacity
 * [C][N] (an alpha at the cap passes nothing to sigma or the opacity), and v_depths[gid] += g dD/dt_i m'(z_i), [C][N] (the cap does not
 * block this one).  Nothing goes to colours; there is no background term.  The call ADDS into the four arrays, laid out as
 * gc_rasterize_bwd_depth_views lays out v_xy / v_conic / v_opacity / v_extra: run it after that call on the same buffers, or zero them.
 * Float atomics: the sums can differ in their last bits from run to run.
 * GC_EINVAL: as the forward.  N = 0 returns GC_OK without a launch. */
int gcx_distort_bwd_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int img_h, int img_w, int tiles_x, int tiles_y,
                          const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                          const float *opacities, const float *depths, int depth_map, float near_plane, float far_plane,
                          const float *final_Ts, const int32_t *final_index, const float *wt, const float *v_distort, float *v_xy,
                          float *v_conic, float *v_opacity, float *v_depths, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GAUSSCTRL_DISTORT_H */

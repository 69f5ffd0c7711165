/*
 * gaussctrl_absgrad.h -- C ABI of libgaussctrl_hip.so, absgrad densification: the compositing backward that also sums the per-pixel
 * |dL/dxy| of every Gaussian.  Same conventions as gaussctrl_hip.h (error codes, caller-owned memory, launches on `stream` only, no hidden
 * synchronisation).
 */
#ifndef GAUSSCTRL_ABSGRAD_H
#define GAUSSCTRL_ABSGRAD_H

#include "gaussctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- What later splatfacto / gsplat versions call use_absgrad / absgrad (AbsGS).  The compositing backward of gaussctrl_hip.h hands back
 * v_xy = sum over pixels p of dL_p/dxy, the SIGNED screen-space gradient: a large splat whose pixels pull in opposite directions sums to
 * about zero and is never split.  This entry point returns, next to it,
 *     v_xy_abs[c][n] = sum over pixels p of (|dL_p/dx_n|, |dL_p/dy_n|)
 * where dL_p is the pixel's whole contribution -- rgb, alpha and (with the depth quartet) depth combined BEFORE the absolute value, which is
 * gsplat's definition.  A (pixel, Gaussian) pair that passes no gradient to the position (alpha at the 0.999 cap, alpha < 1/255, behind the
 * pixel's last composited Gaussian) adds 0.  The quantity exists only inside the backward kernel, before its per-row reduction.
 * Opt-in: nothing in gaussctrl_hip.h calls this, and every other output is what the forms without it write.
 *
 * The arguments of gc_rasterize_bwd_depth_views plus v_xy_abs [C][N][2], which must be ZERO on entry like the other outputs (the kernel adds
 * into them).  The depth quartet (extra, depth, v_depth, v_extra) is all NULL -- then this is gc_rasterize_bwd_views plus v_xy_abs -- or all
 * set; a mixed quartet or a NULL v_xy_abs (with N > 0), C outside 1..65535, N < 0 or M_cap < 0 is GC_EINVAL before any launch.  C = 1 is the
 * single-view case (M_cap is then not read).  The result feeds gc_refine_accumulate_views (gaussctrl_refine.h) in place of v_xy. */
int gc_rasterize_bwd_abs_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int shared_background, int img_h, int img_w, int tiles_x,
                               int tiles_y, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                               const float *colors, const float *opacities, const float *background, const float *final_Ts,
                               const int32_t *final_index, const float *v_out, const float *v_out_alpha, const float *pre_clamp, float *v_xy,
                               float *v_conic, float *v_colors, float *v_opacity, const float *extra, const float *depth, const float *v_depth,
                               float *v_extra, float *v_xy_abs, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GAUSSCTRL_ABSGRAD_H */

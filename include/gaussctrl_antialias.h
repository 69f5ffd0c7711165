/*
 * gaussctrl_antialias.h -- C ABI of libgaussctrl_hip.so, antialiased rasterize_mode: the per-view opacity compensation of the fused render.
 * Same conventions as gaussctrl_hip.h (error codes, caller-owned memory, launches on `stream` only, no hidden synchronisation).
 */
#ifndef GAUSSCTRL_ANTIALIAS_H
#define GAUSSCTRL_ANTIALIAS_H

#include "gaussctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- What later splatfacto / gsplat versions call rasterize_mode = "antialiased" (the Mip-Splatting opacity compensation).  gsplat 0.1.3,
 * which the entry points of gaussctrl_hip.h reproduce, has no such mode: it adds 0.3 to the diagonal of every projected 2 x 2 covariance and
 * keeps the splat's opacity, which brightens and fattens Gaussians thinner than a pixel.  Here each view multiplies the opacity by
 *     rho = sqrt(max(0, det(cov2d) / det(cov2d + 0.3 I)))            (0 for a Gaussian the view culls)
 * Opt-in: nothing in gaussctrl_hip.h calls these.  xys / depths / radii / conics and gsplat's tile box are those of the classic entry points
 * bit for bit; the tight tile boxes are computed for the effective opacity and are therefore smaller.
 *
 * Forward, C views (C = 1: the single-view case; launches of <= 8 views; per-view results do not depend on the batch).  The arguments of
 * the batched classic forward, except: opac [C][N] = sigmoid(opacity_logits) * rho of the view -- pass it to the compositing entry points
 * of gaussctrl_hip.h (the *_views forms with shared_opacities = 0; for one view any of the single-view forms) -- and compensation [C][N] =
 * rho.  tile_boxes [C][N] and depth_pairs [C][N][2] are optional (NULL) as there.  GC_EINVAL before any launch for N < 0, C < 1, a NULL
 * cams / parameter / output pointer, an SH degree outside 0..3 or tile_boxes with more than 255 x 255 tiles; N = 0 returns GC_OK. */
int gc_project_sh_fwd_aa_views(int64_t N, int C, const float *means, const float *log_scales, const float *quats,
                               const float *opacity_logits, const float *features_dc, const float *features_rest, int sh_degree,
                               int degrees_to_use, const float *cams, int img_h, int img_w, int tiles_x, int tiles_y, float clip_thresh,
                               float *xys, float *depths, int32_t *radii, float *conics, int32_t *num_tiles_hit, float *rgbs, float *opac,
                               float *compensation, uint32_t *tile_boxes, uint32_t *depth_pairs, void *stream);

/* Backward.  v_opac [C][N] is the gradient w.r.t. the per-view effective opacity (v_opacity of the compositing backward with
 * shared_opacities = 0).  Per view it adds v_opac * rho * op (1 - op) to v_opacity_logits (op = sigmoid(logit)) and sends v_opac * op through
 * d rho / d cov2d into the gradients of means, log-scales and quaternions, next to the conic's.  rgbs / radii / conics / compensation / v_xy /
 * v_conic / v_rgbs are [C][N][..] as the forward wrote them; v_depths [C][N] is the depth gradient of the depth-supervised backward, or NULL for
 * no depth term.  Views sum in view order; accumulate = 1 adds to the six output buffers, 0 writes them.  `compensation` must be the
 * forward's array (not NULL); the kernels recompute rho from the covariance they rebuild, so its contents are not re-read. */
int gc_project_sh_bwd_aa_views(int64_t N, int C, int accumulate, const float *means, const float *log_scales, const float *quats,
                               const float *opacity_logits, const float *rgbs, int sh_degree, int degrees_to_use, const float *cams,
                               int img_h, int img_w, const int32_t *radii, const float *conics, const float *compensation,
                               const float *v_xy, const float *v_conic, const float *v_rgbs, const float *v_opac, float *v_means,
                               float *v_log_scales, float *v_quats, float *v_opacity_logits, float *v_features_dc, float *v_features_rest,
                               const float *v_depths, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GAUSSCTRL_ANTIALIAS_H */

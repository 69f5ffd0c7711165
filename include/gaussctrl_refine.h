/*
 * gaussctrl_refine.h -- C ABI of libgaussctrl_hip.so, refinement part: splatfacto's densification step on the device.
 * Same conventions as gaussctrl_hip.h (error codes, caller-owned memory, launches on `stream` only, no hidden synchronisation).
 */
#ifndef GAUSSCTRL_REFINE_H
#define GAUSSCTRL_REFINE_H

#include "gaussctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Refinement (densification) of a splat scene on the device: splatfacto's after_train / refinement_after [nerfstudio 1.0.0
 * splatfacto.py] -- screen-space gradient statistics, split / duplicate, cull, opacity reset.  Opt-in: nothing above calls these.
 * The six tensors of a scene are always listed in the order means[N,3] scales[N,3] quats[N,4] opacities[N,1] features_dc[N,3]
 * features_rest[N,R] (R = 0, 9, 24 or 45 floats).  N = 0 is a no-op that returns GC_OK.  Limits (GC_EINVAL): n_split_samples 1 .. 4; every
 * operand below 2^31 elements (N * 45 * (n_split_samples + 2), the largest scene one refinement can produce, is the bound checked). */
#define GC_REFINE_MAX_SPLIT 4
/* the per-Gaussian action word gc_refine_plan writes */
#define GC_REFINE_KEEP 1u          /* the original survives */
#define GC_REFINE_SPLIT 2u         /* split source (never survives) */
#define GC_REFINE_DUP 4u           /* duplicate source */
#define GC_REFINE_EMIT_SPLIT 8u    /* its n_split_samples split children survive the cull */
#define GC_REFINE_EMIT_DUP 16u     /* its duplicate survives the cull */
#define GC_REFINE_BELOW_ALPHA 32u  /* sigmoid(opacity) < cull_alpha_thresh (children share it) */
#define GC_REFINE_TOO_BIG 64u      /* cull_by_scale and max(exp(scales)) > cull_scale_thresh */
#define GC_REFINE_ON_SCREEN 128u   /* cull_by_screen and max_2dsize > cull_screen_size */

/* after_train for C views (C = 1: one view): xys_grad [C][N][2], radii [C][N]; for every view with radii > 0, in view order:
 * grad_norm_sum += sqrt(gx^2 + gy^2), vis_count += 1, max_2dsize = max(max_2dsize, radii * inv_max_dim) (inv_max_dim = 1 / max(H, W)).
 * The three statistics are float32 [N], read and written in place; a C-view call equals C single-view calls bit for bit. */
int gc_refine_accumulate_views(int64_t N, int C, const float *xys_grad, const int32_t *radii, float inv_max_dim, float *grad_norm_sum,
                               float *vis_count, float *max_2dsize, void *stream);

/* The decisions of one refinement.  With densify: avg = grad_norm_sum / vis_count * 0.5 * max_dim (vis_count == 0: never high),
 * high = avg > densify_grad_thresh, big = max(exp(scales)) > densify_size_thresh,
 * split = (big | (split_by_screen & max_2dsize > split_screen_size)) & high, dup = !big & high.  A split source is removed and emits
 * n_split_samples children with scales - log 1.6, a dup source emits one copy.  The cull applies to every row: sigmoid(opacity) <
 * cull_alpha_thresh; with cull_by_scale max(exp(scales)) > cull_scale_thresh (split children on their reduced scales); with
 * cull_by_screen max_2dsize > cull_screen_size (originals only).  Without densify (cull only) the statistics may be NULL.
 * Writes action [N] (GC_REFINE_* bits), ranks [3][N] = exclusive counts, in index order, of the survivors / the split sources whose
 * children are emitted / the dup sources whose copy is emitted, and counts (device int32[5]) = {n_survivors, n_split_src, n_dup_src,
 * n_out = n_survivors + n_split_samples * n_split_src + n_dup_src, n_below_alpha (rows of the grown set, children included)}.
 * No host synchronisation: the caller reads counts back (20 bytes) to size the new tensors.
 * workspace >= gc_refine_plan_workspace_bytes(N), 4-byte aligned. */
size_t gc_refine_plan_workspace_bytes(int64_t N);
int gc_refine_plan(int64_t N, const float *log_scales, const float *opacity_logits, const float *grad_norm_sum, const float *vis_count,
                   const float *max_2dsize, int densify, int n_split_samples, float max_dim, float densify_grad_thresh,
                   float densify_size_thresh, int split_by_screen, float split_screen_size, float cull_alpha_thresh, int cull_by_scale,
                   float cull_scale_thresh, int cull_by_screen, float cull_screen_size, uint32_t *action, int32_t *ranks, int32_t *counts,
                   void *workspace, size_t workspace_bytes, void *stream);

/* One pass builds the new scene from action / ranks and the three counts read back from gc_refine_plan.  params / exp_avg / exp_avg_sq /
 * out_*: HOST arrays of six device pointers (order above).  The out tensors hold n_out rows and are DIFFERENT buffers from the inputs.
 * Output rows: survivor with rank r -> r; child k of the split source with rank j -> n_survivors + k * n_split_src + j, its mean =
 * mean + Rot(quat / |quat|) (exp(scales) * samples[k * n_split_src + j]) (samples [n_split_samples * n_split_src][3], standard normal
 * draws of the caller; NULL allowed when n_split_src == 0), scales - log 1.6, everything else the source's; the duplicate of the dup source
 * with rank j -> n_survivors + n_split_samples * n_split_src + j, an exact copy.  Moments: copied for survivors, zero for children.
 * A moment array pointer, or an entry of it, may be NULL (an optimizer that has not stepped) together with its out counterpart: that
 * tensor is then neither read nor written.  rest_floats = R; with R = 0 entry 5 of every array is ignored. */
int gc_refine_apply(int64_t N, int n_split_samples, int rest_floats, int64_t n_survivors, int64_t n_split_src, int64_t n_dup_src,
                    const uint32_t *action, const int32_t *ranks, const float *samples, const float *const *params,
                    const float *const *exp_avg, const float *const *exp_avg_sq, float *const *out_params, float *const *out_exp_avg,
                    float *const *out_exp_avg_sq, void *stream);

/* splatfacto's opacity reset in one launch: opacities = min(opacities, reset_logit) with reset_logit = logit(2 * cull_alpha_thresh)
 * (formed by the caller), both moments zero (either may be NULL). */
int gc_refine_reset_opacity(int64_t N, float reset_logit, float *opacities, float *exp_avg, float *exp_avg_sq, void *stream);


#ifdef __cplusplus
}
#endif

#endif /* GAUSSCTRL_REFINE_H */

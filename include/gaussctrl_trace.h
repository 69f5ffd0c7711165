/*
 * gaussctrl_trace.h -- C ABI of libgaussctrl_hip.so, edit-region tracing: lift 2D edit masks onto the Gaussians by the compositing weights
 * they receive, pick the traced rows, and take the Adam step on those rows only.  Same conventions as gaussctrl_hip.h (error codes,
 * caller-owned memory, launches on `stream` only, no hidden synchronisation, GC_EINVAL before any launch).
 */
#ifndef GAUSSCTRL_TRACE_H
#define GAUSSCTRL_TRACE_H

#include "gaussctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- What GaussianEditor calls semantic tracing.  The reference of this project composites the unedited pixels back in image space only
 * (gc_pipeline.py:226-234) and then trains every Gaussian; it has none of this, and the formulas are recalled from the paper, not checked
 * against its source: what is written here is the contract.  Opt-in: nothing in gaussctrl_hip.h calls these.
 *
 * For every view c, every pixel p and every Gaussian n that the compositing forward composites at p, vis = alpha * T is the weight the
 * forward gives n's colour at p -- the same alpha cap (0.999), the same 1/255 cull and the same stop at T <= 1e-4 as gc_rasterize_fwd_views,
 * on the same lists.  The call ADDS
 *     w_in[n]  += sum over (c, p) of vis * masks[c][p]
 *     w_all[n] += sum over (c, p) of vis
 * into the two float32 [N] arrays (one pair for all views: the caller zeroes them once, then calls per batch of views).
 * masks: float32 [C][H][W], any value (0..1 in practice).  gaussian_ids_sorted [C][M_cap], tile_bins [C][T][2], xys [C][N][2], conics
 * [C][N][3], opacities [N] (shared_opacities = 1) or [C][N]: the view strides of gc_rasterize_fwd_views.  No image, no colour, no
 * final_Ts / final_index is read or written.  Float atomics: the sums can differ in their last bits from run to run.
 * GC_EINVAL, as gc_rasterize_bwd_abs_views: C outside 1..65535, N < 0, M_cap < 0, tile bounds that do not match the image size; and a
 * NULL masks, w_in or w_all when N > 0.  N = 0 returns GC_OK without a launch. */
int gc_trace_mask_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int img_h, int img_w, int tiles_x, int tiles_y,
                        const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                        const float *opacities, const float *masks, float *w_in, float *w_all, void *stream);

/* select[n] = (w_all[n] > min_weight && w_in[n] > ratio_thresh * w_all[n]), as uint8 0 / 1; count: device int32[1], set to the number
 * selected (integer atomics: the result does not depend on timing).  A Gaussian no view composites (w_all == 0) is never selected,
 * whatever the two thresholds.  No host synchronisation: the caller reads count back (4 bytes).  GC_EINVAL: N < 0, a threshold that is
 * NaN, a NULL count, or a NULL array when N > 0.  N = 0 sets count to 0. */
int gc_trace_select(int64_t N, const float *w_in, const float *w_all, float ratio_thresh, float min_weight, uint8_t *select,
                    int32_t *count, void *stream);

/* gc_adam_step on the elements of the rows with row_select != 0: param / grad / exp_avg / exp_avg_sq are [rows][row_floats] float32,
 * row_select uint8 [rows].  A selected element gets the bits gc_adam_step gives it; in every other row the parameter and both moments keep
 * their bits, and a 16-byte chunk without a selected element is neither loaded nor stored.  GC_EINVAL: a NULL pointer, rows < 0,
 * row_floats < 1, step < 1, rows * row_floats >= 2^31.  rows = 0 is a no-op. */
int gc_adam_step_rows(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t rows, int row_floats,
                      const uint8_t *row_select, float lr, float beta1, float beta2, float eps, int step, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GAUSSCTRL_TRACE_H */

/*
 * gaussctrl_pose.h -- C ABI of libgaussctrl_hip.so, extension set: the gradient of the per-Gaussian front end (projection of the fused
 * render) with respect to the CAMERA, summed over the Gaussians of every view.  Same conventions as gaussctrl_hip.h (error codes, the
 * last-error string, caller-owned memory, launches on `stream` only, no hidden synchronisation, GC_EINVAL before any launch).  The two
 * functions carry the prefix gcx_: they are an extension set beside the library's counted entry points, resolved by the loader from a
 * list of its own (gaussctrl_amd/_lib.py POSE_SYMBOLS).  Opt-in: nothing in gaussctrl_hip.h calls these.
 */
#ifndef GAUSSCTRL_POSE_H
#define GAUSSCTRL_POSE_H

#include "gaussctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- What a per-view pose adjustment (later splatfacto / gsplat 1.x: camera_optimizer, mode SO3xR3) needs from the renderer.
 *
 * The projection reads two camera matrices per view: V, the 3x4 world-to-camera matrix (camera-space mean t = V (p, 1), depth = t_z,
 * the frustum clamp, the Jacobian J of the perspective division and T = J V[:, :3] of the 2D covariance T Sigma T^T), and P, the 4x4 full
 * projection (pixel centre from rows 0, 1 and 3 of P (p, 1); row 2 is never read).  Given the cotangents the projection backward of the
 * fused render takes, the call writes, per view c,
 *
 *     v_V = sum over the Gaussians the view kept (radii > 0) of d <outputs, cotangents> / d V      [3][4]
 *     v_P = the same with respect to P                                                              rows 0, 1, 3 of [4][4]
 *
 * treating V and P as independent.  A caller whose P is projmat V4 (V4 = V over the row 0 0 0 1) chains
 *     d / d V = v_V + (projmat^T v_P4)[:3],      v_P4 = v_P with a zero row 2.
 *
 * Layout of out, float32 [C][2][3][4]:
 *     out[c][0][r][k] = v_V[r][k]                       r = 0..2, k = 0..3
 *     out[c][1][0][k] = v_P[0][k],   out[c][1][1][k] = v_P[1][k],   out[c][1][2][k] = v_P[3][k]
 * Row 2 of v_P is identically zero and has no slot.
 *
 * Contract.  The SH view directions move with the camera in the forward (cam_origin) but pass NO gradient to the pose, as they pass
 * none to the means: the colour cotangent is not an argument.  The outputs differentiated are xys (v_xy), conics (v_conic), depths
 * (v_depths, may be NULL: no depth term) and, antialiased != 0 only, the per-view effective opacity sigmoid(logit) * rho (v_opac; the
 * cotangent of rho is v_opac * sigmoid(logit)).  v_opac is not read, and may be NULL, when antialiased == 0.  A Gaussian with
 * radii <= 0 in a view contributes nothing to that view; the integer outputs and the culls carry no gradient.
 *
 * Arguments as the projection backward over C views takes them: means [N][3], log_scales [N][3], quats [N][4] (raw),
 * opacity_logits [N]; cams a HOST float array [C][GC_VIEW_CAM_FLOATS = 35] (viewmat[12] | projmat[16] | cam_origin[3] | fx fy cx cy per
 * view); radii [C][N] int32, conics [C][N][3], v_xy [C][N][2], v_conic [C][N][3], v_opac [C][N], v_depths [C][N].  Views are processed
 * in groups of 8 per launch.
 *
 * Reduction: every workgroup leaves one float32 partial per view in `workspace`; a second kernel adds the partials of a view in a fixed
 * order in double precision and rounds once.  No atomics: the same inputs give the same bits, run to run.  workspace: device memory of
 * at least gcx_pose_bwd_views_workspace_bytes(N, C) bytes, 4-byte aligned; no byte beyond that size is touched.
 *
 * GC_EINVAL (before anything is launched): C < 1, N < 0, C * N * 3 >= 2^31 (the per-view arrays are addressed with 32-bit element
 * offsets elsewhere in the library), img_h or img_w < 1, out NULL, cams NULL; with N > 0 also a NULL parameter, radii, conics, v_xy,
 * v_conic or workspace pointer, and a NULL v_opac when antialiased != 0.  N == 0 writes zeros to out and touches nothing else. */
size_t gcx_pose_bwd_views_workspace_bytes(int64_t N, int C);
int gcx_pose_bwd_views(int64_t N, int C, int antialiased, const float *means, const float *log_scales, const float *quats,
                       const float *opacity_logits, const float *cams, int img_h, int img_w, const int32_t *radii, const float *conics,
                       const float *v_xy, const float *v_conic, const float *v_opac, const float *v_depths, void *workspace, float *out,
                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GAUSSCTRL_POSE_H */

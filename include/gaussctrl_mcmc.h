/*
 * gaussctrl_mcmc.h -- C ABI of libgaussctrl_hip.so, MCMC densification part: relocate dead Gaussians, grow to a cap, perturb the means.
 * Same conventions as gaussctrl_hip.h / gaussctrl_refine.h (error codes, caller-owned memory, launches on `stream` only, no hidden
 * synchronisation).
 */
#ifndef GAUSSCTRL_MCMC_H
#define GAUSSCTRL_MCMC_H

#include "gaussctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The densification strategy of 3DGS-MCMC ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat 1.x MCMCStrategy).  The
 * reference of this project has none of it and the formulas are recalled from the paper, not checked against its source: what is written
 * here is the contract.  Opt-in: nothing above calls these.  The six tensors of a scene are listed in the order means[N,3] scales[N,3]
 * quats[N,4] opacities[N,1] features_dc[N,3] features_rest[N,R] (R = 0, 9, 24 or 45 floats).  N = 0 and n = 0 are no-ops that return
 * GC_OK.  Every operand must stay below 2^31 elements (GC_EINVAL): N * 45, and (N + n) * 45 where rows are appended. */

/* Dead rows and sampling weights.  a = sigmoid(opacity_logits[i]) rounded to float32; row i is dead iff a <= min_opacity;
 * weights[i] = dead ? 0 : a (float32 [N]: weight 0 and dead are the same fact); dead_idx (int32 [N]) receives the dead rows in ascending
 * order in its first n_dead entries (the rest is not written); counts = device int32[2] {n_dead, n_alive}.  No host synchronisation: the
 * caller reads counts back (8 bytes).  workspace >= gc_mcmc_dead_workspace_bytes(N), 4-byte aligned. */
size_t gc_mcmc_dead_workspace_bytes(int64_t N);
int gc_mcmc_dead(int64_t N, const float *opacity_logits, float min_opacity, float *weights, int32_t *dead_idx, int32_t *counts,
                 void *workspace, size_t workspace_bytes, void *stream);

/* Relocation / growth, in place.  sampled_idx: int32 [n], values in [0, N): the live rows drawn (with repetition) by the caller.
 * dest_idx: int32 [n] rows in [0, N) that receive the copies (the dead rows), or NULL: copy j goes to row N + j and every tensor holds at
 * least N + n rows.  mult: int32 [N] scratch OUTPUT, cleared and filled here: mult[i] = #{j : sampled_idx[j] == i}.
 * Every row i with mult[i] > 0:  r = min(mult[i] + 1, 51), o = sigmoid(opacity_i), o_new = -expm1(log1p(-o) / r),
 *   D = sum_{i'=1..r} sum_{k=0..i'-1} C(i'-1, k) (-1)^k o_new^(k+1) / sqrt(k+1)   ( = sum_{m=1..r} C(r, m) (-1)^(m-1) o_new^m / sqrt(m) ),
 *   scales_i += log(o / D) on the three log-scales, opacity_i = logit(clamp(o_new, min_opacity, 1 - 2^-23)), every moment row i = 0;
 * evaluated in double from the float32 inputs and rounded once (o is limited to 1 - 2^-23 first, where the formulas stay finite).
 * Then row d_j (dest_idx[j] or N + j) of the six tensors becomes a copy of the UPDATED row sampled_idx[j], its moment rows zero.  Every
 * other row and moment keeps its bits.  The caller guarantees that the destination rows are distinct and disjoint from the sampled rows
 * (dead rows have weight 0).  An index outside its range, in sampled_idx or dest_idx, is never dereferenced: an entry whose sampled_idx is
 * out of range changes nothing; one whose dest_idx is out of range writes no row (mult still counts its draw).  Stream-ordered launches
 * (count, update the sources, copy); integer atomics only, so the result does not depend on timing.
 * params / exp_avg / exp_avg_sq: HOST arrays of six device pointers (order above).  A moment array pointer, or an entry of it, may be NULL
 * (an optimizer that has not stepped): that tensor is neither read nor written.  rest_floats = R; with R = 0 entry 5 is ignored. */
int gc_mcmc_relocate(int64_t N, int64_t n, int rest_floats, const int32_t *sampled_idx, const int32_t *dest_idx, float min_opacity,
                     int32_t *mult, float *const *params, float *const *exp_avg, float *const *exp_avg_sq, void *stream);

/* The per-step perturbation, one launch, one pass (56 bytes read, 12 written per Gaussian):
 *   means_i += Rot(quat_i / |quat_i|) diag(exp(2 scales_i)) Rot^T noise_i * g(sigmoid(opacity_i)) * scaler,
 *   g(o) = 1 / (1 + exp(100 (o - 0.005))) in float32: above o of about 0.885 the exponential overflows, g is exactly 0 and the mean keeps
 *   its bits, as it does for scaler = 0.
 * noise [N][3]: standard normal draws of the caller.  Only means is written. */
int gc_mcmc_inject_noise(int64_t N, float *means, const float *log_scales, const float *quats, const float *opacity_logits,
                         const float *noise, float scaler, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GAUSSCTRL_MCMC_H */

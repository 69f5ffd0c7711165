// train_mcmc.hip -- the densification strategy of 3DGS-MCMC (gsplat 1.x MCMCStrategy; formulas recalled, include/gaussctrl_mcmc.h is the
// contract) as streaming HIP kernels for gfx950: a scene of fixed size whose dead Gaussians are moved to where opacity lives, which grows
// 5 % at a time up to a cap, and whose means are perturbed after every optimizer step.
//
//   k_mcmc_dead_flag / k_mcmc_dead_scan / k_mcmc_dead_compact   sigmoid, the dead test, the sampling weights; per-workgroup counts -> exclusive
//                         offsets + the two totals (one workgroup) -> the dead rows in ascending order (stable compaction by ballot ranks).
//   k_mcmc_count          mult[i] = how often row i was drawn (integer atomics: order-independent).
//   k_mcmc_update         one lane per Gaussian; the drawn ones (a few per cent) get their new opacity and scales, formed in double and
//                         rounded once, and zero moments.
//   k_mcmc_copy           one lane per draw: the updated source row into its destination row (a dead row, or row N + j), moments zero; the
//                         features_rest rows move as contiguous R-float segments, the workgroup's lanes side by side.
//   k_mcmc_inject_noise   the per-step hot path, one lane per Gaussian: 56 bytes in, 12 out.  The rotation and the two 3 x 3 products are
//                         formed in double from the float32 inputs (about 70 FMAs at the fp32 rate on this chip; the kernel stays
//                         HBM-bound), the gate g and exp(2 s) in float32 as the header states them.
// update runs before copy, so a copy is the updated row bit for bit and D (up to 51 terms) is formed once per source, not once per draw.
// Sampled rows and destination rows are disjoint by the caller's contract, so no launch reads what it writes in another lane.
#include "train_rows.h"
#include "../../include/gaussctrl_mcmc.h"

namespace {

constexpr int MAX_RATIO = 51;             // r = min(mult + 1, 51)
constexpr double MAX_OPACITY = 1.0 - 0x1p-23;

__device__ __forceinline__ double sigmoid64(float x) { return 1.0 / (1.0 + exp(-(double)x)); }

// ---------------------------------------------------------------------------------------------------------------- dead rows
__global__ __launch_bounds__(256) void k_mcmc_dead_flag(int64_t N, const float *__restrict__ op_logit, float min_opacity,
                                                        float *__restrict__ weights, int32_t *__restrict__ block_sums)
{
    __shared__ int32_t red[4];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLK + tid;
    bool dead = false;
    if (i < N) {
        const float a = (float)sigmoid64(op_logit[i]);
        dead = !(a > min_opacity);                     // a <= min_opacity; a NaN opacity is dead too (weight 0, never sampled)
        weights[i] = dead ? 0.f : a;
    }
    const int c = __popcll(__ballot(dead));
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) block_sums[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup: block_sums [nblk] -> exclusive offsets in place, counts = {n_dead, N - n_dead}.
__global__ __launch_bounds__(256) void k_mcmc_dead_scan(int64_t N, int64_t nblk, int32_t *__restrict__ block_sums, int32_t *__restrict__ counts)
{
    const int32_t n_dead = scan_counts(block_sums, nblk, true);
    if (threadIdx.x == 0) { counts[0] = n_dead; counts[1] = (int32_t)(N - n_dead); }
}

__global__ __launch_bounds__(256) void k_mcmc_dead_compact(int64_t N, const float *__restrict__ weights, const int32_t *__restrict__ block_offs,
                                                           int32_t *__restrict__ dead_idx)
{
    __shared__ int32_t wcnt[4];
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const bool dead = i < N && weights[i] == 0.f;      // weight 0 and dead are the same fact (min_opacity >= 0)
    const uint64_t b = __ballot(dead);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (!dead) return;
    const int32_t r = ballot_rank(block_offs[blockIdx.x], b, wcnt);
    if (r >= 0 && r < N) dead_idx[r] = (int32_t)i;
}

// ---------------------------------------------------------------------------------------------------------------- relocate / grow
__global__ __launch_bounds__(256) void k_mcmc_count(int64_t N, int64_t n, const int32_t *__restrict__ sampled, int32_t *__restrict__ mult)
{
    const int64_t j = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (j >= n) return;
    const int32_t s = sampled[j];
    if (s >= 0 && s < N) atomicAdd(&mult[s], 1);
}

template <int R>
__global__ __launch_bounds__(256) void k_mcmc_update(int64_t N, const int32_t *__restrict__ mult, float min_opacity, Rows t)
{
    __shared__ uint8_t hit[BLK];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * BLK, i = i0 + tid;
    const int m = i < N ? mult[i] : 0;
    if (m > 0) {
        const int r = m + 1 < MAX_RATIO ? m + 1 : MAX_RATIO;
        const double o = fmin(sigmoid64(t.t[0][3][i]), MAX_OPACITY);
        const double o_new = -expm1(log1p(-o) / (double)r);
        // D = sum_{m=1..r} C(r, m) (-1)^(m-1) o_new^m / sqrt(m): the header's double sum with the inner binomials summed (hockey stick)
        double c = 1.0, p = 1.0, D = 0.0;
        for (int k = 1; k <= r; ++k) {
            c = c * (double)(r - k + 1) / (double)k;
            p *= o_new;
            const double term = c * p / sqrt((double)k);
            D += (k & 1) ? term : -term;
        }
        const double inc = log(o / D);
        float *ls = t.t[0][1];
#pragma unroll
        for (int a = 0; a < 3; ++a) ls[3 * i + a] = (float)((double)ls[3 * i + a] + inc);
        const double oc = fmin(fmax(o_new, (double)min_opacity), MAX_OPACITY);
        t.t[0][3][i] = (float)(log(oc) - log1p(-oc));
        zero_narrow_moments(t, i);
    }
    if constexpr (R > 0) {
        hit[tid] = m > 0;
        __syncthreads();
        const int nhere = (int)(N - i0 < BLK ? N - i0 : BLK);
#pragma unroll 1
        for (int q = 1; q < 3; ++q) {
            float *dst = t.t[q][5];
            if (!dst) continue;                                       // (kernel argument: uniform)
            for (int e = tid; e < nhere * R; e += BLK)
                if (hit[e / R]) dst[i0 * R + e] = 0.f;
        }
    }
}

template <int R>
__global__ __launch_bounds__(256) void k_mcmc_copy(int64_t N, int64_t n, int64_t n_rows, const int32_t *__restrict__ sampled,
                                                   const int32_t *__restrict__ dest, Rows t)
{
    __shared__ int32_t ssrc[BLK], sdst[BLK];
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * BLK, j = j0 + tid;
    int32_t s = -1, d = -1;
    if (j < n) {
        const int32_t s0 = sampled[j];
        const int64_t d0 = dest ? (int64_t)dest[j] : N + j;
        if (s0 >= 0 && s0 < N && d0 >= 0 && d0 < n_rows) { s = s0; d = (int32_t)d0; }      // an index out of range: the entry is skipped
    }
    if (s >= 0) {
        copy_narrow(t, s, d);
        zero_narrow_moments(t, d);
    }
    if constexpr (R > 0) {
        ssrc[tid] = s; sdst[tid] = d;
        __syncthreads();
        const int nhere = (int)(n - j0 < BLK ? n - j0 : BLK);
#pragma unroll 1
        for (int q = 0; q < 3; ++q) {
            float *p = t.t[q][5];
            if (!p) continue;                                         // (kernel argument: uniform)
            for (int e = tid; e < nhere * R; e += BLK) {
                const int r = e / R, c = e - r * R;
                if (ssrc[r] < 0) continue;
                p[(int64_t)sdst[r] * R + c] = q == 0 ? p[(int64_t)ssrc[r] * R + c] : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- noise
__global__ __launch_bounds__(256) void k_mcmc_inject_noise(int64_t N, float *__restrict__ means, const float *__restrict__ log_scales,
                                                           const float *__restrict__ quats, const float *__restrict__ op_logit,
                                                           const float *__restrict__ noise, float scaler)
{
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= N) return;
    const float o = 1.f / (1.f + expf(-op_logit[i]));
    const float g = 1.f / (1.f + expf(100.f * (o - 0.005f)));        // expf overflows to inf above o ~ 0.885: g = 0 exactly
    const float gs = g * scaler;
    if (gs == 0.f) return;                                           // the mean keeps its bits (and its 44 other bytes are not read)
    const float4 qf = reinterpret_cast<const float4 *>(quats)[i];
    const float e0 = expf(2.f * log_scales[3 * i]), e1 = expf(2.f * log_scales[3 * i + 1]), e2 = expf(2.f * log_scales[3 * i + 2]);
    const double n0 = noise[3 * i], n1 = noise[3 * i + 1], n2 = noise[3 * i + 2];
    // R^T n, scaled by exp(2 s), then R v: the covariance never exists as a matrix
    const Rot64 rot(qf.x, qf.y, qf.z, qf.w);
    const Vec64 u = rot.mul_t(n0, n1, n2);
    const Vec64 d = rot.mul((double)e0 * u.x, (double)e1 * u.y, (double)e2 * u.z);
    const double k = (double)gs;
    means[3 * i] = (float)((double)means[3 * i] + d.x * k);
    means[3 * i + 1] = (float)((double)means[3 * i + 1] + d.y * k);
    means[3 * i + 2] = (float)((double)means[3 * i + 2] + d.z * k);
}

}  // namespace

extern "C" {

size_t gc_mcmc_dead_workspace_bytes(int64_t N) { return sizeof(int32_t) * (size_t)(N > 0 ? (N + BLK - 1) / BLK : 1); }

/* Dead rows, sampling weights and the two counts; see the header. */
int gc_mcmc_dead(int64_t N, const float *opacity_logits, float min_opacity, float *weights, int32_t *dead_idx, int32_t *counts,
                 void *workspace, size_t workspace_bytes, void *stream)
{
    GC_REQUIRE(N >= 0, "bad arguments");
    GC_REQUIRE(min_opacity >= 0.f && min_opacity < 1.f, "min_opacity must be in [0, 1)");
    GC_REQUIRE(fits_i32(N), "N must be < 2^31 elements");
    if (N == 0) return GC_OK;
    GC_REQUIRE(opacity_logits && weights && dead_idx && counts && workspace, "null argument");
    if (workspace_bytes < gc_mcmc_dead_workspace_bytes(N)) { gc::set_error("gc_mcmc_dead: workspace too small"); return GC_ENOSPC; }
    const int64_t nblk = (N + BLK - 1) / BLK;
    int32_t *sums = (int32_t *)workspace;
    hipStream_t s = gc::S(stream);
    hipLaunchKernelGGL(k_mcmc_dead_flag, dim3((unsigned)nblk), dim3(BLK), 0, s, N, opacity_logits, min_opacity, weights, sums);
    hipLaunchKernelGGL(k_mcmc_dead_scan, dim3(1), dim3(256), 0, s, N, nblk, sums, counts);
    hipLaunchKernelGGL(k_mcmc_dead_compact, dim3((unsigned)nblk), dim3(BLK), 0, s, N, (const float *)weights, (const int32_t *)sums, dead_idx);
    return gc::check_launch("gc_mcmc_dead");
}

int gc_mcmc_relocate(int64_t N, int64_t n, int rest_floats, const int32_t *sampled_idx, const int32_t *dest_idx, float min_opacity,
                     int32_t *mult, float *const *params, float *const *exp_avg, float *const *exp_avg_sq, void *stream)
{
    GC_REQUIRE(N >= 0 && n >= 0, "bad arguments");
    GC_REQUIRE(rest_floats == 0 || rest_floats == 9 || rest_floats == 24 || rest_floats == 45, "features_rest must hold 0, 9, 24 or 45 floats per Gaussian");
    GC_REQUIRE(min_opacity >= 0.f && min_opacity < 1.f, "min_opacity must be in [0, 1)");
    GC_REQUIRE(fits_i32(N) && fits_i32(n), "N and n must be < 2^31");
    const int64_t n_rows = dest_idx ? N : N + n;
    GC_REQUIRE(fits_i32(n_rows * MAX_REST), "rows * 45 must be < 2^31 elements");
    if (N == 0 || n == 0) return GC_OK;
    GC_REQUIRE(sampled_idx && mult && params, "null argument");
    Rows t;
    GC_REQUIRE(fill_rows(t, rest_floats, params, exp_avg, exp_avg_sq), "null parameter tensor");
    hipStream_t s = gc::S(stream);
    if (hipMemsetAsync(mult, 0, sizeof(int32_t) * (size_t)N, s) != hipSuccess) return gc::check_launch("gc_mcmc_relocate");
    hipLaunchKernelGGL(k_mcmc_count, dim3(gc::cdiv(n, BLK)), dim3(BLK), 0, s, N, n, sampled_idx, mult);
    with_rest_floats(rest_floats, [&](auto R) {
        hipLaunchKernelGGL(k_mcmc_update<decltype(R)::value>, dim3(gc::cdiv(N, BLK)), dim3(BLK), 0, s, N, (const int32_t *)mult, min_opacity, t);
        hipLaunchKernelGGL(k_mcmc_copy<decltype(R)::value>, dim3(gc::cdiv(n, BLK)), dim3(BLK), 0, s, N, n, n_rows, sampled_idx, dest_idx, t);
    });
    return gc::check_launch("gc_mcmc_relocate");
}

int gc_mcmc_inject_noise(int64_t N, float *means, const float *log_scales, const float *quats, const float *opacity_logits,
                         const float *noise, float scaler, void *stream)
{
    GC_REQUIRE(N >= 0, "bad arguments");
    GC_REQUIRE(fits_i32(N * 4), "N * 4 must be < 2^31 elements");
    if (N == 0) return GC_OK;
    GC_REQUIRE(means && log_scales && quats && opacity_logits && noise, "null argument");
    GC_REQUIRE(((uintptr_t)quats & 15) == 0, "quats must be 16-byte aligned");
    hipLaunchKernelGGL(k_mcmc_inject_noise, dim3(gc::cdiv(N, BLK)), dim3(BLK), 0, gc::S(stream), N, means, log_scales, quats, opacity_logits,
                       noise, scaler);
    return gc::check_launch("gc_mcmc_inject_noise");
}

}  // extern "C"

// train_refine.hip -- splatfacto's refinement step (after_train + refinement_after of nerfstudio 1.0.0 splatfacto.py: screen-space gradient
// statistics, split / duplicate, cull, opacity reset) as streaming HIP kernels for gfx950.
//
// One refinement is   plan (3 small launches)  ->  20-byte read-back of the counts  ->  apply (1 launch)  [-> reset (1 launch)].
//   k_refine_accumulate   one lane per Gaussian, the C views folded in index order inside the lane (bit-identical to C single-view calls).
//   k_refine_decide       the per-Gaussian action word from parameters, statistics, thresholds and step flags + per-workgroup counts;
//   k_refine_scan_blocks  one workgroup turns the per-workgroup counts into exclusive offsets and writes the five totals;
//   k_refine_ranks        survivor / split / duplicate rank of every Gaussian (three exclusive scans, one pass over the action words).
//   k_refine_apply        one pass builds the NEW scene: per source Gaussian the 59-float record of the six tensors and of both Adam moments
//                         is read once and every output row the Gaussian owns is written (survivor: copy; child: moments zero).  The
//                         features_rest block (45 floats = 180 B per Gaussian, x 3 tensors) never moves per lane: the workgroup's 256
//                         source records are ONE contiguous 46 080-byte span (16-byte loads into LDS, as k_project_sh_fwd stages it), and
//                         the survivors / the k-th split children / the duplicates of a workgroup are each ONE contiguous span of output
//                         rows (the ranks are monotone), written with 256 contiguous bytes per wave instruction.
//   k_refine_reset_opacity  opacities = min(opacities, reset_logit), both moments zero.
// All HBM-bound: apply moves 59 x 4 x 3 = 708 B in and 708 B out per surviving Gaussian.  Built with the STRICT flags (no contraction):
// the decisions compare float expressions with thresholds, and the expressions are the ones written here.
#include "train_rows.h"
#include "../../include/gaussctrl_refine.h"

namespace {

constexpr float LOG_SIZE_FAC = 0.4700036292457356f;      // log(1.6): a split child's scales are the source's - log(1.6)

__global__ __launch_bounds__(256) void k_refine_accumulate(int64_t N, int C, const float *__restrict__ xys_grad, const int32_t *__restrict__ radii,
                                                           float inv_max_dim, float *__restrict__ grad_norm_sum, float *__restrict__ vis_count,
                                                           float *__restrict__ max_2dsize)
{
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= N) return;
    float s = grad_norm_sum[i], c = vis_count[i], m = max_2dsize[i];
    bool seen = false;
    for (int v = 0; v < C; ++v) {
        const int32_t r = radii[(int64_t)v * N + i];
        if (r > 0) {
            const float2 g = reinterpret_cast<const float2 *>(xys_grad)[(int64_t)v * N + i];
            s += sqrtf(g.x * g.x + g.y * g.y);
            c += 1.f;
            m = fmaxf(m, (float)r * inv_max_dim);
            seen = true;
        }
    }
    if (seen) { grad_norm_sum[i] = s; vis_count[i] = c; max_2dsize[i] = m; }
}

struct PlanArgs {
    int densify, n_split, split_by_screen, cull_by_scale, cull_by_screen;
    float max_dim, densify_grad_thresh, densify_size_thresh, split_screen_size, cull_alpha_thresh, cull_scale_thresh, cull_screen_size;
};

// per-workgroup counts: block_sums [4][nblk] = survivors, emitting split sources, emitting duplicate sources, rows below the alpha threshold
__global__ __launch_bounds__(256) void k_refine_decide(int64_t N, int64_t nblk, const float *__restrict__ log_scales, const float *__restrict__ op_logit,
                                                       const float *__restrict__ grad_norm_sum, const float *__restrict__ vis_count,
                                                       const float *__restrict__ max_2dsize, PlanArgs a, uint32_t *__restrict__ action,
                                                       int32_t *__restrict__ block_sums)
{
    __shared__ int32_t red[4][4];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLK + tid;
    uint32_t act = 0;
    int below_rows = 0;
    if (i < N) {
        const float l0 = log_scales[3 * i], l1 = log_scales[3 * i + 1], l2 = log_scales[3 * i + 2];
        const float smax = fmaxf(fmaxf(expf(l0), expf(l1)), expf(l2));
        const float alpha = 1.f / (1.f + expf(-op_logit[i]));
        const bool below = alpha < a.cull_alpha_thresh;
        const float m2d = (a.densify && a.split_by_screen) || a.cull_by_screen ? max_2dsize[i] : 0.f;
        bool split = false, dup = false;
        if (a.densify) {
            const float cnt = vis_count[i];
            bool high = false;
            if (cnt > 0.f)              // never seen: torch's 0 / 0 = NaN compares false; here the division is not made
                high = grad_norm_sum[i] / cnt * 0.5f * a.max_dim > a.densify_grad_thresh;
            const bool big = smax > a.densify_size_thresh;
            split = (big || (a.split_by_screen && m2d > a.split_screen_size)) && high;
            dup = !big && high;
        }
        const bool too_big = a.cull_by_scale && smax > a.cull_scale_thresh;
        const bool on_screen = a.cull_by_screen && m2d > a.cull_screen_size;
        const float cmax = fmaxf(fmaxf(expf(l0 - LOG_SIZE_FAC), expf(l1 - LOG_SIZE_FAC)), expf(l2 - LOG_SIZE_FAC));     // a split child's scales
        const bool child_too_big = a.cull_by_scale && cmax > a.cull_scale_thresh;
        if (!split && !below && !too_big && !on_screen) act |= GC_REFINE_KEEP;
        if (split) act |= GC_REFINE_SPLIT;
        if (dup) act |= GC_REFINE_DUP;
        if (split && !below && !child_too_big) act |= GC_REFINE_EMIT_SPLIT;
        if (dup && !below && !too_big) act |= GC_REFINE_EMIT_DUP;          // (a duplicate carries max_2dsize 0: no screen test)
        if (below) act |= GC_REFINE_BELOW_ALPHA;
        if (too_big) act |= GC_REFINE_TOO_BIG;
        if (on_screen) act |= GC_REFINE_ON_SCREEN;
        action[i] = act;
        below_rows = below ? 1 + (split ? a.n_split : 0) + (dup ? 1 : 0) : 0;
    }
    const int w = tid >> 6;
    const int c0 = __popcll(__ballot((act & GC_REFINE_KEEP) != 0)), c1 = __popcll(__ballot((act & GC_REFINE_EMIT_SPLIT) != 0)),
              c2 = __popcll(__ballot((act & GC_REFINE_EMIT_DUP) != 0));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) below_rows += __shfl_xor(below_rows, d, 64);
    if ((tid & 63) == 0) { red[0][w] = c0; red[1][w] = c1; red[2][w] = c2; red[3][w] = below_rows; }
    __syncthreads();
    if (tid < 4) block_sums[tid * nblk + blockIdx.x] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// One workgroup: block_sums [4][nblk] -> exclusive offsets in place (rows 0..2; row 3 is only summed), counts[5] = {n_survivors,
// n_split_src, n_dup_src, n_out, n_below_alpha}.
__global__ __launch_bounds__(256) void k_refine_scan_blocks(int64_t nblk, int n_split, int32_t *__restrict__ block_sums, int32_t *__restrict__ counts)
{
    const int32_t n_surv = scan_counts(block_sums, nblk, true), n_split_src = scan_counts(block_sums + nblk, nblk, true),
                  n_dup_src = scan_counts(block_sums + 2 * nblk, nblk, true), n_below = scan_counts(block_sums + 3 * nblk, nblk, false);
    if (threadIdx.x == 0) {
        counts[0] = n_surv; counts[1] = n_split_src; counts[2] = n_dup_src;
        counts[3] = n_surv + n_split * n_split_src + n_dup_src;
        counts[4] = n_below;
    }
}

// ranks [3][N]: exclusive counts of KEEP / EMIT_SPLIT / EMIT_DUP before each Gaussian
__global__ __launch_bounds__(256) void k_refine_ranks(int64_t N, int64_t nblk, const uint32_t *__restrict__ action, const int32_t *__restrict__ block_offs,
                                                      int32_t *__restrict__ ranks)
{
    __shared__ int32_t wcnt[3][4];
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const uint32_t act = i < N ? action[i] : 0u;
    const uint64_t b0 = __ballot((act & GC_REFINE_KEEP) != 0), b1 = __ballot((act & GC_REFINE_EMIT_SPLIT) != 0), b2 = __ballot((act & GC_REFINE_EMIT_DUP) != 0);
    if ((threadIdx.x & 63) == 0) { const int w = threadIdx.x >> 6; wcnt[0][w] = __popcll(b0); wcnt[1][w] = __popcll(b1); wcnt[2][w] = __popcll(b2); }
    __syncthreads();
    if (i >= N) return;
    ranks[i] = ballot_rank(block_offs[blockIdx.x], b0, wcnt[0]);
    ranks[N + i] = ballot_rank(block_offs[nblk + blockIdx.x], b1, wcnt[1]);
    ranks[2 * N + i] = ballot_rank(block_offs[2 * nblk + blockIdx.x], b2, wcnt[2]);
}

// output rows of one source Gaussian's children: [k] the k-th split child, [4] the duplicate; bit j of mask: emitted
struct Children { int row[5]; uint32_t mask; };

// one contiguous span of output rows of features_rest (or of one of its moments): row r of the span is source row list[r] of the LDS block
template <int R>
__device__ __forceinline__ void write_span(float *__restrict__ dst, int64_t first_row, int n, int64_t n_out, const float *srest, const uint16_t *list,
                                           bool zero)
{
    if (n <= 0 || first_row < 0 || first_row + n > n_out) return;          // (rows outside the caller's buffers are never written)
    if constexpr (R > 0) {
        float *o = dst + first_row * R;
        for (int e = threadIdx.x; e < n * R; e += BLK) {
            const int r = e / R, c = e - r * R;
            o[e] = zero ? 0.f : srest[(int)list[r] * R + c];
        }
    }
}

template <int R>
__global__ __launch_bounds__(256) void k_refine_apply(int64_t N, int n_split, int64_t n_surv, int64_t n_split_src, int64_t n_out,
                                                      const uint32_t *__restrict__ action, const int32_t *__restrict__ ranks,
                                                      const float *__restrict__ samples, ConstRows in, Rows out)
{
    __shared__ __attribute__((aligned(16))) float srest[R > 0 ? BLK * R : 4];
    __shared__ uint16_t list[3][BLK];
    __shared__ int32_t first[3], count[3];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * BLK, i = i0 + tid;
    const int nhere = (int)(N - i0 < BLK ? N - i0 : BLK);
    const int64_t dup_base = n_surv + (int64_t)n_split * n_split_src;
    uint32_t act = 0;
    Children ch = {{0, 0, 0, 0, 0}, 0};
    int row = 0;
    bool keep = false;
    if (i < N) {
        act = action[i];
        const int32_t r0 = ranks[i], r1 = ranks[N + i], r2 = ranks[2 * N + i];
        keep = (act & GC_REFINE_KEEP) != 0 && r0 < n_out;
        row = r0;
#pragma unroll
        for (int k = 0; k < GC_REFINE_MAX_SPLIT; ++k) {
            const int64_t r = n_surv + (int64_t)k * n_split_src + r1;
            if ((act & GC_REFINE_EMIT_SPLIT) && k < n_split && r1 < n_split_src && r < n_out) { ch.row[k] = (int)r; ch.mask |= 1u << k; }
        }
        if ((act & GC_REFINE_EMIT_DUP) && dup_base + r2 < n_out) { ch.row[4] = (int)(dup_base + r2); ch.mask |= 16u; }
        // ---- the five narrow tensors, per lane
        const Narrow src = load_narrow(in, 0, i);
        if (keep) store_narrow(out, 0, row, src);
        if (ch.mask & 15u) {
            // child k: mean + Rot(q / |q|) (exp(scales) * z_k), scales - log 1.6, the rest unchanged.  The offset is formed in double and
            // rounded once: a few dozen operations on the ~5 % of lanes that split, invisible next to the 1.4 KB the lane moves.
            const Rot64 rot(src.v[QUAT_AT], src.v[QUAT_AT + 1], src.v[QUAT_AT + 2], src.v[QUAT_AT + 3]);
            const double e0 = exp((double)src.v[SCALE_AT]), e1 = exp((double)src.v[SCALE_AT + 1]), e2 = exp((double)src.v[SCALE_AT + 2]);
            Narrow child = src;
#pragma unroll
            for (int a = 0; a < 3; ++a) child.v[SCALE_AT + a] = src.v[SCALE_AT + a] - LOG_SIZE_FAC;
#pragma unroll
            for (int k = 0; k < GC_REFINE_MAX_SPLIT; ++k) {
                if (!(ch.mask >> k & 1u)) continue;
                const int64_t r = ch.row[k], srow = r - n_surv;            // samples row = k * n_split_src + split rank
                const Vec64 d = rot.mul(e0 * (double)samples[3 * srow], e1 * (double)samples[3 * srow + 1], e2 * (double)samples[3 * srow + 2]);
                child.v[MEAN_AT] = (float)((double)src.v[MEAN_AT] + d.x);
                child.v[MEAN_AT + 1] = (float)((double)src.v[MEAN_AT + 1] + d.y);
                child.v[MEAN_AT + 2] = (float)((double)src.v[MEAN_AT + 2] + d.z);
                store_narrow(out, 0, r, child);
            }
        }
        if (ch.mask & 16u) store_narrow(out, 0, ch.row[4], src);
        // the moments of the narrow tensors: the survivor's rows are copied, every child row is zero
        if (keep) { store_narrow(out, 1, row, load_narrow(in, 1, i)); store_narrow(out, 2, row, load_narrow(in, 2, i)); }
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (ch.mask >> j & 1u) zero_narrow_moments(out, ch.row[j]);
        // ---- features_rest: this workgroup's members of each output span, in index order
        if (R > 0) {
            const int32_t f0 = ranks[i0], f1 = ranks[N + i0], f2 = ranks[2 * N + i0];       // ranks of the workgroup's first Gaussian
            const bool k0 = (act & GC_REFINE_KEEP) != 0, k1 = (act & GC_REFINE_EMIT_SPLIT) != 0, k2 = (act & GC_REFINE_EMIT_DUP) != 0;
            if (k0 && (unsigned)(r0 - f0) < (unsigned)BLK) list[0][r0 - f0] = (uint16_t)tid;
            if (k1 && (unsigned)(r1 - f1) < (unsigned)BLK) list[1][r1 - f1] = (uint16_t)tid;
            if (k2 && (unsigned)(r2 - f2) < (unsigned)BLK) list[2][r2 - f2] = (uint16_t)tid;
            if (tid == nhere - 1) {
                first[0] = f0; first[1] = f1; first[2] = f2;
                count[0] = r0 - f0 + (k0 ? 1 : 0); count[1] = r1 - f1 + (k1 ? 1 : 0); count[2] = r2 - f2 + (k2 ? 1 : 0);
            }
        }
    }
    if (R == 0) return;
#pragma unroll 1
    for (int m = 0; m < 3; ++m) {
        const float *src = in.t[m][5];
        float *dst = out.t[m][5];
        if (!src || !dst) continue;                                   // (kernel arguments: uniform)
        __syncthreads();                                              // the lists (m = 0) / the previous tensor's spans are done with LDS
        const int cnt4 = nhere * R / 4;                               // i0 * R * 4 bytes = 256 * R * 4 * blockIdx: 16-byte aligned
        const float *blk = src + i0 * R;
        for (int j = tid; j < cnt4; j += BLK) reinterpret_cast<float4 *>(srest)[j] = reinterpret_cast<const float4 *>(blk)[j];
        for (int j = cnt4 * 4 + tid; j < nhere * R; j += BLK) srest[j] = blk[j];
        __syncthreads();
        const int n0 = count[0] < BLK ? count[0] : BLK, n1 = count[1] < BLK ? count[1] : BLK, n2 = count[2] < BLK ? count[2] : BLK;
        write_span<R>(dst, first[0], n0, n_out, srest, list[0], false);
        for (int k = 0; k < n_split; ++k) write_span<R>(dst, n_surv + (int64_t)k * n_split_src + first[1], n1, n_out, srest, list[1], m > 0);
        write_span<R>(dst, dup_base + first[2], n2, n_out, srest, list[2], m > 0);
    }
}

__global__ __launch_bounds__(256) void k_refine_reset_opacity(int64_t N, float reset_logit, float *__restrict__ op, float *__restrict__ m,
                                                              float *__restrict__ v)
{
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= N) return;
    const float o = op[i];
    if (o > reset_logit) op[i] = reset_logit;          // (NaN stays NaN, as torch.clamp leaves it)
    if (m) m[i] = 0.f;
    if (v) v[i] = 0.f;
}

}  // namespace

extern "C" {

/* Statistics of splatfacto's after_train for C views of one scene; see the header. */
int gc_refine_accumulate_views(int64_t N, int C, const float *xys_grad, const int32_t *radii, float inv_max_dim, float *grad_norm_sum,
                               float *vis_count, float *max_2dsize, void *stream)
{
    GC_REQUIRE(N >= 0 && C >= 1, "bad arguments");
    GC_REQUIRE(fits_i32(N * 2 * (int64_t)C), "C * N * 2 must be < 2^31 elements");
    if (N == 0) return GC_OK;
    GC_REQUIRE(xys_grad && radii && grad_norm_sum && vis_count && max_2dsize, "null argument");
    hipLaunchKernelGGL(k_refine_accumulate, dim3(gc::cdiv(N, BLK)), dim3(BLK), 0, gc::S(stream), N, C, xys_grad, radii, inv_max_dim,
                       grad_norm_sum, vis_count, max_2dsize);
    return gc::check_launch("gc_refine_accumulate_views");
}

size_t gc_refine_plan_workspace_bytes(int64_t N) { return sizeof(int32_t) * 4 * (size_t)(N > 0 ? (N + BLK - 1) / BLK : 1); }

int gc_refine_plan(int64_t N, const float *log_scales, const float *opacity_logits, const float *grad_norm_sum, const float *vis_count,
                   const float *max_2dsize, int densify, int n_split_samples, float max_dim, float densify_grad_thresh,
                   float densify_size_thresh, int split_by_screen, float split_screen_size, float cull_alpha_thresh, int cull_by_scale,
                   float cull_scale_thresh, int cull_by_screen, float cull_screen_size, uint32_t *action, int32_t *ranks, int32_t *counts,
                   void *workspace, size_t workspace_bytes, void *stream)
{
    GC_REQUIRE(N >= 0, "bad arguments");
    GC_REQUIRE(n_split_samples >= 1 && n_split_samples <= GC_REFINE_MAX_SPLIT, "n_split_samples must be 1 .. 4");
    GC_REQUIRE(fits_i32(N * MAX_REST * (int64_t)(n_split_samples + 2)), "N * 45 * (n_split_samples + 2) must be < 2^31 elements");
    if (N == 0) return GC_OK;
    GC_REQUIRE(log_scales && opacity_logits && action && ranks && counts && workspace, "null argument");
    GC_REQUIRE(!densify || (grad_norm_sum && vis_count), "densify needs the gradient statistics");
    GC_REQUIRE(!((densify && split_by_screen) || cull_by_screen) || max_2dsize, "the screen-size tests need max_2dsize");
    if (workspace_bytes < gc_refine_plan_workspace_bytes(N)) { gc::set_error("gc_refine_plan: workspace too small"); return GC_ENOSPC; }
    const int64_t nblk = (N + BLK - 1) / BLK;
    PlanArgs a;
    a.densify = densify != 0; a.n_split = n_split_samples; a.split_by_screen = split_by_screen != 0; a.cull_by_scale = cull_by_scale != 0;
    a.cull_by_screen = cull_by_screen != 0; a.max_dim = max_dim; a.densify_grad_thresh = densify_grad_thresh;
    a.densify_size_thresh = densify_size_thresh; a.split_screen_size = split_screen_size; a.cull_alpha_thresh = cull_alpha_thresh;
    a.cull_scale_thresh = cull_scale_thresh; a.cull_screen_size = cull_screen_size;
    int32_t *sums = (int32_t *)workspace;
    hipStream_t s = gc::S(stream);
    hipLaunchKernelGGL(k_refine_decide, dim3((unsigned)nblk), dim3(BLK), 0, s, N, nblk, log_scales, opacity_logits, grad_norm_sum, vis_count,
                       max_2dsize, a, action, sums);
    hipLaunchKernelGGL(k_refine_scan_blocks, dim3(1), dim3(256), 0, s, nblk, n_split_samples, sums, counts);
    hipLaunchKernelGGL(k_refine_ranks, dim3((unsigned)nblk), dim3(BLK), 0, s, N, nblk, (const uint32_t *)action, (const int32_t *)sums, ranks);
    return gc::check_launch("gc_refine_plan");
}

int gc_refine_apply(int64_t N, int n_split_samples, int rest_floats, int64_t n_survivors, int64_t n_split_src, int64_t n_dup_src,
                    const uint32_t *action, const int32_t *ranks, const float *samples, const float *const *params,
                    const float *const *exp_avg, const float *const *exp_avg_sq, float *const *out_params, float *const *out_exp_avg,
                    float *const *out_exp_avg_sq, void *stream)
{
    GC_REQUIRE(N >= 0, "bad arguments");
    GC_REQUIRE(n_split_samples >= 1 && n_split_samples <= GC_REFINE_MAX_SPLIT, "n_split_samples must be 1 .. 4");
    GC_REQUIRE(rest_floats == 0 || rest_floats == 9 || rest_floats == 24 || rest_floats == 45, "features_rest must hold 0, 9, 24 or 45 floats per Gaussian");
    GC_REQUIRE(n_survivors >= 0 && n_survivors <= N && n_split_src >= 0 && n_split_src <= N && n_dup_src >= 0 && n_dup_src <= N, "bad counts");
    const int64_t n_out = n_survivors + n_split_samples * n_split_src + n_dup_src;
    GC_REQUIRE(fits_i32(N * MAX_REST) && fits_i32(n_out * MAX_REST), "N * 45 and n_out * 45 must be < 2^31 elements");
    if (N == 0 || n_out == 0) return GC_OK;
    GC_REQUIRE(action && ranks && params && out_params, "null argument");
    GC_REQUIRE(n_split_src == 0 || samples, "split children need samples");
    ConstRows in;
    Rows out;
    GC_REQUIRE(fill_rows(in, rest_floats, params, exp_avg, exp_avg_sq) && fill_rows(out, rest_floats, out_params, out_exp_avg, out_exp_avg_sq),
               "null parameter tensor");
    for (int t = 0; t < 6; ++t)
        GC_REQUIRE((in.t[1][t] != nullptr) == (out.t[1][t] != nullptr) && (in.t[2][t] != nullptr) == (out.t[2][t] != nullptr),
                   "a moment needs both its input and its output");
    with_rest_floats(rest_floats, [&](auto R) {
        hipLaunchKernelGGL(k_refine_apply<decltype(R)::value>, dim3(gc::cdiv(N, BLK)), dim3(BLK), 0, gc::S(stream), N, n_split_samples,
                           n_survivors, n_split_src, n_out, action, ranks, samples, in, out);
    });
    return gc::check_launch("gc_refine_apply");
}

int gc_refine_reset_opacity(int64_t N, float reset_logit, float *opacities, float *exp_avg, float *exp_avg_sq, void *stream)
{
    GC_REQUIRE(N >= 0, "bad arguments");
    GC_REQUIRE(fits_i32(N), "N must be < 2^31 elements");
    if (N == 0) return GC_OK;
    GC_REQUIRE(opacities, "null argument");
    hipLaunchKernelGGL(k_refine_reset_opacity, dim3(gc::cdiv(N, BLK)), dim3(BLK), 0, gc::S(stream), N, reset_logit, opacities, exp_avg, exp_avg_sq);
    return gc::check_launch("gc_refine_reset_opacity");
}

}  // extern "C"

// raster_trace.hip -- edit-region tracing (include/gaussctrl_trace.h) for gfx950: the compositing weights every Gaussian receives from
// masked and from all pixels, and the row selection made from them.
//
// k_trace_mask is a compositing-class kernel built from the pieces of raster_tile.h: one 16x16 tile per 256-lane workgroup, one wave per
// 8x8 pixel block, the depth-sorted list staged through LDS in batches of 256 splats with the exact per-block culling mask, the scalar
// ballot walk of k_rasterize_nd_fwd with its two early-outs, fwd_step for alpha / T / stop (so vis is the forward's, bit for bit), and
// the reduction of k_rasterize_nd_bwd for the two partials (vis * mask, vis): row_sum, lane column picks its partial, xor_rows_sum, two
// lanes add into the per-batch LDS accumulator; after a batch the staging lane of each splat flushes at most one hardware float atomic
// per array -- once per (tile, splat).  It owns only its memory schedule: SplatA + SplatQ + sG[2][256] in LDS, no image, no colours, no
// final_Ts / final_index.  Algorithmic bytes: M x 28 (id + geometry) + HW x 4 (mask) + N x 8 (the two sums).
#include "raster_tile.h"
#include "../../include/gaussctrl_trace.h"

namespace {

struct SplatQ { float cxy, cyy; };

__global__ __launch_bounds__(BLOCK) void k_trace_mask(int H, int W, int tiles_x, const int32_t *__restrict__ ids_sorted,
                                                      const int32_t *__restrict__ tile_bins, const float *__restrict__ xys,
                                                      const float *__restrict__ conics, const float *__restrict__ opacities,
                                                      const float *__restrict__ masks, float *__restrict__ w_in, float *__restrict__ w_all, CV cv)
{
    {
        const int64_t v = blockIdx.z;
        ids_sorted += v * cv.m; tile_bins += v * 2 * cv.tiles; xys += v * 2 * cv.n; conics += v * 3 * cv.n; opacities += v * cv.n_op;
        masks += v * (int64_t)H * W;
    }
    __shared__ SplatA sA[BLOCK];
    __shared__ SplatQ sQ[BLOCK];
    __shared__ float sG[2 * BLOCK];
    __shared__ unsigned char sMask[BLOCK];
    const TileCtx tc = tile_ctx(H, W, tiles_x, tile_bins);
    const int tid = tc.tid, lane = tc.lane, wid = tc.wid, end = tc.end;
    bool done = !tc.inside;                                              // pixels outside the image: done from the start, mask 0
    float T = 1.f;
    const float mv = tc.inside ? masks[tc.i * W + tc.j] : 0.f;
    sG[tid] = 0.f; sG[BLOCK + tid] = 0.f;                                // (the first barrier of the loop orders this before the walk)
    const bool col1 = (lane & 15) == 1;
    for (int bs = tc.start; bs < end; bs += BLOCK) {
        if (__syncthreads_and(done)) break;
        const int idx = bs + tid;
        unsigned mk = 0;
        int gid = -1;
        if (idx < end) {
            gid = ids_sorted[idx];
            const Geom s = load_geometry((int64_t)gid, xys, conics, opacities);
            sA[tid] = s.a;
            sQ[tid] = {s.cxy, s.cyy};
            mk = block_mask(s, tc.tx0, tc.ty0);
        }
        sMask[tid] = (unsigned char)mk;
        __syncthreads();
        const int n = min(BLOCK, end - bs);
        bool wave_done = __all(done);                                    // a finished wave only helps staging
        for (int c = 0; c * 64 < n && !wave_done; ++c) {
            unsigned long long bal = block_ballot(sMask, c, lane, wid);
            while (bal) {                                                // scalar walk over the splats that can touch this block
                const int t = c * 64 + __builtin_ctzll(bal);
                bal &= bal - 1;
                const SplatQ q = sQ[t];
                const FwdStep f = fwd_step(sA[t], q.cxy, q.cyy, tc.px, tc.py, bs + t, T, 0, done);
                T = f.T; done = f.done;
                if (__any(f.vis != 0.f)) {                               // wave-uniform: every lane takes part in the reduction
                    const float g_in = row_sum(f.vis * mv), g_all = row_sum(f.vis);
                    float x = col1 ? g_all : g_in;                      // lane column c keeps partial c
                    x = xor_rows_sum(x);
                    if (lane < 2) __hip_atomic_fetch_add(&sG[lane * BLOCK + t], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if (__all(done)) { wave_done = true; break; }
            }
        }
        __syncthreads();
        if (gid >= 0) {                                                  // flush: at most one atomic per array and (tile, splat)
            const auto [v, any] = take_partials<2>(sG, tid);
            if (any) {
                if (v[0] != 0.f) unsafeAtomicAdd(w_in + gid, v[0]);
                if (v[1] != 0.f) unsafeAtomicAdd(w_all + gid, v[1]);
            }
        }
        // the next staging pass overwrites sA / sQ / sMask: every wave has left the walk (barrier above); sG slots are private to their
        // staging lane until the next barrier
    }
}

// one lane per Gaussian; the count leaves through a wave ballot and one integer atomic per wave
__global__ __launch_bounds__(256) void k_trace_select(int64_t N, const float *__restrict__ w_in, const float *__restrict__ w_all,
                                                      float ratio_thresh, float min_weight, uint8_t *__restrict__ select,
                                                      int32_t *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool s = false;
    if (i < N) {
        const float a = w_all[i];
        s = a != 0.f && a > min_weight && w_in[i] > ratio_thresh * a;
        select[i] = s ? 1 : 0;
    }
    const unsigned long long bal = __ballot(s);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (int32_t)__popcll(bal));
}

}  // namespace

extern "C" {

int gc_trace_mask_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int img_h, int img_w, int tiles_x, int tiles_y,
                        const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                        const float *opacities, const float *masks, float *w_in, float *w_all, void *stream)
{
    GC_REQUIRE(C >= 1 && C <= 65535 && N >= 0 && M_cap >= 0, "bad arguments");
    if (const int rc = check_tiles(__func__, img_h, img_w, tiles_x, tiles_y)) return rc;
    if (N == 0) return GC_OK;
    GC_REQUIRE(masks && w_in && w_all, "masks, w_in and w_all are required");
    GC_REQUIRE(gaussian_ids_sorted && tile_bins && xys && conics && opacities, "null argument");
    hipLaunchKernelGGL(k_trace_mask, dim3(tiles_x, tiles_y, C), dim3(BLOCK), 0, gc::S(stream), img_h, img_w, tiles_x, gaussian_ids_sorted, tile_bins,
                       xys, conics, opacities, masks, w_in, w_all, view_strides(N, M_cap, shared_opacities, 1, tiles_x * tiles_y));
    return gc::check_launch("gc_trace_mask_views");
}

int gc_trace_select(int64_t N, const float *w_in, const float *w_all, float ratio_thresh, float min_weight, uint8_t *select, int32_t *count,
                    void *stream)
{
    GC_REQUIRE(N >= 0 && count, "bad arguments");
    GC_REQUIRE(ratio_thresh == ratio_thresh && min_weight == min_weight, "ratio_thresh and min_weight must not be NaN");
    GC_REQUIRE(N == 0 || (w_in && w_all && select), "null argument");
    GC_REQUIRE(N < (1ll << 31) * 256, "N too large");
    if (hipMemsetAsync(count, 0, sizeof(int32_t), gc::S(stream)) != hipSuccess) return GC_ELAUNCH;
    if (N == 0) return GC_OK;
    hipLaunchKernelGGL(k_trace_select, dim3(gc::cdiv(N, 256)), dim3(256), 0, gc::S(stream), N, w_in, w_all, ratio_thresh, min_weight, select,
                       count);
    return gc::check_launch("gc_trace_select");
}

}  // extern "C"

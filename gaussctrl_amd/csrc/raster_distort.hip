// raster_distort.hip -- distortion loss (include/ext/gaussctrl_distort.h) for gfx950: per pixel, the weighted spread in (mapped) depth of the
// splats composited there, and its backward to xys / conics / opacities / depths.
//
// Two compositing-class kernels built from the pieces of raster_tile.h, which own only their memory schedule:
//   k_distort_fwd  the shape of k_trace_mask: one 16x16 tile per 256-lane workgroup, one wave per 8x8 pixel block, the depth-sorted list staged
//                  through LDS in batches of 256 records (SplatA + SplatD: the conic's other two entries and the mapped depth t) with the exact
//                  per-block culling mask, the scalar ballot walk with both early-outs, fwd_step for alpha / T / stop (so w = vis is the
//                  forward's, bit for bit).  Per pixel T, B = sum w t and D by value; no image, no colours, no final_Ts / final_index.
//   k_distort_bwd  the shape of k_rasterize_nd_bwd: bwd_pixel, bwd_walk_max, bwd_batch, pair_eval, pair_weight, geom_grad; back to front from
//                  final_Ts / final_index with the suffix sums S, Bs, R per pixel by value, B_i = wt - Bs_i - w_i t_i.  Seven partials per splat
//                  (cxx cxy cyy, x y, o, depth): row_sum, lane column picks its partial, xor_rows_sum, seven lanes add into the per-batch LDS
//                  accumulator; after a batch the staging lane of each splat flushes one hardware float atomic per partial -- once per
//                  (tile, splat).  It ADDS into the four gradient arrays.
// Algorithmic bytes: M x 32 (id + geometry + depth) + HW x 8 (forward: two images written) / HW x 16 (backward: four read) + N x 28 (gradients).
#include <math.h>

#include "raster_tile.h"
#include "../../include/ext/gaussctrl_distort.h"

namespace {

struct SplatD { float cxy, cyy, t, dm; };      // dm = m'(z): what v_depths takes of dD/dt (forward: not read)

// depth_map 0: m(z) = z; 1: m(z) = far (z - near) / ((far - near) z), the operations in the header's order
struct DepthMap { int mode; float nearp, farp; };
struct MappedT { float t, dm; };
__device__ __forceinline__ MappedT map_depth(const DepthMap m, float z)
{
    if (m.mode == 0) return {z, 1.f};
    const float span = m.farp - m.nearp;
    return {(m.farp * (z - m.nearp)) / (span * z), (m.farp * m.nearp) / (span * (z * z))};
}

__global__ __launch_bounds__(BLOCK) void k_distort_fwd(int H, int W, int tiles_x, const int32_t *__restrict__ ids_sorted,
                                                       const int32_t *__restrict__ tile_bins, const float *__restrict__ xys,
                                                       const float *__restrict__ conics, const float *__restrict__ opacities,
                                                       const float *__restrict__ depths, DepthMap dmap, float *__restrict__ distort,
                                                       float *__restrict__ wt, CV cv)
{
    {
        const int64_t v = blockIdx.z, hw = (int64_t)H * W;
        ids_sorted += v * cv.m; tile_bins += v * 2 * cv.tiles; xys += v * 2 * cv.n; conics += v * 3 * cv.n; opacities += v * cv.n_op;
        depths += v * cv.n; distort += v * hw; wt += v * hw;
    }
    __shared__ SplatA sA[BLOCK];
    __shared__ SplatD sD[BLOCK];
    __shared__ unsigned char sMask[BLOCK];
    const TileCtx tc = tile_ctx(H, W, tiles_x, tile_bins);
    const int tid = tc.tid, lane = tc.lane, wid = tc.wid, end = tc.end;
    bool done = !tc.inside;                                              // pixels outside the image: done from the start
    float T = 1.f, B = 0.f, D = 0.f;
    for (int bs = tc.start; bs < end; bs += BLOCK) {
        if (__syncthreads_and(done)) break;
        const int idx = bs + tid;
        unsigned mk = 0;
        if (idx < end) {
            const int gid = ids_sorted[idx];
            const Geom s = load_geometry((int64_t)gid, xys, conics, opacities);
            const MappedT mt = map_depth(dmap, depths[gid]);
            sA[tid] = s.a;
            sD[tid] = {s.cxy, s.cyy, mt.t, mt.dm};
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
                const SplatD q = sD[t];
                const float A = 1.f - T;                                 // the weight in front of this entry
                const FwdStep f = fwd_step(sA[t], q.cxy, q.cyy, tc.px, tc.py, bs + t, T, 0, done);
                D += 2.f * f.vis * (q.t * A - B);                        // vis == 0 where the entry is not composited
                B += f.vis * q.t;
                T = f.T; done = f.done;
                if (__all(done)) { wave_done = true; break; }
            }
        }
        // the next staging pass overwrites sA / sD / sMask: the barrier at the head of the loop is passed only after every wave left the walk
    }
    if (tc.inside) {
        const int pix = tc.i * W + tc.j;
        distort[pix] = D;
        wt[pix] = B;
    }
}

__global__ __launch_bounds__(BLOCK) void k_distort_bwd(int H, int W, int tiles_x, const int32_t *__restrict__ ids_sorted,
                                                       const int32_t *__restrict__ tile_bins, const float *__restrict__ xys,
                                                       const float *__restrict__ conics, const float *__restrict__ opacities,
                                                       const float *__restrict__ depths, DepthMap dmap,
                                                       const float *__restrict__ final_Ts, const int32_t *__restrict__ final_index,
                                                       const float *__restrict__ wt, const float *__restrict__ v_distort,
                                                       float *__restrict__ v_xy, float *__restrict__ v_conic, float *__restrict__ v_opacity,
                                                       float *__restrict__ v_depths, CV cv)
{
    constexpr int NQ = 7;                                               // partials: cxx cxy cyy, x y, opacity, depth
    {
        const int64_t v = blockIdx.z, hw = (int64_t)H * W;
        ids_sorted += v * cv.m; tile_bins += v * 2 * cv.tiles; xys += v * 2 * cv.n; conics += v * 3 * cv.n; opacities += v * cv.n_op;
        depths += v * cv.n; final_Ts += v * hw; final_index += v * hw; wt += v * hw; v_distort += v * hw;
        v_xy += v * 2 * cv.n; v_conic += v * 3 * cv.n; v_opacity += v * cv.n; v_depths += v * cv.n;
    }
    __shared__ SplatA sA[BLOCK];
    __shared__ SplatD sD[BLOCK];
    __shared__ float sG[BLOCK * NQ];
    __shared__ unsigned char sMask[BLOCK];
    __shared__ int sMax[4];
    const TileCtx tc = tile_ctx(H, W, tiles_x, tile_bins);
    const int tid = tc.tid, lane = tc.lane, wid = tc.wid, start = tc.start;
    if (tc.end <= start) return;
    const BwdPixel fp = bwd_pixel(tc, W, final_Ts, final_index);
    const float wtp = tc.inside ? wt[fp.pix] : 0.f;
    const float g = tc.inside ? v_distort[fp.pix] : 0.f;
    float T = fp.T_final;
    float S = 0.f, Bs = 0.f, R = 0.f;                                    // over the entries behind the current one
    const WalkMax wm = bwd_walk_max<NQ>(fp.bin_final, tid, lane, wid, sG, sMax);
    if (wm.kmax < start) return;
    const int col16 = lane & 15;
    for (int batch_end = wm.kmax; batch_end >= start; batch_end -= BLOCK) {
        const int idx = batch_end - tid;
        int gid = -1;
        unsigned mk = 0;
        if (idx >= start) {
            gid = ids_sorted[idx];
            const Geom s = load_geometry((int64_t)gid, xys, conics, opacities);
            const MappedT mt = map_depth(dmap, depths[gid]);
            sA[tid] = s.a;
            sD[tid] = {s.cxy, s.cyy, mt.t, mt.dm};
            mk = block_mask(s, tc.tx0, tc.ty0);
        }
        sMask[tid] = (unsigned char)mk;
        __syncthreads();
        const BwdBatch bt = bwd_batch(batch_end, start, wm.wmax);
        for (int c = bt.t0 >> 6; c * 64 < bt.n; ++c) {
            unsigned long long bal = block_ballot_from(sMask, c, lane, wid, bt.t0);
            while (bal) {
                const int t = c * 64 + __builtin_ctzll(bal);
                bal &= bal - 1;
                const SplatA a = sA[t];
                const SplatD q = sD[t];
                const Pair pr = pair_eval(a, q.cxy, q.cyy, tc.px, tc.py, batch_end - t, fp.bin_final);
                if (!__any(pr.valid)) continue;
                float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f, p4 = 0.f, p5 = 0.f, p6 = 0.f;
                if (pr.valid) {
                    const PairT w = pair_weight(pr.alpha, T);
                    T = w.T;                                             // the transmittance in front of this entry
                    const float A = 1.f - T;
                    const float wti = w.fac * q.t;
                    const float B = (wtp - Bs) - wti;
                    const float dw = 2.f * ((q.t * A - B) + (Bs - q.t * S));
                    const float dt = 2.f * w.fac * (A - S);
                    const float da = T * dw - R * w.ra;
                    S += w.fac; Bs += wti; R += w.fac * dw;
                    const GeomGrad gg = geom_grad(g * da, pr, a, q.cxy, q.cyy);
                    p0 = gg.cxx; p1 = gg.cxy; p2 = gg.cyy; p3 = gg.x; p4 = gg.y; p5 = gg.o;
                    p6 = g * dt * q.dm;
                }
                p0 = row_sum(p0); p1 = row_sum(p1); p2 = row_sum(p2); p3 = row_sum(p3); p4 = row_sum(p4); p5 = row_sum(p5); p6 = row_sum(p6);
                float x = p0;                                            // lane column c keeps partial c
                x = col16 == 1 ? p1 : x; x = col16 == 2 ? p2 : x; x = col16 == 3 ? p3 : x;
                x = col16 == 4 ? p4 : x; x = col16 == 5 ? p5 : x; x = col16 == 6 ? p6 : x;
                x = xor_rows_sum(x);
                if (lane < NQ) __hip_atomic_fetch_add(&sG[lane * BLOCK + t], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        if (gid >= 0) {                                                  // flush: one atomic per partial and (tile, splat) touched at all
            const auto [v, any] = take_partials<NQ>(sG, tid);
            if (any) {
                unsafeAtomicAdd(v_conic + 3 * (int64_t)gid, v[0]);
                unsafeAtomicAdd(v_conic + 3 * (int64_t)gid + 1, v[1]);
                unsafeAtomicAdd(v_conic + 3 * (int64_t)gid + 2, v[2]);
                unsafeAtomicAdd(v_xy + 2 * (int64_t)gid, v[3]);
                unsafeAtomicAdd(v_xy + 2 * (int64_t)gid + 1, v[4]);
                unsafeAtomicAdd(v_opacity + gid, v[5]);
                unsafeAtomicAdd(v_depths + gid, v[6]);
            }
        }
        // the next staging pass overwrites sA / sD / sMask: every wave has left the walk (barrier above); sG slots are private to their
        // staging lane until the next barrier
    }
}

// the checks both entry points share; GC_OK = go on
int check_distort(const char *what, int C, int64_t N, int64_t M_cap, int H, int W, int tiles_x, int tiles_y, int depth_map, float nearp, float farp)
{
    if (!(C >= 1 && C <= 65535 && N >= 0 && M_cap >= 0)) { gc::set_error("%s: bad arguments", what); return GC_EINVAL; }
    if (const int rc = check_tiles(what, H, W, tiles_x, tiles_y)) return rc;
    if (depth_map != 0 && depth_map != 1) { gc::set_error("%s: depth_map must be 0 (linear) or 1 (ndc)", what); return GC_EINVAL; }
    if (depth_map == 1 && !(nearp > 0.f && nearp < farp && farp < INFINITY)) {       // a NaN fails every comparison
        gc::set_error("%s: depth_map 1 needs 0 < near_plane < far_plane", what);
        return GC_EINVAL;
    }
    return GC_OK;
}

}  // namespace

extern "C" {

int gcx_distort_fwd_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int img_h, int img_w, int tiles_x, int tiles_y,
                          const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                          const float *opacities, const float *depths, int depth_map, float near_plane, float far_plane,
                          float *distort, float *wt, void *stream)
{
    if (const int rc = check_distort(__func__, C, N, M_cap, img_h, img_w, tiles_x, tiles_y, depth_map, near_plane, far_plane)) return rc;
    if (N == 0) {                                                        // nothing is composited anywhere
        const size_t bytes = sizeof(float) * (size_t)C * img_h * img_w;
        if (distort && hipMemsetAsync(distort, 0, bytes, gc::S(stream)) != hipSuccess) return GC_ELAUNCH;
        if (wt && hipMemsetAsync(wt, 0, bytes, gc::S(stream)) != hipSuccess) return GC_ELAUNCH;
        return GC_OK;
    }
    GC_REQUIRE(gaussian_ids_sorted && tile_bins && xys && conics && opacities && depths && distort && wt, "null argument");
    hipLaunchKernelGGL(k_distort_fwd, dim3(tiles_x, tiles_y, C), dim3(BLOCK), 0, gc::S(stream), img_h, img_w, tiles_x, gaussian_ids_sorted, tile_bins,
                       xys, conics, opacities, depths, DepthMap{depth_map, near_plane, far_plane}, distort, wt,
                       view_strides(N, M_cap, shared_opacities, 1, tiles_x * tiles_y));
    return gc::check_launch("gcx_distort_fwd_views");
}

int gcx_distort_bwd_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int img_h, int img_w, int tiles_x, int tiles_y,
                          const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                          const float *opacities, const float *depths, int depth_map, float near_plane, float far_plane,
                          const float *final_Ts, const int32_t *final_index, const float *wt, const float *v_distort, float *v_xy,
                          float *v_conic, float *v_opacity, float *v_depths, void *stream)
{
    if (const int rc = check_distort(__func__, C, N, M_cap, img_h, img_w, tiles_x, tiles_y, depth_map, near_plane, far_plane)) return rc;
    if (N == 0) return GC_OK;
    GC_REQUIRE(gaussian_ids_sorted && tile_bins && xys && conics && opacities && depths, "null argument");
    GC_REQUIRE(final_Ts && final_index && wt && v_distort && v_xy && v_conic && v_opacity && v_depths, "null argument");
    hipLaunchKernelGGL(k_distort_bwd, dim3(tiles_x, tiles_y, C), dim3(BLOCK), 0, gc::S(stream), img_h, img_w, tiles_x, gaussian_ids_sorted, tile_bins,
                       xys, conics, opacities, depths, DepthMap{depth_map, near_plane, far_plane}, final_Ts, final_index, wt, v_distort, v_xy,
                       v_conic, v_opacity, v_depths, view_strides(N, M_cap, shared_opacities, 1, tiles_x * tiles_y));
    return gc::check_launch("gcx_distort_bwd_views");
}

}  // extern "C"

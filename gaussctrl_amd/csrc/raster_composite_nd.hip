// raster_composite_nd.hip -- per-tile alpha compositing of colors[N][C] for any channel count C >= 1 (forward + backward) for gfx950.
//
// gsplat 0.1.3's rasterize_gaussians sends C == 3 to rasterize_forward (raster_composite.hip) and every other count to
// nd_rasterize_forward / nd_rasterize_backward: these are the latter.  Same semantics as the 3-channel kernels (SURVEY.md Appendix
// A.4 / A.5) and the same structure: one 16x16 tile per 256-lane workgroup, one wave per 8x8 pixel block, the depth-sorted list staged
// through LDS in batches of 256 splats with the exact per-block culling mask, a scalar walk over the ballot of the wave's block.
// All of that IS the 3-channel kernels' code: tile context, record staging, the forward step (alpha / T / stop), the backward prologue,
// pair step, gradient tail, batch bounds and ballots are the pieces of raster_tile.h, instantiated here with a 64-bit Gaussian index.
// final_Ts and final_index are therefore the 3-channel kernels' bit for bit.  This file owns its memory schedule: SplatQ + sCol[256][CH]
// in LDS, a plain ballot walk without prefetch, CH accumulators per pixel, CH + 6 partials in groups of 16 lane columns.
//
// Channel chunking: a launch instantiated for CH in {1, 2, 4, 8, 16, 32} covers the channels [base + z CH, base + (z + 1) CH) in
// workgroup z of grid.z.  C <= 32 is one launch with the smallest CH >= C; C > 32 is C / 32 chunks of 32 channels plus, when
// C % 32 != 0, a second launch of one chunk with the smallest CH >= C % 32.  Staged colours are zero-padded to CH; only c < C is read
// or stored.  Every chunk recomputes alpha (a handful of instructions next to CH FMAs per (pixel, splat)); only the chunk that holds
// channel 0 writes final_Ts / final_index (forward) and adds the v_out_alpha term (backward).  The geometry gradients are linear in
// v_out, so each chunk adds its own channels' share of them, background term included; v_colors columns of different chunks are
// disjoint.
//
// Limits (GC_EINVAL): C >= 1, H W C < 2^31 and (backward) N C < 2^31 elements, C / 32 < 65536 chunks.
#include <type_traits>

#include "raster_tile.h"

namespace {

constexpr int CH_MAX = 32;

struct SplatQ { float cxy, cyy; };

// colours of the n staged splats, [n][CH] row-major, channels >= nc zero: consecutive lanes write consecutive LDS words and read
// consecutive channels of one Gaussian
template <int CH>
__device__ __forceinline__ void stage_colors(float *__restrict__ sCol, const int *__restrict__ sGid, int n, int tid,
                                             const float *__restrict__ colors, int C, int cb, int nc)
{
    for (int e = tid; e < n * CH; e += BLOCK) {
        const int t = e / CH, c = e % CH;
        sCol[e] = c < nc ? colors[(int64_t)sGid[t] * C + cb + c] : 0.f;
    }
}

template <int CH>
__global__ __launch_bounds__(BLOCK) void k_rasterize_nd_fwd(int H, int W, int tiles_x, int C, int base,
                                                            const int32_t *__restrict__ ids_sorted,
                                                            const int32_t *__restrict__ tile_bins,
                                                            const float *__restrict__ xys, const float *__restrict__ conics,
                                                            const float *__restrict__ colors, const float *__restrict__ opacities,
                                                            const float *__restrict__ background, float *__restrict__ out_img,
                                                            float *__restrict__ final_Ts, int32_t *__restrict__ final_index)
{
    __shared__ SplatA sA[BLOCK];
    __shared__ SplatQ sQ[BLOCK];
    __shared__ __attribute__((aligned(16))) float sCol[BLOCK * CH];
    __shared__ int sGid[BLOCK];
    __shared__ unsigned char sMask[BLOCK];
    const int cb = base + blockIdx.z * CH, nc = min(CH, C - cb);
    const TileCtx tc = tile_ctx(H, W, tiles_x, tile_bins);
    const int tid = tc.tid, lane = tc.lane, wid = tc.wid, end = tc.end;
    bool done = !tc.inside;
    float T = 1.f;
    int last = 0;
    float acc[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) acc[k] = 0.f;
    for (int bs = tc.start; bs < end; bs += BLOCK) {
        if (__syncthreads_and(done)) break;
        const int idx = bs + tid;
        unsigned mk = 0;
        int gid = 0;
        if (idx < end) {
            gid = ids_sorted[idx];
            const Geom s = load_geometry((int64_t)gid, xys, conics, opacities);
            sA[tid] = s.a;
            sQ[tid] = {s.cxy, s.cyy};
            mk = block_mask(s, tc.tx0, tc.ty0);
        }
        sGid[tid] = gid;
        sMask[tid] = (unsigned char)mk;
        __syncthreads();
        const int n = min(BLOCK, end - bs);
        stage_colors<CH>(sCol, sGid, n, tid, colors, C, cb, nc);
        __syncthreads();
        bool wave_done = __all(done);                                // a finished wave only helps staging
        for (int c = 0; c * 64 < n && !wave_done; ++c) {
            unsigned long long bal = block_ballot(sMask, c, lane, wid);
            while (bal) {                                              // scalar walk over the splats that can touch this block
                const int t = c * 64 + __builtin_ctzll(bal);
                bal &= bal - 1;
                const SplatQ q = sQ[t];
                const FwdStep f = fwd_step(sA[t], q.cxy, q.cyy, tc.px, tc.py, bs + t, T, last, done);
                const float *col = sCol + t * CH;
#pragma unroll
                for (int k = 0; k < CH; ++k) acc[k] += col[k] * f.vis;
                T = f.T; last = f.last; done = f.done;
                if (__all(done)) { wave_done = true; break; }
            }
        }
    }
    if (tc.inside) {
        const int pix = tc.i * W + tc.j;
        if (cb == 0) {
            final_Ts[pix] = T;
            final_index[pix] = last;
        }
        float *o = out_img + (int64_t)pix * C + cb;
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (k < nc) o[k] = acc[k] + T * background[cb + k];
    }
}

// Backward.  Per (block, splat) with at least one contributing pixel: the CH + 6 partials (CH colours, conic 3, xy 2, opacity 1) are
// summed over each row of 16 lanes with DPP; then per group of 16 partials lane c of every row picks partial c, two lane-swap steps add
// the four rows and lanes 0..15 add their value into the per-batch LDS accumulator.  After a batch the staging lane of each splat
// flushes one hardware float atomic per partial -- once per (tile, splat), as in k_rasterize_bwd.
template <int CH>
__global__ __launch_bounds__(BLOCK) void k_rasterize_nd_bwd(int H, int W, int tiles_x, int C, int base,
                                                            const int32_t *__restrict__ ids_sorted,
                                                            const int32_t *__restrict__ tile_bins,
                                                            const float *__restrict__ xys, const float *__restrict__ conics,
                                                            const float *__restrict__ colors, const float *__restrict__ opacities,
                                                            const float *__restrict__ background,
                                                            const float *__restrict__ final_Ts, const int32_t *__restrict__ final_index,
                                                            const float *__restrict__ v_out, const float *__restrict__ v_out_alpha,
                                                            float *__restrict__ v_xy, float *__restrict__ v_conic,
                                                            float *__restrict__ v_colors, float *__restrict__ v_opacity)
{
    constexpr int NQ = CH + 6;                                          // partials: colours, cxx cxy cyy, x y, opacity
    __shared__ SplatA sA[BLOCK];
    __shared__ SplatQ sQ[BLOCK];
    __shared__ __attribute__((aligned(16))) float sCol[BLOCK * CH];
    __shared__ float sG[BLOCK * NQ];
    __shared__ int sGid[BLOCK];
    __shared__ unsigned char sMask[BLOCK];
    __shared__ int sMax[4];
    const int cb = base + blockIdx.z * CH, nc = min(CH, C - cb);
    const TileCtx tc = tile_ctx(H, W, tiles_x, tile_bins);
    const int tid = tc.tid, lane = tc.lane, wid = tc.wid, start = tc.start;
    const bool inside = tc.inside;
    if (tc.end <= start) return;
    const BwdPixel fp = bwd_pixel(tc, W, final_Ts, final_index);
    const int pix = fp.pix;
    const float T_final = fp.T_final;
    float T = T_final;
    float vo[CH], S[CH];
    float voa = 0.f, bgdot = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        vo[k] = inside && k < nc ? v_out[(int64_t)pix * C + cb + k] : 0.f;
        S[k] = 0.f;
        if (k < nc) bgdot += background[cb + k] * vo[k];
    }
    if (inside && cb == 0 && v_out_alpha) voa = v_out_alpha[pix];
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
            sA[tid] = s.a;
            sQ[tid] = {s.cxy, s.cyy};
            mk = block_mask(s, tc.tx0, tc.ty0);
        }
        sGid[tid] = gid;
        sMask[tid] = (unsigned char)mk;
        __syncthreads();
        const BwdBatch bt = bwd_batch(batch_end, start, wm.wmax);
        stage_colors<CH>(sCol, sGid, bt.n, tid, colors, C, cb, nc);
        __syncthreads();
        for (int c = bt.t0 >> 6; c * 64 < bt.n; ++c) {
            unsigned long long bal = block_ballot_from(sMask, c, lane, wid, bt.t0);
            while (bal) {
                const int t = c * 64 + __builtin_ctzll(bal);
                bal &= bal - 1;
                const SplatA a = sA[t];
                const SplatQ q = sQ[t];
                const Pair pr = pair_eval(a, q.cxy, q.cyy, tc.px, tc.py, batch_end - t, fp.bin_final);
                if (!__any(pr.valid)) continue;
                float g[NQ];
#pragma unroll
                for (int p = 0; p < NQ; ++p) g[p] = 0.f;
                if (pr.valid) {
                    const PairT w = pair_weight(pr.alpha, T);
                    const float ra = w.ra, fac = w.fac;
                    T = w.T;
                    const float *col = sCol + t * CH;
                    float v_alpha = 0.f;
#pragma unroll
                    for (int p = 0; p < CH; ++p) {
                        const float cp = col[p];
                        g[p] = fac * vo[p];
                        v_alpha += (cp * T - S[p] * ra) * vo[p];
                        S[p] += cp * fac;
                    }
                    v_alpha += T_final * ra * voa;
                    v_alpha += -T_final * ra * bgdot;
                    const GeomGrad gg = geom_grad(v_alpha, pr, a, q.cxy, q.cyy);
                    g[CH] = gg.cxx; g[CH + 1] = gg.cxy; g[CH + 2] = gg.cyy; g[CH + 3] = gg.x; g[CH + 4] = gg.y; g[CH + 5] = gg.o;
                }
#pragma unroll
                for (int p = 0; p < NQ; ++p) g[p] = row_sum(g[p]);
#pragma unroll
                for (int g0 = 0; g0 < NQ; g0 += 16) {
                    float x = g[g0];                                    // lane column c keeps partial g0 + c
#pragma unroll
                    for (int p = 1; p < 16 && g0 + p < NQ; ++p) x = col16 == p ? g[g0 + p] : x;
                    x = xor_rows_sum(x);
                    if (lane < min(16, NQ - g0)) __hip_atomic_fetch_add(&sG[(g0 + lane) * BLOCK + t], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        if (gid >= 0) {                                                 // flush: one atomic per partial and (tile, splat) touched at all
            const auto [v, any] = take_partials<NQ>(sG, tid);
            if (any) {
                float *vc = v_colors + (int64_t)gid * C + cb;
#pragma unroll
                for (int p = 0; p < CH; ++p)
                    if (p < nc) unsafeAtomicAdd(vc + p, v[p]);
                unsafeAtomicAdd(v_conic + 3 * (int64_t)gid, v[CH]);
                unsafeAtomicAdd(v_conic + 3 * (int64_t)gid + 1, v[CH + 1]);
                unsafeAtomicAdd(v_conic + 3 * (int64_t)gid + 2, v[CH + 2]);
                unsafeAtomicAdd(v_xy + 2 * (int64_t)gid, v[CH + 3]);
                unsafeAtomicAdd(v_xy + 2 * (int64_t)gid + 1, v[CH + 4]);
                unsafeAtomicAdd(v_opacity + gid, v[CH + 5]);
            }
        }
        // the next staging pass overwrites sA / sQ / sGid / sMask / sCol: every wave has left the walk (barrier above); sG slots are
        // private to their staging lane until the next barrier
    }
}

template <class F>
void for_ch(int c, F f)        // f(CH): CH = the smallest of {1, 2, 4, 8, 16, 32} that holds c channels
{
    if (c <= 1) f(std::integral_constant<int, 1>{});
    else if (c <= 2) f(std::integral_constant<int, 2>{});
    else if (c <= 4) f(std::integral_constant<int, 4>{});
    else if (c <= 8) f(std::integral_constant<int, 8>{});
    else if (c <= 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, CH_MAX>{});
}

// the launches of one pass: C / 32 chunks of 32 channels when C > 32, then one chunk of the smallest CH that holds the channels left.
// f(CH, grid, base): instantiation, launch grid and first channel
template <class F>
void for_each_launch(const CompositeArgs &a, int C, F f)
{
    const int full = C > CH_MAX ? C / CH_MAX : 0, rest = C - full * CH_MAX;
    if (full) f(std::integral_constant<int, CH_MAX>{}, dim3(a.tiles_x, a.tiles_y, full), 0);
    if (rest) for_ch(rest, [&](auto CH) { f(CH, dim3(a.tiles_x, a.tiles_y, 1), full * CH_MAX); });
}

}  // namespace

extern "C" {

int gc_rasterize_nd_fwd(int img_h, int img_w, int tiles_x, int tiles_y, int channels, const int32_t *gaussian_ids_sorted,
                        const int32_t *tile_bins, const float *xys, const float *conics, const float *colors, const float *opacities,
                        const float *background, float *out_img, float *final_Ts, int32_t *final_index, void *stream)
{
    GC_REQUIRE(channels >= 1, "channels must be >= 1");
    GC_REQUIRE(channels / CH_MAX < 65536, "channels must be < 32 * 65536");
    GC_REQUIRE((int64_t)img_h * img_w * channels < (1ll << 31), "H * W * channels must be < 2^31 elements");
    if (const int rc = check_tiles(__func__, img_h, img_w, tiles_x, tiles_y)) return rc;
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background, {}};
    for_each_launch(a, channels, [&](auto CH, dim3 grid, int base) {
        hipLaunchKernelGGL(k_rasterize_nd_fwd<decltype(CH)::value>, grid, dim3(BLOCK), 0, gc::S(stream), a.H, a.W, a.tiles_x, channels, base,
                           a.ids, a.bins, a.xys, a.conics, a.colors, a.opac, a.bg, out_img, final_Ts, final_index);
    });
    return gc::check_launch("gc_rasterize_nd_fwd");
}

int gc_rasterize_nd_bwd(int img_h, int img_w, int tiles_x, int tiles_y, int64_t N, int channels, const int32_t *gaussian_ids_sorted,
                        const int32_t *tile_bins, const float *xys, const float *conics, const float *colors, const float *opacities,
                        const float *background, const float *final_Ts, const int32_t *final_index, const float *v_out,
                        const float *v_out_alpha, float *v_xy, float *v_conic, float *v_colors, float *v_opacity, void *stream)
{
    GC_REQUIRE(channels >= 1, "channels must be >= 1");
    GC_REQUIRE(channels / CH_MAX < 65536, "channels must be < 32 * 65536");
    GC_REQUIRE(N >= 0 && N * channels < (1ll << 31), "N * channels must be < 2^31 elements");
    GC_REQUIRE((int64_t)img_h * img_w * channels < (1ll << 31), "H * W * channels must be < 2^31 elements");
    if (const int rc = check_tiles(__func__, img_h, img_w, tiles_x, tiles_y)) return rc;
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background, {}};
    for_each_launch(a, channels, [&](auto CH, dim3 grid, int base) {
        hipLaunchKernelGGL(k_rasterize_nd_bwd<decltype(CH)::value>, grid, dim3(BLOCK), 0, gc::S(stream), a.H, a.W, a.tiles_x, channels, base,
                           a.ids, a.bins, a.xys, a.conics, a.colors, a.opac, a.bg, final_Ts, final_index, v_out, v_out_alpha, v_xy, v_conic,
                           v_colors, v_opacity);
    });
    return gc::check_launch("gc_rasterize_nd_bwd");
}

}  // extern "C"

// raster_composite.hip -- per-tile alpha compositing (forward + backward) for gfx950.
//
// Replaces gsplat 0.1.3's rasterize_forward / rasterize_backward reached from
// /root/reference/gaussctrl/gc_model.py:174-186,191-202 and the autograd fired by gc_trainer.py:275.
// Semantics: SURVEY.md Appendix A.4 / A.5 (alpha cap 0.999, cull alpha < 1/255 or sigma < 0, stop
// when T*(1-alpha) <= 1e-4, pixel (j,i) sampled at (j,i)).
//
// CDNA4 mapping: one 16x16 tile = one 256-lane workgroup = 4 wave64s, each wave owning an 8x8 pixel
// block (a compact block is touched by fewer splats than a 16x4 strip: fwd 318 -> 293 us, bwd 515 -> 479 us at
// N = 4 M).  The tile's depth-sorted splat list is staged through LDS in batches of 256 records
// (48 B each, two ds_read_b128 + one ds_read_b64 per record, all lanes reading the same address ->
// LDS broadcast, no bank conflicts).  The RGB pass and the reference's second "depth" pass are one
// sweep (extra channel).  Backward replays the list back-to-front starting at the workgroup's
// largest final_index (not at the end of the tile list), reduces the nine per-splat partials over
// the 64 lanes with DPP row operations and issues one hardware float atomic per value per wave.
#include <type_traits>

#include "raster_tile.h"
#include "../../include/gaussctrl_absgrad.h"

namespace {

// Batched views (gc_rasterize_fwd_views / gc_rasterize_bwd_views): blockIdx.z = view, strides in CV (raster_tile.h).
struct SplatB { float cxy, cyy, r, g; };
struct SplatC { float b, e; };

template <bool HAS_EXTRA>
__global__ __launch_bounds__(BLOCK) void k_rasterize_fwd(int H, int W, int tiles_x,
                                                         const int32_t *__restrict__ ids_sorted,
                                                         const int32_t *__restrict__ tile_bins,
                                                         const float *__restrict__ xys, const float *__restrict__ conics,
                                                         const float *__restrict__ colors, const float *__restrict__ opacities,
                                                         const float *__restrict__ extra, const float *__restrict__ background,
                                                         float *__restrict__ out_img, float *__restrict__ out_extra,
                                                         float *__restrict__ final_Ts, int32_t *__restrict__ final_index, CV cv)
{
    {
        const int64_t v = blockIdx.z, hw = (int64_t)H * W;
        ids_sorted += v * cv.m; tile_bins += v * 2 * cv.tiles; xys += v * 2 * cv.n; conics += v * 3 * cv.n; colors += v * 3 * cv.n;
        opacities += v * cv.n_op; background += v * cv.bg;
        if (HAS_EXTRA) { extra += v * cv.n; out_extra += v * hw; }
        out_img += v * 3 * hw; final_Ts += v * hw; final_index += v * hw;
    }
    __shared__ SplatA sA[BLOCK];
    __shared__ SplatB sB[BLOCK];
    __shared__ SplatC sC[BLOCK];
    __shared__ unsigned char sMask[BLOCK];
    const TileCtx tc = tile_ctx(H, W, tiles_x, tile_bins);
    const int tid = tc.tid, lane = tc.lane, wid = tc.wid, end = tc.end;
    bool done = !tc.inside;
    float T = 1.f;
    int last = 0;
    float r = 0.f, g = 0.f, b = 0.f, e = 0.f;
    for (int bs = tc.start; bs < end; bs += BLOCK) {
        if (__syncthreads_and(done)) break;
        const int idx = bs + tid;
        unsigned mk = 0;
        if (idx < end) {
            const int gid = ids_sorted[idx];
            const Geom s = load_geometry(gid, xys, conics, opacities);
            sA[tid] = s.a;
            sB[tid] = {s.cxy, s.cyy, colors[3 * gid], colors[3 * gid + 1]};
            sC[tid] = {colors[3 * gid + 2], HAS_EXTRA ? extra[gid] : 0.f};
            mk = block_mask(s, tc.tx0, tc.ty0);
        }
        sMask[tid] = (unsigned char)mk;
        __syncthreads();
        const int n = min(BLOCK, end - bs);
        bool wave_done = __all(done);                                // a finished wave only helps staging
        for (int c = 0; c * 64 < n && !wave_done; ++c) {
            unsigned long long bal = block_ballot(sMask, c, lane, wid);
            if (!bal) continue;
            // scalar walk over the splats that can touch this block; branch-free body (selects), the next record is read from LDS
            // while the current one is evaluated
            int t = c * 64 + __builtin_ctzll(bal);
            bal &= bal - 1;
            SplatA a = sA[t];
            SplatB bb = sB[t];
            SplatC cc = sC[t];
            for (;;) {
                const int tn = c * 64 + (bal ? __builtin_ctzll(bal) : 0);
                const bool more = bal != 0;
                bal &= bal - 1;
                const SplatA an = sA[tn];
                const SplatB bn = sB[tn];
                const SplatC cn = sC[tn];
                const FwdStep f = fwd_step(a, bb.cxy, bb.cyy, tc.px, tc.py, bs + t, T, last, done);
                r += bb.r * f.vis; g += bb.g * f.vis; b += cc.b * f.vis;
                if (HAS_EXTRA) e += cc.e * f.vis;
                T = f.T; last = f.last; done = f.done;
                if (!more) break;
                if (__all(done)) { wave_done = true; break; }
                t = tn; a = an; bb = bn; cc = cn;
            }
        }
    }
    if (tc.inside) {
        const int pix = tc.i * W + tc.j;
        final_Ts[pix] = T;
        final_index[pix] = last;
        out_img[3 * pix] = r + T * background[0];
        out_img[3 * pix + 1] = g + T * background[1];
        out_img[3 * pix + 2] = b + T * background[2];
        if (HAS_EXTRA) out_extra[pix] = e;
    }
}

// Backward.  Per (block, splat) with at least one contributing pixel: nine partials are summed over the rows with DPP (36 adds), lane c
// of every row picks value c, two lane-swap steps add the four rows, and lanes 0..8 add their value into a per-batch LDS accumulator
// (ONE ds_add_f32 instruction).  After a batch the staging lane of each splat flushes nine hardware float atomics -- once per
// (tile, splat) instead of once per (block, splat), issued by 256 lanes at a time.
//
// HAS_DEPTH (gc_rasterize_bwd_depth_views): the forward's `extra` value is a fourth composited channel with background 0 -- E = sum e_i
// alpha_i T_i -- that the rgb clamp does not touch, and the backward of the finalize epilogue (depth = E / alpha_px, 1000 where alpha_px = 0)
// is folded into the pixel load like the clamp's: vE = v_depth / alpha_px, voa += -v_depth * depth / alpha_px; the sentinel carries no
// gradient.  Per (pixel, splat): g_e = fac * vE, v_alpha += (e_i T - S3 ra) vE, S3 += e_i fac.  A tenth partial rides the same reduction
// (lane column 9), the staged blue value becomes the forward's SplatC{b, e}.  <false> is the kernel without any of it.
//
// ABS (gc_rasterize_bwd_abs_views): absgrad densification (AbsGS; gsplat's `absgrad`).  Next to the signed v_xy the kernel sums |g_x|, |g_y|
// per (pixel, splat) -- taken after the pixel's whole v_sigma is formed (rgb, alpha and, with HAS_DEPTH, depth combined first), so opposite
// pulls of different PIXELS no longer cancel while the channels of one pixel still do.  Two more partials ride the same reduction in lane
// columns NP-2 / NP-1 and the staging lane flushes them into v_xy_abs [C][N][2].  A pair that passes no gradient (alpha cap, !valid) adds 0.
// <.., false> is the kernel without any of it.
struct DepthIO { const float *extra, *depth, *v_depth; float *v_extra; };      // [C][N], [C][H][W], [C][H][W]; [C][N] zero on entry
struct NoDepthIO {};
struct NoAbsIO {};

template <bool HAS_DEPTH, bool ABS>
__global__ __launch_bounds__(BLOCK) void k_rasterize_bwd(int H, int W, int tiles_x,
                                                         const int32_t *__restrict__ ids_sorted,
                                                         const int32_t *__restrict__ tile_bins,
                                                         const float *__restrict__ xys, const float *__restrict__ conics,
                                                         const float *__restrict__ colors, const float *__restrict__ opacities,
                                                         const float *__restrict__ background,
                                                         const float *__restrict__ final_Ts, const int32_t *__restrict__ final_index,
                                                         const float *__restrict__ v_out, const float *__restrict__ v_out_alpha,
                                                         const float *__restrict__ pre_clamp,
                                                         float *__restrict__ v_xy, float *__restrict__ v_conic,
                                                         float *__restrict__ v_colors, float *__restrict__ v_opacity, CV cv,
                                                         std::conditional_t<HAS_DEPTH, DepthIO, NoDepthIO> dz,
                                                         std::conditional_t<ABS, float *, NoAbsIO> v_xy_abs)
{
    constexpr int NP = (HAS_DEPTH ? 10 : 9) + (ABS ? 2 : 0);            // partials per splat
    {
        const int64_t v = blockIdx.z, hw = (int64_t)H * W;
        ids_sorted += v * cv.m; tile_bins += v * 2 * cv.tiles; xys += v * 2 * cv.n; conics += v * 3 * cv.n; colors += v * 3 * cv.n;
        opacities += v * cv.n_op; background += v * cv.bg;
        final_Ts += v * hw; final_index += v * hw; v_out += v * 3 * hw;
        if (v_out_alpha) v_out_alpha += v * hw;
        if (pre_clamp) pre_clamp += v * 3 * hw;
        v_xy += v * 2 * cv.n; v_conic += v * 3 * cv.n; v_colors += v * 3 * cv.n; v_opacity += v * cv.n;
        if constexpr (HAS_DEPTH) { dz.extra += v * cv.n; dz.depth += v * hw; dz.v_depth += v * hw; dz.v_extra += v * cv.n; }
        if constexpr (ABS) v_xy_abs += v * 2 * cv.n;
    }
    __shared__ SplatA sA[BLOCK];
    __shared__ SplatB sB[BLOCK];
    __shared__ std::conditional_t<HAS_DEPTH, SplatC, float> sBlue[BLOCK];
    __shared__ float sG[BLOCK * NP];
    __shared__ unsigned char sMask[BLOCK];
    __shared__ int sMax[4];
    const TileCtx tc = tile_ctx(H, W, tiles_x, tile_bins);
    const int tid = tc.tid, lane = tc.lane, wid = tc.wid, start = tc.start;
    const bool inside = tc.inside;
    if (tc.end <= start) return;
    const BwdPixel fp = bwd_pixel(tc, W, final_Ts, final_index);
    const int pix = fp.pix;
    const float T_final = fp.T_final;
    float T = T_final;
    float vo0 = 0.f, vo1 = 0.f, vo2 = 0.f, voa = 0.f;
    if (inside) {
        vo0 = v_out[3 * pix]; vo1 = v_out[3 * pix + 1]; vo2 = v_out[3 * pix + 2];
        if (pre_clamp) {      // backward of rgb = min(rgb, 1) (gc_model.py:188): the gradient passes where the un-clamped value is <= 1
            vo0 = pre_clamp[3 * pix] <= 1.f ? vo0 : 0.f; vo1 = pre_clamp[3 * pix + 1] <= 1.f ? vo1 : 0.f; vo2 = pre_clamp[3 * pix + 2] <= 1.f ? vo2 : 0.f;
        }
        if (v_out_alpha) voa = v_out_alpha[pix];
    }
    float vE = 0.f, S3 = 0.f;
    if constexpr (HAS_DEPTH) {
        const float alpha_px = 1.f - T_final;                           // as gc_raster_finalize formed it
        if (inside && alpha_px > 0.f) {
            const float vd = dz.v_depth[pix];
            vE = vd / alpha_px;
            voa += -vd * dz.depth[pix] / alpha_px;
        }
    }
    const float bgdot = background[0] * vo0 + background[1] * vo1 + background[2] * vo2;
    float S0 = 0.f, S1 = 0.f, S2 = 0.f;
    const WalkMax wm = bwd_walk_max<NP>(fp.bin_final, tid, lane, wid, sG, sMax);
    if (wm.kmax < start) return;
    const int col = lane & 15;
    for (int batch_end = wm.kmax; batch_end >= start; batch_end -= BLOCK) {
        const int idx = batch_end - tid;
        int gid = -1;
        unsigned mk = 0;
        if (idx >= start) {
            gid = ids_sorted[idx];
            const Geom s = load_geometry(gid, xys, conics, opacities);
            sA[tid] = s.a;
            sB[tid] = {s.cxy, s.cyy, colors[3 * gid], colors[3 * gid + 1]};
            if constexpr (HAS_DEPTH) sBlue[tid] = {colors[3 * gid + 2], dz.extra[gid]};
            else sBlue[tid] = colors[3 * gid + 2];
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
                const SplatB bb = sB[t];
                const Pair pr = pair_eval(a, bb.cxy, bb.cyy, tc.px, tc.py, batch_end - t, fp.bin_final);
                if (!__any(pr.valid)) continue;
                float g_r = 0.f, g_g = 0.f, g_b = 0.f, g_e = 0.f, g_ax = 0.f, g_ay = 0.f;
                GeomGrad gg{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (pr.valid) {
                    const PairT w = pair_weight(pr.alpha, T);
                    const float ra = w.ra, fac = w.fac;
                    T = w.T;
                    g_r = fac * vo0; g_g = fac * vo1; g_b = fac * vo2;
                    float cb, ce = 0.f;
                    if constexpr (HAS_DEPTH) { const SplatC cc = sBlue[t]; cb = cc.b; ce = cc.e; }
                    else cb = sBlue[t];
                    float v_alpha = (bb.r * T - S0 * ra) * vo0 + (bb.g * T - S1 * ra) * vo1 + (cb * T - S2 * ra) * vo2;
                    if constexpr (HAS_DEPTH) {
                        g_e = fac * vE;
                        v_alpha += (ce * T - S3 * ra) * vE;
                        S3 += ce * fac;
                    }
                    v_alpha += T_final * ra * voa;
                    v_alpha += -T_final * ra * bgdot;
                    S0 += bb.r * fac; S1 += bb.g * fac; S2 += cb * fac;
                    gg = geom_grad(v_alpha, pr, a, bb.cxy, bb.cyy);
                    if constexpr (ABS) { g_ax = fabsf(gg.x); g_ay = fabsf(gg.y); }
                }
                g_r = row_sum(g_r); g_g = row_sum(g_g); g_b = row_sum(g_b);
                gg.cxx = row_sum(gg.cxx); gg.cxy = row_sum(gg.cxy); gg.cyy = row_sum(gg.cyy);
                gg.x = row_sum(gg.x); gg.y = row_sum(gg.y); gg.o = row_sum(gg.o);
                float x = g_r;                                          // lane column c keeps value c
                x = col == 1 ? g_g : x; x = col == 2 ? g_b : x; x = col == 3 ? gg.cxx : x; x = col == 4 ? gg.cxy : x;
                x = col == 5 ? gg.cyy : x; x = col == 6 ? gg.x : x; x = col == 7 ? gg.y : x; x = col == 8 ? gg.o : x;
                if constexpr (HAS_DEPTH) { g_e = row_sum(g_e); x = col == 9 ? g_e : x; }
                if constexpr (ABS) { g_ax = row_sum(g_ax); g_ay = row_sum(g_ay); x = col == NP - 2 ? g_ax : x; x = col == NP - 1 ? g_ay : x; }
                x = xor_rows_sum(x);
                if (lane < NP) __hip_atomic_fetch_add(&sG[lane * BLOCK + t], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        if (gid >= 0) {                                                 // flush: NP atomics per (tile, splat) that was touched at all
            const auto [v, any] = take_partials<NP>(sG, tid);
            if (any) {
                unsafeAtomicAdd(v_colors + 3 * gid, v[0]);
                unsafeAtomicAdd(v_colors + 3 * gid + 1, v[1]);
                unsafeAtomicAdd(v_colors + 3 * gid + 2, v[2]);
                unsafeAtomicAdd(v_conic + 3 * gid, v[3]);
                unsafeAtomicAdd(v_conic + 3 * gid + 1, v[4]);
                unsafeAtomicAdd(v_conic + 3 * gid + 2, v[5]);
                unsafeAtomicAdd(v_xy + 2 * gid, v[6]);
                unsafeAtomicAdd(v_xy + 2 * gid + 1, v[7]);
                unsafeAtomicAdd(v_opacity + gid, v[8]);
                if constexpr (HAS_DEPTH) unsafeAtomicAdd(dz.v_extra + gid, v[9]);
                if constexpr (ABS) { unsafeAtomicAdd(v_xy_abs + 2 * gid, v[NP - 2]); unsafeAtomicAdd(v_xy_abs + 2 * gid + 1, v[NP - 1]); }
            }
        }
        // the next staging pass overwrites sA / sB / sMask: every wave has left the loop (barrier above); sG slots are private to
        // their staging lane until the next barrier
    }
}

// the launches: every entry point fills CompositeArgs (what each compositing launch reads) and the IO struct of its direction, and names itself
struct FwdIO { const float *extra; float *out_img, *out_extra, *final_Ts; int32_t *final_index; };
struct BwdIO {
    const float *final_Ts; const int32_t *final_index; const float *v_out, *v_out_alpha, *pre_clamp;
    float *v_xy, *v_conic, *v_colors, *v_opacity;
};

int rasterize_fwd_impl(const char *what, int C, const CompositeArgs &a, const FwdIO &o, void *stream)
{
    if (const int rc = check_tiles(what, a.H, a.W, a.tiles_x, a.tiles_y)) return rc;
    if ((o.extra == nullptr) != (o.out_extra == nullptr)) { gc::set_error("%s: extra and out_extra must be given together", what); return GC_EINVAL; }
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(a.tiles_x, a.tiles_y, C), dim3(BLOCK), 0, gc::S(stream), a.H, a.W, a.tiles_x, a.ids, a.bins, a.xys, a.conics,
                           a.colors, a.opac, o.extra, a.bg, o.out_img, o.out_extra, o.final_Ts, o.final_index, a.cv);
    };
    if (o.extra) launch(k_rasterize_fwd<true>);
    else launch(k_rasterize_fwd<false>);
    return gc::check_launch(what);
}

int rasterize_bwd_impl(const char *what, int C, const CompositeArgs &a, const BwdIO &o, void *stream, const DepthIO *dz = nullptr,
                       float *v_xy_abs = nullptr)
{
    if (const int rc = check_tiles(what, a.H, a.W, a.tiles_x, a.tiles_y)) return rc;
    // the kernel's last two parameters are the empty structs where a switch is off
    const auto launch = [&](auto kernel, auto dz_arg, auto abs_arg) {
        hipLaunchKernelGGL(kernel, dim3(a.tiles_x, a.tiles_y, C), dim3(BLOCK), 0, gc::S(stream), a.H, a.W, a.tiles_x, a.ids, a.bins, a.xys, a.conics,
                           a.colors, a.opac, a.bg, o.final_Ts, o.final_index, o.v_out, o.v_out_alpha, o.pre_clamp, o.v_xy, o.v_conic, o.v_colors,
                           o.v_opacity, a.cv, dz_arg, abs_arg);
    };
    if (dz && v_xy_abs) launch(k_rasterize_bwd<true, true>, *dz, v_xy_abs);
    else if (v_xy_abs) launch(k_rasterize_bwd<false, true>, NoDepthIO{}, v_xy_abs);
    else if (dz) launch(k_rasterize_bwd<true, false>, *dz, NoAbsIO{});
    else launch(k_rasterize_bwd<false, false>, NoDepthIO{}, NoAbsIO{});
    return gc::check_launch(what);
}

}  // namespace

extern "C" {

int gc_rasterize_fwd(int img_h, int img_w, int tiles_x, int tiles_y, const int32_t *gaussian_ids_sorted,
                     const int32_t *tile_bins, const float *xys, const float *conics, const float *colors,
                     const float *opacities, const float *extra, const float *background, float *out_img,
                     float *out_extra, float *final_Ts, int32_t *final_index, void *stream)
{
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                          view_strides(0, 0, 1, 1, tiles_x * tiles_y)};
    return rasterize_fwd_impl("gc_rasterize_fwd", 1, a, {extra, out_img, out_extra, final_Ts, final_index}, stream);
}

/* C views in one launch (grid.z = view): gaussian_ids_sorted [C][M_cap], tile_bins [C][T][2], xys / conics / colors / extra [C][N][..],
 * opacities [N] (shared_opacities = 1) or [C][N], background [3] (shared_background = 1) or [C][3]; outputs [C][H][W][..]. */
int gc_rasterize_fwd_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int shared_background, int img_h, int img_w, int tiles_x,
                           int tiles_y, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                           const float *colors, const float *opacities, const float *extra, const float *background, float *out_img,
                           float *out_extra, float *final_Ts, int32_t *final_index, void *stream)
{
    GC_REQUIRE(C >= 1 && C <= 65535 && N >= 0 && M_cap >= 0, "bad arguments");
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                          view_strides(N, M_cap, shared_opacities, shared_background, tiles_x * tiles_y)};
    return rasterize_fwd_impl("gc_rasterize_fwd_views", C, a, {extra, out_img, out_extra, final_Ts, final_index}, stream);
}

int gc_rasterize_bwd(int img_h, int img_w, int tiles_x, int tiles_y, int64_t N, const int32_t *gaussian_ids_sorted,
                     const int32_t *tile_bins, const float *xys, const float *conics, const float *colors,
                     const float *opacities, const float *background, const float *final_Ts, const int32_t *final_index,
                     const float *v_out, const float *v_out_alpha, float *v_xy, float *v_conic, float *v_colors,
                     float *v_opacity, void *stream)
{
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                          view_strides(N, 0, 1, 1, tiles_x * tiles_y)};
    return rasterize_bwd_impl("gc_rasterize_bwd", 1, a, {final_Ts, final_index, v_out, v_out_alpha, nullptr, v_xy, v_conic, v_colors, v_opacity}, stream);
}

/* the same with the backward of get_outputs' rgb clamp folded into the pixel load: v_out is masked where pre_clamp > 1 */
int gc_rasterize_bwd_clamped(int img_h, int img_w, int tiles_x, int tiles_y, int64_t N, const int32_t *gaussian_ids_sorted,
                             const int32_t *tile_bins, const float *xys, const float *conics, const float *colors,
                             const float *opacities, const float *background, const float *final_Ts, const int32_t *final_index,
                             const float *v_out, const float *v_out_alpha, const float *pre_clamp, float *v_xy, float *v_conic,
                             float *v_colors, float *v_opacity, void *stream)
{
    GC_REQUIRE(pre_clamp, "pre_clamp image required (gc_rasterize_bwd is the form without the clamp)");
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                          view_strides(N, 0, 1, 1, tiles_x * tiles_y)};
    return rasterize_bwd_impl("gc_rasterize_bwd_clamped", 1, a,
                              {final_Ts, final_index, v_out, v_out_alpha, pre_clamp, v_xy, v_conic, v_colors, v_opacity}, stream);
}

/* C views in one launch: v_out [C][H][W][3], v_out_alpha [C][H][W] or NULL, pre_clamp [C][H][W][3] or NULL (clamp backward folded in);
 * v_xy [C][N][2], v_conic [C][N][3], v_colors [C][N][3], v_opacity [C][N] must be ZERO on entry (the kernel adds into them). */
int gc_rasterize_bwd_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int shared_background, int img_h, int img_w, int tiles_x,
                           int tiles_y, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                           const float *colors, const float *opacities, const float *background, const float *final_Ts,
                           const int32_t *final_index, const float *v_out, const float *v_out_alpha, const float *pre_clamp, float *v_xy,
                           float *v_conic, float *v_colors, float *v_opacity, void *stream)
{
    GC_REQUIRE(C >= 1 && C <= 65535 && N >= 0 && M_cap >= 0, "bad arguments");
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                          view_strides(N, M_cap, shared_opacities, shared_background, tiles_x * tiles_y)};
    return rasterize_bwd_impl("gc_rasterize_bwd_views", C, a,
                              {final_Ts, final_index, v_out, v_out_alpha, pre_clamp, v_xy, v_conic, v_colors, v_opacity}, stream);
}

/* gc_rasterize_bwd_views with the depth channel differentiable (k_rasterize_bwd<true>): extra [C][N] = what the forward composited, depth
 * [C][H][W] = the FINALIZED image (E / alpha, 1000 where alpha == 0), v_depth [C][H][W] its gradient; v_extra [C][N] ZERO on entry like the
 * other four outputs.  C = 1 is the single-view case (M_cap is then not read). */
int gc_rasterize_bwd_depth_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int shared_background, int img_h, int img_w, int tiles_x,
                                 int tiles_y, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                                 const float *colors, const float *opacities, const float *background, const float *final_Ts,
                                 const int32_t *final_index, const float *v_out, const float *v_out_alpha, const float *pre_clamp, float *v_xy,
                                 float *v_conic, float *v_colors, float *v_opacity, const float *extra, const float *depth, const float *v_depth,
                                 float *v_extra, void *stream)
{
    GC_REQUIRE(C >= 1 && C <= 65535 && N >= 0 && M_cap >= 0, "bad arguments");
    GC_REQUIRE(extra && depth && v_depth && v_extra, "extra, depth, v_depth and v_extra are required (gc_rasterize_bwd_views is the form without depth)");
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                          view_strides(N, M_cap, shared_opacities, shared_background, tiles_x * tiles_y)};
    const DepthIO dz{extra, depth, v_depth, v_extra};
    return rasterize_bwd_impl("gc_rasterize_bwd_depth_views", C, a,
                              {final_Ts, final_index, v_out, v_out_alpha, pre_clamp, v_xy, v_conic, v_colors, v_opacity}, stream, &dz);
}

/* absgrad densification (include/gaussctrl_absgrad.h, k_rasterize_bwd<.., true>): the arguments of gc_rasterize_bwd_depth_views plus v_xy_abs
 * [C][N][2], ZERO on entry, which receives sum over pixels of (|dL_p/dx|, |dL_p/dy|).  The depth quartet is all NULL (the form without depth)
 * or all set. */
int gc_rasterize_bwd_abs_views(int C, int64_t N, int64_t M_cap, int shared_opacities, int shared_background, int img_h, int img_w, int tiles_x,
                               int tiles_y, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys, const float *conics,
                               const float *colors, const float *opacities, const float *background, const float *final_Ts,
                               const int32_t *final_index, const float *v_out, const float *v_out_alpha, const float *pre_clamp, float *v_xy,
                               float *v_conic, float *v_colors, float *v_opacity, const float *extra, const float *depth, const float *v_depth,
                               float *v_extra, float *v_xy_abs, void *stream)
{
    GC_REQUIRE(C >= 1 && C <= 65535 && N >= 0 && M_cap >= 0, "bad arguments");
    const int set = (extra != nullptr) + (depth != nullptr) + (v_depth != nullptr) + (v_extra != nullptr);
    if (N > 0) {      // (the per-Gaussian arrays of an empty scene have no address)
        GC_REQUIRE(v_xy_abs, "v_xy_abs is required (gc_rasterize_bwd_views / gc_rasterize_bwd_depth_views are the forms without it)");
        GC_REQUIRE(set == 0 || set == 4, "extra, depth, v_depth and v_extra must be all NULL (no depth) or all set");
    }
    const CompositeArgs a{img_h, img_w, tiles_x, tiles_y, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                          view_strides(N, M_cap, shared_opacities, shared_background, tiles_x * tiles_y)};
    const DepthIO dz{extra, depth, v_depth, v_extra};
    return rasterize_bwd_impl("gc_rasterize_bwd_abs_views", C, a,
                              {final_Ts, final_index, v_out, v_out_alpha, pre_clamp, v_xy, v_conic, v_colors, v_opacity}, stream,
                              set == 4 ? &dz : nullptr, v_xy_abs);
}

}  // extern "C"

// raster_tile.h -- the tile compositor written once for the 3-channel kernels (raster_composite.hip) and the N-channel ones
// (raster_composite_nd.hip): the SURVEY A.4 constants, the first splat record, the exact per-block culling mask, the DPP / lane-swap
// reductions of the backward, and the tile walk itself -- tile context, record staging, the forward per-(pixel, splat) step, the backward
// prologue, pair step and gradient tail, batch bounds and ballots, the take-and-test of a splat's partials.  The pieces are __forceinline__
// and hand state in and out BY VALUE (a helper that advances a caller's array through a reference is what put the conv cursor into scratch,
// DESIGN.md 3.2).  A kernel owns only its memory schedule: LDS layout, prefetch, channel accumulation, placement of the partials on lane
// columns and the list of atomics it flushes.  Host side: what every compositing launch reads (CompositeArgs) and the tile-bounds check.
// Everything is in an unnamed namespace: each translation unit keeps its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int TILE = 16;
constexpr int BLOCK = TILE * TILE;
constexpr float ALPHA_CAP = 0.999f;
constexpr float ALPHA_MIN = 1.f / 255.f;
constexpr float T_STOP = 1e-4f;

struct SplatA { float x, y, opac, cxx; };

// ---- block culling ---------------------------------------------------------------------------------------------------------
// gsplat bins a Gaussian into every tile of the BOX around a circle of 3 sqrt(lambda_max); most (tile, Gaussian) pairs of an anisotropic
// or faint Gaussian never reach alpha >= 1/255 anywhere in the tile, and of the rest few touch all four 8x8 blocks.  When a batch is
// staged, the lane that loads a record also evaluates -- exactly, the form is convex -- the minimum of sigma over each block's
// rectangle of pixel centres and keeps a 4-bit mask "block w can reach alpha >= 1/255" (threshold sigma <= ln(255 opacity), with a
// margin far above the rounding of either side).  A wave then walks only the set bits of its block's ballot (scalar loop: s_ff1 +
// s_andn2), so culled pairs cost no vector work at all.  The per-pixel test is unchanged: results are bit-identical to the unculled loop.
__device__ __forceinline__ float edge_min(float a, float b, float c, float rc, float e, float lo, float hi)
{
    // min over v in [lo, hi] of 0.5 (a e^2 + c v^2) + b e v   (c > 0, rc = 1-ulp reciprocal of c): v* = clamp(-b e / c).  Evaluating at a
    // v that is off by delta overestimates the minimum by c delta^2 / 2 ~ 1e-14 sigma -- twelve orders below the margin kept on tau
    const float v = fminf(fmaxf(-b * e * rc, lo), hi);
    return 0.5f * (a * e * e + c * v * v) + b * e * v;
}

__device__ __forceinline__ unsigned block_mask(const float x, const float y, const float opac, const float cxx, const float cxy,
                                               const float cyy, const float tile_x0, const float tile_y0)
{
#ifdef GC_NO_BLOCK_CULL                                                  // A/B builds only (tests compare culled vs unculled)
    return 0xFu;
#endif
    if (!(cxx > 0.f && cyy > 0.f)) return 0xFu;                       // degenerate conic: no culling
    const float tau = __logf(255.f * opac) * 1.001f + 0.01f;          // alpha >= 1/255  <=>  sigma <= ln(255 opacity)
    if (!(tau >= 0.f)) return tau < 0.f ? 0u : 0xFu;                  // NaN -> keep
    const float rxx = __builtin_amdgcn_rcpf(cxx), ryy = __builtin_amdgcn_rcpf(cyy);
    unsigned m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {                                     // wave w owns the 8x8 block (w & 1, w >> 1) of the tile
        const float bx = tile_x0 + 8.f * (w & 1), by = tile_y0 + 8.f * (w >> 1);
        const float dx0 = x - (bx + 7.f), dx1 = x - bx, dy0 = y - (by + 7.f), dy1 = y - by;      // d = splat - pixel over the block
        float smin;
        if (dx0 <= 0.f && dx1 >= 0.f && dy0 <= 0.f && dy1 >= 0.f) smin = 0.f;
        else {
            smin = fminf(fminf(edge_min(cxx, cxy, cyy, ryy, dx0, dy0, dy1), edge_min(cxx, cxy, cyy, ryy, dx1, dy0, dy1)),
                         fminf(edge_min(cyy, cxy, cxx, rxx, dy0, dx0, dx1), edge_min(cyy, cxy, cxx, rxx, dy1, dx0, dx1)));
        }
        if (!(smin > tau)) m |= 1u << w;
    }
    return m;
}

// ---- reduction of the per-splat partials over a wave --------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)      // v + v[dpp lane], all rows / banks
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_sum(float v)      // every lane ends with the sum over its row of 16 lanes
{
    v = dpp_add<0xB1>(v);     // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);     // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);    // row_half_mirror
    v = dpp_add<0x140>(v);    // row_mirror
    return v;
}
__device__ __forceinline__ float xor_rows_sum(float v)  // sum over the four rows, lane-wise (lane l: lanes l%16 + 16 k)
{
    {
        const unsigned x = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
        v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    {
        const unsigned x = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
        v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    return v;
}

// ---- the tile walk ------------------------------------------------------------------------------------------------------------
// Batched views: blockIdx.z = view (camera); per-view arrays are [C][...] with the strides below (elements).  A single-view launch has
// gridDim.z == 1: every offset is 0.
struct CV {
    int64_t n;       // per-Gaussian arrays of a view: xys / 2, conics / 3, colors / 3, extra, v_* ([C][N])
    int64_t n_op;    // opacities: N when per view, 0 when one array serves every view (sigmoid(opacity) does not depend on the camera)
    int64_t m;       // gaussian_ids_sorted ([C][M_cap])
    int tiles;       // tile_bins ([C][T][2])
    int bg;          // background: 3 when per view, 0 when shared
};

// one workgroup = one 16x16 tile, one wave = one 8x8 pixel block of it, one lane = pixel (j, i)
struct TileCtx {
    int tid, lane, wid, i, j;
    bool inside;
    float px, py, tx0, ty0;
    int start, end;                                                    // the tile's range of the sorted list
};
__device__ __forceinline__ TileCtx tile_ctx(int H, int W, int tiles_x, const int32_t *__restrict__ tile_bins)
{
    TileCtx c;
    const int tile = blockIdx.y * tiles_x + blockIdx.x;
    c.tid = threadIdx.x; c.lane = c.tid & 63; c.wid = c.tid >> 6;
    c.j = blockIdx.x * TILE + 8 * (c.wid & 1) + (c.lane & 7);
    c.i = blockIdx.y * TILE + 8 * (c.wid >> 1) + (c.lane >> 3);
    c.inside = (c.i < H) && (c.j < W);
    c.px = (float)c.j; c.py = (float)c.i;
    c.tx0 = (float)(blockIdx.x * TILE); c.ty0 = (float)(blockIdx.y * TILE);
    c.start = tile_bins[2 * tile]; c.end = tile_bins[2 * tile + 1];
    return c;
}

// the geometry of one list entry as its staging lane loads it (I = the caller's index width) and its culling mask.  Two pieces: the
// kernel stores the record to LDS between them, so the record is not live across the mask's branches
struct Geom { SplatA a; float cxy, cyy; };
template <typename I>
__device__ __forceinline__ Geom load_geometry(I gid, const float *__restrict__ xys, const float *__restrict__ conics,
                                              const float *__restrict__ opacities)
{
    const float2 xy = *reinterpret_cast<const float2 *>(xys + 2 * gid);
    const float c0 = conics[3 * gid], c1 = conics[3 * gid + 1], c2 = conics[3 * gid + 2];
    return {{xy.x, xy.y, opacities[gid], c0}, c1, c2};
}
__device__ __forceinline__ unsigned block_mask(const Geom g, float tile_x0, float tile_y0)
{
    return block_mask(g.a.x, g.a.y, g.a.opac, g.a.cxx, g.cxy, g.cyy, tile_x0, tile_y0);
}

// the ballot of "record c * 64 + lane can reach this wave's block"; _from: without the records before t0 of the batch
__device__ __forceinline__ unsigned long long block_ballot(const unsigned char *sMask, int c, int lane, int wid)
{
    return __ballot((sMask[c * 64 + lane] >> wid) & 1);
}
__device__ __forceinline__ unsigned long long block_ballot_from(const unsigned char *sMask, int c, int lane, int wid, int t0)
{
    unsigned long long bal = block_ballot(sMask, c, lane, wid);
    if (c * 64 < t0) bal &= ~0ull << (t0 - c * 64);
    return bal;
}

// sigma = 0.5 (cxx dx^2 + cyy dy^2) + cxy dx dy with the two fused multiply-adds WRITTEN OUT: under -ffp-contract=fast the compiler picks which
// product of a sum it fuses per call site, and forward, backward and both channel layouts must form the same bits (final_index decisions)
__device__ __forceinline__ float conic_sigma(float cxx, float cxy, float cyy, float dx, float dy)
{
    return __fmaf_rn(cxy * dx, dy, 0.5f * __fmaf_rn(cxx * dx, dx, cyy * dy * dy));
}

// Forward, one (pixel, splat): the one place the forward applies ALPHA_CAP, ALPHA_MIN and T_STOP.  k = the splat's index in the sorted
// list; T / last / done = the pixel's state before and after; vis = alpha T when the splat is composited, else 0.  (The kernels keep
// the state in three locals: carried through a loop inside a struct, the bool comes back as a byte in a VGPR.)
struct FwdStep { float T; int last; bool done; float vis; };
__device__ __forceinline__ FwdStep fwd_step(const SplatA a, float cxy, float cyy, float px, float py, int k, float T, int last, bool done)
{
    const float dx = a.x - px, dy = a.y - py;
    const float sigma = conic_sigma(a.cxx, cxy, cyy, dx, dy);
    const float alpha = fminf(ALPHA_CAP, a.opac * __expf(-sigma));
    const bool hit = !done && !(sigma < 0.f || alpha < ALPHA_MIN);
    const float next_T = T * (1.f - alpha);
    const bool stop = hit && next_T <= T_STOP;
    const bool add = hit && !stop;
    const float vis = add ? alpha * T : 0.f;
    T = add ? next_T : T;
    last = add ? k : last;
    done |= stop;
    return {T, last, done, vis};
}

// Backward prologue.  What the forward left for the pixel ...
struct BwdPixel { int pix; float T_final; int bin_final; };
__device__ __forceinline__ BwdPixel bwd_pixel(const TileCtx c, int W, const float *__restrict__ final_Ts, const int32_t *__restrict__ final_index)
{
    const int pix = c.inside ? c.i * W + c.j : 0;
    return {pix, c.inside ? final_Ts[pix] : 1.f, c.inside ? final_index[pix] : -1};
}
// ... and the wave / workgroup maxima of final_index (nothing beyond them was composited), with the NP x BLOCK accumulator zeroed.
// Both are wave-uniform: they keep the splat walk in scalar registers.  Ends with a barrier.
struct WalkMax { int wmax, kmax; };
template <int NP>
__device__ __forceinline__ WalkMax bwd_walk_max(int bin_final, int tid, int lane, int wid, float *sG, int *sMax)
{
    int wmax = bin_final;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d, 64));
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    if (lane == 0) sMax[wid] = wmax;
#pragma unroll
    for (int q = 0; q < NP; ++q) sG[q * BLOCK + tid] = 0.f;
    __syncthreads();
    return {wmax, __builtin_amdgcn_readfirstlane(max(max(sMax[0], sMax[1]), max(sMax[2], sMax[3])))};
}

// a backward batch ends at list index batch_end and runs towards start: n records, of which the first t0 lie behind every pixel's last one
struct BwdBatch { int n, t0; };
__device__ __forceinline__ BwdBatch bwd_batch(int batch_end, int start, int wmax)
{
    return {min(BLOCK, batch_end - start + 1), max(0, batch_end - wmax)};
}

// Backward, one (pixel, splat) in two parts around the wave's "no pixel is valid" early-out: the pair's alpha as the forward formed it ...
struct Pair { float dx, dy, vis, araw, alpha; bool valid; };
__device__ __forceinline__ Pair pair_eval(const SplatA a, float cxy, float cyy, float px, float py, int k, int bin_final)
{
    const float dx = a.x - px, dy = a.y - py;
    const float sigma = conic_sigma(a.cxx, cxy, cyy, dx, dy);
    const float vis = __expf(-sigma);
    const float araw = a.opac * vis;
    const float alpha = fminf(ALPHA_CAP, araw);
    return {dx, dy, vis, araw, alpha, (k <= bin_final) && !(sigma < 0.f || alpha < ALPHA_MIN)};
}
// ... and, for a valid pixel, the transmittance in front of the splat (T is the one behind it) and its weight fac = alpha T
struct PairT { float ra, T, fac; };
__device__ __forceinline__ PairT pair_weight(float alpha, float T)
{
    const float ra = __builtin_amdgcn_rcpf(1.f - alpha);               // 1-ulp reciprocal: alpha <= 0.999, the IEEE division sequence is 10 instructions
    T *= ra;
    return {ra, T, alpha * T};
}

// Gradient tail: from the pixel's v_alpha the opacity partial (o) and the five geometry partials.  alpha clamped at the cap passes no
// gradient to sigma / opacity (select instead of a nested exec-mask branch).
struct GeomGrad { float cxx, cxy, cyy, x, y, o; };
__device__ __forceinline__ GeomGrad geom_grad(float v_alpha, const Pair p, const SplatA a, float cxy, float cyy)
{
    const float va = p.araw > ALPHA_CAP ? 0.f : p.vis * v_alpha;
    const float v_sigma = -a.opac * va;
    return {0.5f * v_sigma * p.dx * p.dx, v_sigma * p.dx * p.dy, 0.5f * v_sigma * p.dy * p.dy,
            v_sigma * (a.cxx * p.dx + cxy * p.dy), v_sigma * (cxy * p.dx + cyy * p.dy), va};
}

// the staging lane takes its splat's NP partials out of the accumulator (and leaves zeros); any = at least one is non-zero
template <int NP> struct Partials { float v[NP]; bool any; };
template <int NP>
__device__ __forceinline__ Partials<NP> take_partials(float *sG, int tid)
{
    Partials<NP> p;
    p.any = false;
#pragma unroll
    for (int q = 0; q < NP; ++q) { p.v[q] = sG[q * BLOCK + tid]; sG[q * BLOCK + tid] = 0.f; p.any |= p.v[q] != 0.f; }
    return p;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// what every compositing launch reads; grid = (tiles_x, tiles_y, views or channel chunks)
struct CompositeArgs {
    int H, W, tiles_x, tiles_y;
    const int32_t *ids, *bins;
    const float *xys, *conics, *colors, *opac, *bg;
    CV cv;
};
inline CV view_strides(int64_t N, int64_t M_cap, int shared_opacities, int shared_background, int tiles)
{
    return {N, shared_opacities ? 0 : N, M_cap, tiles, shared_background ? 0 : 3};
}
inline int check_tiles(const char *what, int H, int W, int tiles_x, int tiles_y)
{
    if (H > 0 && W > 0 && tiles_x == (W + TILE - 1) / TILE && tiles_y == (H + TILE - 1) / TILE) return GC_OK;
    gc::set_error("%s: tile bounds do not match the image size", what);
    return GC_EINVAL;
}

}  // namespace

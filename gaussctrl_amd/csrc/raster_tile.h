// raster_tile.h -- pieces of the tile compositor shared by the 3-channel kernels (raster_composite.hip) and the N-channel
// ones (raster_composite_nd.hip): the SURVEY A.4 constants, the first splat record, the exact per-block culling mask and the
// DPP / lane-swap reductions of the backward.  Everything is in an unnamed namespace: each translation unit keeps its own copy.
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

}  // namespace

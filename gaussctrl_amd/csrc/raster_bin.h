// raster_bin.h -- pieces of the tile binning shared by raster_bin.hip (scan, gsplat-shaped chain) and raster_sort.hip (two-level binning).
#pragma once
#include "common.h"

namespace {

constexpr int TILE = 16;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int wave_incl_scan(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(v, d, 64); if (lane >= d) v += y; }
    return v;
}

// inclusive scan of one int per thread over a workgroup of 256 threads (4 waves); *total = the workgroup's sum.  The leading barrier lets a
// kernel call it again right away (the four wave sums are one LDS array per kernel).
__device__ __forceinline__ int block_incl_scan256(int v, int *total)
{
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int sc = wave_incl_scan(v);
    __syncthreads();
    if (lane == 63) wsum[wid] = sc;
    __syncthreads();
    int off = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) if (w < wid) off += wsum[w];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return sc + off;
}

}  // namespace

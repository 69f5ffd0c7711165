// train_rows.h -- pieces shared by the kernels that change a scene's rows (train_refine.hip, train_mcmc.hip), in an unnamed namespace: each
// translation unit keeps its own copy; both are built with the STRICT flags (no contraction), so the expressions are evaluated as written wherever
// they are inlined.  Per-lane state (row values, child rows, masks) goes in and out of every function BY VALUE; the lambdas of for_narrow touch
// only locals of the function that holds them.  No kernel of the two files has private memory (tests/test_kernel_resources.py).
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int BLK = 256;                  // Gaussians (or draws) per workgroup, one per lane
constexpr int MAX_REST = 45;              // floats of features_rest per Gaussian at sh_degree 3
inline bool fits_i32(int64_t elements) { return elements < (1ll << 31); }
__device__ __forceinline__ int lanes_below(uint64_t mask) { return __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// One workgroup of 256 lanes: the exclusive scan of counts[0 .. n), in place when `write` is set; returns the total in every lane.
// 256-entry chunks with a running carry; a chunk's sum is (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]).
__device__ __forceinline__ int32_t scan_counts(int32_t *__restrict__ counts, int64_t n, bool write)
{
    __shared__ int32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int32_t carry = 0;
    for (int64_t base = 0; base < n; base += 256) {
        const int64_t j = base + tid;
        const int32_t v = j < n ? counts[j] : 0;
        int32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int32_t before = 0;
        for (int k = 0; k < w; ++k) before += wsum[k];
        const int32_t all = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (j < n && write) counts[j] = carry + before + inc - v;
        carry += all;
        __syncthreads();
    }
    return carry;
}

// The rank of a flagged lane among the flagged lanes of the whole launch: the workgroup's offset + the counts of the waves before + the
// lanes below.  wcnt[w] = popcount of wave w's ballot, published by the caller before ITS barrier (one for all its flags).
__device__ __forceinline__ int32_t ballot_rank(int32_t block_off, uint64_t ballot, const int32_t *wcnt)
{
    int32_t r = block_off + lanes_below(ballot);
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) r += wcnt[k];
    return r;
}

struct Vec64 { double x, y, z; };
struct Rot64 {                             // Rot(q / |q|) of a float quaternion (w, x, y, z), in double
    double r00, r01, r02, r10, r11, r12, r20, r21, r22;

    __device__ __forceinline__ Rot64(float fw, float fx, float fy, float fz)
    {
        const double qw = fw, qx = fx, qy = fy, qz = fz;
        const double inv = 1.0 / sqrt((qw * qw + qx * qx) + (qy * qy + qz * qz));
        const double w = qw * inv, x = qx * inv, y = qy * inv, z = qz * inv;
        r00 = 1.0 - 2.0 * (y * y + z * z); r01 = 2.0 * (x * y - w * z); r02 = 2.0 * (x * z + w * y);
        r10 = 2.0 * (x * y + w * z); r11 = 1.0 - 2.0 * (x * x + z * z); r12 = 2.0 * (y * z - w * x);
        r20 = 2.0 * (x * z - w * y); r21 = 2.0 * (y * z + w * x); r22 = 1.0 - 2.0 * (x * x + y * y);
    }
    __device__ __forceinline__ Vec64 mul(double a, double b, double c) const         // R v
    { return {(r00 * a + r01 * b) + r02 * c, (r10 * a + r11 * b) + r12 * c, (r20 * a + r21 * b) + r22 * c}; }
    __device__ __forceinline__ Vec64 mul_t(double a, double b, double c) const       // R^T v
    { return {(r00 * a + r10 * b) + r20 * c, (r01 * a + r11 * b) + r21 * c, (r02 * a + r12 * b) + r22 * c}; }
};

// the six tensors in the order means, scales, quats, opacities, features_dc, features_rest; [0] parameters, [1] exp_avg, [2] exp_avg_sq
template <typename T> struct RowTable { T *t[3][6]; };
using ConstRows = RowTable<const float>; using Rows = RowTable<float>;

// the ABI's three pointer arrays into a table (a null moment array: no such moment); false when a tensor in use has no parameter pointer
template <typename T>
inline bool fill_rows(RowTable<T> &tab, int rest_floats, T *const *params, T *const *exp_avg, T *const *exp_avg_sq)
{
    bool ok = true;
    for (int k = 0; k < 6; ++k) {
        tab.t[0][k] = params[k];
        tab.t[1][k] = exp_avg ? exp_avg[k] : nullptr;
        tab.t[2][k] = exp_avg_sq ? exp_avg_sq[k] : nullptr;
        ok = ok && (params[k] || (k == 5 && rest_floats == 0));
    }
    return ok;
}

struct Narrow { float v[14]; };           // one Gaussian's row of the five narrow tensors, side by side
constexpr int MEAN_AT = 0, SCALE_AT = 3, QUAT_AT = 6, OPACITY_AT = 10, DC_AT = 11;

// The five narrow tensors: f(tensor index, width, first float in Narrow), each an integral constant.  The widths are written here only.
template <int V> using Int = std::integral_constant<int, V>;
template <typename F>
__device__ __forceinline__ void for_narrow(F f)
{
    f(Int<0>{}, Int<3>{}, Int<MEAN_AT>{}); f(Int<1>{}, Int<3>{}, Int<SCALE_AT>{}); f(Int<2>{}, Int<4>{}, Int<QUAT_AT>{});
    f(Int<3>{}, Int<1>{}, Int<OPACITY_AT>{}); f(Int<4>{}, Int<3>{}, Int<DC_AT>{});
}

// Rows of the five narrow tensors in part m of a table; a tensor that does not exist (a missing moment) is skipped.
template <typename T>
__device__ __forceinline__ Narrow load_narrow(const RowTable<T> &tab, int m, int64_t row)
{
    Narrow r = {};
    for_narrow([&](auto t, auto w, auto o) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < w; ++c) r.v[o + c] = tab.t[m][t] ? tab.t[m][t][row * w + c] : 0.f;
    });
    return r;
}
__device__ __forceinline__ void store_narrow(const Rows &tab, int m, int64_t row, Narrow r)
{
    for_narrow([&](auto t, auto w, auto o) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < w; ++c) if (tab.t[m][t]) tab.t[m][t][row * w + c] = r.v[o + c];
    });
}
// per tensor, without the detour through a Narrow: parameter row `from` into row `to`; both moments of a row, where they exist, zero
__device__ __forceinline__ void copy_narrow(const Rows &tab, int64_t from, int64_t to)
{
    for_narrow([&](auto t, auto w, auto) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < w; ++c) tab.t[0][t][to * w + c] = tab.t[0][t][from * w + c];
    });
}
__device__ __forceinline__ void zero_narrow_moments(const Rows &tab, int64_t row)
{
#pragma unroll
    for (int m = 1; m < 3; ++m)
        for_narrow([&](auto t, auto w, auto) __attribute__((always_inline)) {
            if (!tab.t[m][t]) return;
#pragma unroll
            for (int c = 0; c < w; ++c) tab.t[m][t][row * w + c] = 0.f;
        });
}

// f(Int<rest_floats>{}) for the four widths of features_rest (sh_degree 0 .. 3); the entry points have refused every other value
template <typename F>
inline void with_rest_floats(int rest_floats, F f)
{
    switch (rest_floats) {
    case 0: f(Int<0>{}); break;
    case 9: f(Int<9>{}); break;
    case 24: f(Int<24>{}); break;
    default: f(Int<45>{}); break;
    }
}

}  // namespace

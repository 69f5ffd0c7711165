// train_bilagrid.hip -- per-view bilateral grids of 3x4 colour transforms (include/gaussctrl_bilagrid.h) for gfx950: the slice at
// (x, y, luma) with its backward, and the total-variation regulariser.
//
// The slice kernels run one 256-lane workgroup per tile of (16 R) x (16 R) pixels, R in {1, 2}: lane (tx, ty) owns the R x R pixels
// (x0 + 16 i + tx, y0 + 16 j + ty).  The grid vertices a tile can reach form a box ("slab") of nx x ny x L vertices x 12 channels; a
// pixel's x and y cells come from cell_of(), which host and device evaluate in the same float32 operations, so the host sizes the LDS by
// the largest slab any tile has and every workgroup finds its own box from its first and last pixel (cell_of is monotone).
//   backward, slab in LDS  : lanes of a wave that share a cell sum their 96 contributions in registers (scatter_wave), the sums are LDS
//                            float atomics into the slab; after a barrier every touched slab element leaves as ONE global float atomic.
//                            At 512 x 512 on a 16 x 16 x 8 grid a 16-pixel tile reaches 3 x 3 x 8 vertices (3.4 KB), a 16 x 16 image
//                            the whole 96 KB grid.
//   backward, no slab      : where the slab does not fit SLAB_MAX_BYTES the same sums are global float atomics of their own.
//   vertex reads           : forward and backward read the grid from a copy of the slab staged in LDS while slab (+ copy) stays within
//                            STAGE_MAX_BYTES, else through L1 / L2.
// Scalars only: no float2 / float4 arithmetic (Makefile).
#include <math.h>
#include "raster_tile.h"
#include "../../include/gaussctrl_bilagrid.h"

namespace {

constexpr int NCH = 12;                       // the 3x4 transform
constexpr int VIEWS_PER_LAUNCH = 64;          // view indices travel as a kernel argument: the caller's array is host memory
constexpr int SLAB_MAX_BYTES = 128 << 10;     // of the 160 KB LDS of a gfx950 CU
#ifndef GC_BILAGRID_STAGE_MAX_BYTES            // A/B builds only (-DGC_BILAGRID_STAGE_MAX_BYTES=0: scripts/bench_bilagrid.py --ab-lib)
#define GC_BILAGRID_STAGE_MAX_BYTES (64 << 10)
#endif
// grid values are staged in LDS beside the work while all of it stays within this: measured faster than the same reads through L1 / L2
// at eight images (profiles/bilagrid_bench.txt), but not worth a CU's whole LDS
constexpr int STAGE_MAX_BYTES = GC_BILAGRID_STAGE_MAX_BYTES;
constexpr int MIN_BLOCKS_FOR_R2 = 512;        // 32 x 32 tiles only while they still make two workgroups per CU

struct Views { int v[VIEWS_PER_LAUNCH]; };

struct Shape {
    int H, W, GW, GH, L, R;
    float su, sv;                             // (GW - 1) / W, (GH - 1) / H
};

// cell and fraction of pixel p on an axis with G vertices: the same float32 operations on the host (slab sizing) and on the device
__host__ __device__ inline int cell_of(int p, float s, int G, float &f)
{
    const float u = ((float)p + 0.5f) * s;
    int i = (int)u;                           // u >= 0: truncation is floor
    i = i > G - 2 ? G - 2 : i;
    f = u - (float)i;
    return i;
}

struct Pix {
    int xi, yi, zi;
    float fx, fy, fz;
    float zs;                                 // d z / d luma: L - 1, or 0 where the clamp is active
};

__device__ inline Pix locate(const Shape &sh, int x, int y, float r, float g, float b)
{
    Pix p;
    p.xi = cell_of(x, sh.su, sh.GW, p.fx);
    p.yi = cell_of(y, sh.sv, sh.GH, p.fy);
    const float luma = 0.299f * r + 0.587f * g + 0.114f * b;
    const float lm = (float)(sh.L - 1);
    p.zs = (luma > 0.f && luma < 1.f) ? lm : 0.f;
    const float z = fminf(fmaxf(luma, 0.f), 1.f) * lm;
    int zi = (int)z;
    zi = zi > sh.L - 2 ? sh.L - 2 : zi;
    p.zi = zi;
    p.fz = z - (float)zi;
    return p;
}

// the box of grid cells a tile's pixels fall into, from its first and last pixel (cell_of is monotone in p)
struct Box { int cx0, cy0, nx, ny; };

__host__ __device__ inline Box tile_box(const Shape &sh, int x0, int y0)
{
    const int T = 16 * sh.R;
    const int x1 = (x0 + T < sh.W ? x0 + T : sh.W) - 1, y1 = (y0 + T < sh.H ? y0 + T : sh.H) - 1;
    float f;
    Box b;
    b.cx0 = cell_of(x0, sh.su, sh.GW, f);
    b.cy0 = cell_of(y0, sh.sv, sh.GH, f);
    b.nx = cell_of(x1, sh.su, sh.GW, f) - b.cx0 + 2;
    b.ny = cell_of(y1, sh.sv, sh.GH, f) - b.cy0 + 2;
    return b;
}

// where a pixel's 8 vertices lie in an array of 12 channel planes: offset of vertex (0, 0, 0) and the three strides
struct Corner { int base, sy, sz, sk; };

__device__ inline Corner corner_global(const Shape &sh, const Pix &p)
{
    return {(p.zi * sh.GH + p.yi) * sh.GW + p.xi, sh.GW, sh.GH * sh.GW, sh.L * sh.GH * sh.GW};
}

__device__ inline Corner corner_slab(const Shape &sh, const Box &b, const Pix &p)
{
    return {(p.zi * b.ny + (p.yi - b.cy0)) * b.nx + (p.xi - b.cx0), b.nx, b.ny * b.nx, sh.L * b.ny * b.nx};
}

__device__ inline void weights(const Pix &p, float (&w)[8])
{
    const float x0 = 1.f - p.fx, y0 = 1.f - p.fy, z0 = 1.f - p.fz;
    w[0] = z0 * y0 * x0; w[1] = z0 * y0 * p.fx; w[2] = z0 * p.fy * x0; w[3] = z0 * p.fy * p.fx;
    w[4] = p.fz * y0 * x0; w[5] = p.fz * y0 * p.fx; w[6] = p.fz * p.fy * x0; w[7] = p.fz * p.fy * p.fx;
}

__device__ inline void offsets(const Corner &c, int (&o)[8])
{
#pragma unroll
    for (int v = 0; v < 8; ++v) o[v] = c.base + (v >> 2) * c.sz + ((v >> 1) & 1) * c.sy + (v & 1);
}

// slab element e (channel-major, then z, y, x inside the box) -> its element in the view's grid
__device__ inline int slab_to_grid(const Shape &sh, const Box &b, int e)
{
    const int sx = e % b.nx;
    int t = e / b.nx;
    const int sy = t % b.ny;
    t /= b.ny;                                // t = k * L + l
    return (t * sh.GH + (b.cy0 + sy)) * sh.GW + b.cx0 + sx;
}

template <bool STAGE>
__global__ __launch_bounds__(BLOCK) void k_bilagrid_slice_fwd(Shape sh, Views views, int c0, const float *__restrict__ grids,
                                                              const float *__restrict__ rgb, float *__restrict__ out)
{
    extern __shared__ float slab[];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int T = 16 * sh.R, x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int64_t cells = (int64_t)sh.L * sh.GH * sh.GW;
    const float *gv = grids + (int64_t)views.v[blockIdx.z] * NCH * cells;
    const int64_t img = (int64_t)(c0 + (int)blockIdx.z) * sh.H * sh.W;
    Box box = {0, 0, 0, 0};
    if (STAGE) {
        box = tile_box(sh, x0, y0);
        const int n = NCH * sh.L * box.ny * box.nx;
        for (int e = tid; e < n; e += BLOCK) slab[e] = gv[slab_to_grid(sh, box, e)];
        __syncthreads();
    }
    for (int j = 0; j < sh.R; ++j)
        for (int i = 0; i < sh.R; ++i) {
            const int x = x0 + 16 * i + tx, y = y0 + 16 * j + ty;
            if (x >= sh.W || y >= sh.H) continue;
            const int64_t px = (img + (int64_t)y * sh.W + x) * 3;
            const float r = rgb[px], g = rgb[px + 1], b = rgb[px + 2];
            const Pix p = locate(sh, x, y, r, g, b);
            const Corner cn = STAGE ? corner_slab(sh, box, p) : corner_global(sh, p);
            float w[8];
            int o[8];
            weights(p, w);
            offsets(cn, o);
            float A[NCH];
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                float a = 0.f;
#pragma unroll
                for (int v = 0; v < 8; ++v) a += w[v] * (STAGE ? slab[o[v] + k * cn.sk] : gv[o[v] + (int64_t)k * cn.sk]);
                A[k] = a;
            }
            out[px] = A[0] * r + A[1] * g + A[2] * b + A[3];
            out[px + 1] = A[4] * r + A[5] * g + A[6] * b + A[7];
            out[px + 2] = A[8] * r + A[9] * g + A[10] * b + A[11];
        }
}

// accumulation targets of the backward
enum { ACC_GLOBAL = 0,      // no slab fits: float atomics straight into v_grids
       ACC_SLAB = 1,        // the slab of sums in LDS, vertex reads through L1 / L2
       ACC_SLAB_STAGED = 2  // and the slab of grid values staged beside it
};

// One add into the accumulation target (LDS slab or the view's gradient grid).
template <int MODE>
__device__ __forceinline__ void acc_add(float *acc, int idx, float x)
{
    if (MODE == ACC_GLOBAL) unsafeAtomicAdd(acc + idx, x);
    else __hip_atomic_fetch_add(acc + idx, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The 96 contributions w[v] * va[k] of every active lane of a wave, added at (its cell's base) + (corner v) + k * sk.
// An LDS float atomic costs a few cycles per LANE (measured: 64 lanes on one address, the common case of a smooth image, and 64 lanes on
// scattered addresses differ by 1.5 x only), so lanes that share a cell are summed in registers first: the leader's cell is broadcast,
// its lanes' contributions of one corner go through row_sum (raster_tile.h), lane column k keeps channel k, xor_rows_sum adds the four
// rows, and lanes 0..11 issue ONE atomic each -- 8 atomic instructions of 12 lanes per cell instead of 96 of up to 64.  After
// MAX_CELLS_PER_WAVE cells (a noisy image) the lanes that are left add for themselves.  Every lane of the wave must call this (the DPP
// and lane-swap steps read all lanes); inactive lanes carry zeros.
constexpr int MAX_CELLS_PER_WAVE = 8;

template <int MODE>
__device__ __forceinline__ void scatter_wave(float *acc, bool active, int cell, const Corner ca, const float (&w)[8], const float (&va)[NCH])
{
    const int lane = threadIdx.x & 63, col = lane & 15;
    bool pending = active;
    for (int round = 0;; ++round) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;
        if (round == MAX_CELLS_PER_WAVE) {
            if (pending) {
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    const int o = ca.base + (v >> 2) * ca.sz + ((v >> 1) & 1) * ca.sy + (v & 1);
#pragma unroll
                    for (int k = 0; k < NCH; ++k) acc_add<MODE>(acc, o + k * ca.sk, w[v] * va[k]);
                }
            }
            break;
        }
        const int leader = __builtin_ctzll(m);
        const int cell0 = __builtin_amdgcn_readlane(cell, leader), base0 = __builtin_amdgcn_readlane(ca.base, leader);
        const bool mine = pending && cell == cell0;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const float wm = mine ? w[v] : 0.f;
            float y = 0.f;
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const float x = row_sum(wm * va[k]);
                y = col == k ? x : y;
            }
            y = xor_rows_sum(y);
            if (lane < NCH && y != 0.f) acc_add<MODE>(acc, base0 + (v >> 2) * ca.sz + ((v >> 1) & 1) * ca.sy + (v & 1) + lane * ca.sk, y);
        }
        pending = pending && !mine;
    }
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_bilagrid_slice_bwd(Shape sh, Views views, int c0, const float *__restrict__ grids,
                                                              const float *__restrict__ rgb, const float *__restrict__ v_out,
                                                              float *__restrict__ v_grids, float *__restrict__ v_rgb)
{
    extern __shared__ float slab[];                                      // [n_slab] sums, then (ACC_SLAB_STAGED) [n_slab] grid values
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int T = 16 * sh.R, x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int64_t cells = (int64_t)sh.L * sh.GH * sh.GW;
    const int64_t view_off = (int64_t)views.v[blockIdx.z] * NCH * cells;
    const float *gv = grids + view_off;
    float *vg = v_grids + view_off;
    const int64_t img = (int64_t)(c0 + (int)blockIdx.z) * sh.H * sh.W;
    Box box = {0, 0, 0, 0};
    int n_slab = 0;
    if (MODE != ACC_GLOBAL) {
        box = tile_box(sh, x0, y0);
        n_slab = NCH * sh.L * box.ny * box.nx;
        for (int e = tid; e < n_slab; e += BLOCK) {
            slab[e] = 0.f;
            if (MODE == ACC_SLAB_STAGED) slab[n_slab + e] = gv[slab_to_grid(sh, box, e)];
        }
        __syncthreads();
    }
    const float *gs = slab + n_slab;
    float *acc = MODE == ACC_GLOBAL ? vg : slab;
    for (int j = 0; j < sh.R; ++j)
        for (int i = 0; i < sh.R; ++i) {
            const int x = x0 + 16 * i + tx, y = y0 + 16 * j + ty;
            const bool active = x < sh.W && y < sh.H;                    // (no lane leaves: the wave reduces together)
            float w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float va[NCH] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            // the accumulation target's strides are the workgroup's: lanes 0..11 add a cell's sums even where their own pixel is outside
            Corner ca = MODE != ACC_GLOBAL ? Corner{0, box.nx, box.ny * box.nx, sh.L * box.ny * box.nx}
                                           : Corner{0, sh.GW, sh.GH * sh.GW, sh.L * sh.GH * sh.GW};
            int cell = -1;
            if (active) {
                const int64_t px = (img + (int64_t)y * sh.W + x) * 3;
                const float r = rgb[px], g = rgb[px + 1], b = rgb[px + 2];
                const float vo0 = v_out[px], vo1 = v_out[px + 1], vo2 = v_out[px + 2];
                const Pix p = locate(sh, x, y, r, g, b);
                const Corner cg = corner_global(sh, p);
                const Corner cs = MODE != ACC_GLOBAL ? corner_slab(sh, box, p) : cg;
                const Corner cr = MODE == ACC_SLAB_STAGED ? cs : cg;     // where the vertex values are read
                ca.base = cs.base;
                cell = cg.base;
                int o[8];
                weights(p, w);
                offsets(cr, o);
                const float x0w = 1.f - p.fx, y0w = 1.f - p.fy;
                const float wxy[4] = {y0w * x0w, y0w * p.fx, p.fy * x0w, p.fy * p.fx};
                float t0 = 0.f, t1 = 0.f, t2 = 0.f, zt = 0.f;
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const int ch = k & 3, row = k >> 2;
                    const float vo = row == 0 ? vo0 : row == 1 ? vo1 : vo2;
                    va[k] = vo * (ch == 0 ? r : ch == 1 ? g : ch == 2 ? b : 1.f);             // v_A[k]
                    float gk[8];
#pragma unroll
                    for (int v = 0; v < 8; ++v) gk[v] = MODE == ACC_SLAB_STAGED ? gs[o[v] + k * cr.sk] : gv[o[v] + (int64_t)k * cr.sk];
                    float dadz = 0.f;
#pragma unroll
                    for (int v = 0; v < 4; ++v) dadz += wxy[v] * (gk[v + 4] - gk[v]);
                    zt += va[k] * dadz;
                    if (ch < 3) {
                        float a = 0.f;
#pragma unroll
                        for (int v = 0; v < 8; ++v) a += w[v] * gk[v];
                        if (ch == 0) t0 += a * vo; else if (ch == 1) t1 += a * vo; else t2 += a * vo;
                    }
                }
                zt *= p.zs;
                v_rgb[px] = t0 + 0.299f * zt;
                v_rgb[px + 1] = t1 + 0.587f * zt;
                v_rgb[px + 2] = t2 + 0.114f * zt;
            }
            scatter_wave<MODE>(acc, active, cell, ca, w, va);
        }
    if (MODE != ACC_GLOBAL) {
        __syncthreads();
        for (int e = tid; e < n_slab; e += BLOCK) {                      // one global atomic per touched grid element and workgroup
            const float s = slab[e];
            if (s != 0.f) unsafeAtomicAdd(vg + slab_to_grid(sh, box, e), s);
        }
    }
}

__device__ inline double block_sum(double v, double *sh4)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}

// one lane per grid element: its share of the three sums of squared forward differences (the differences it starts), and the gradient
// it receives from the differences it starts and ends
__global__ __launch_bounds__(BLOCK) void k_bilagrid_tv(int n, int GW, int GH, int L, const float *__restrict__ g, float weight, double dx,
                                                       double dy, double dz, float *__restrict__ v_grids, double *__restrict__ partial)
{
    __shared__ double sh4[4];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double val = 0.0;                                                     // the value in double: 1 / count per axis (dx, dy, dz) is not a float
    if (i < n) {
        const int x = i % GW, y = (i / GW) % GH, z = (i / (GW * GH)) % L;
        const int sy = GW, sz = GW * GH;
        const float cx = (float)dx, cy = (float)dy, cz = (float)dz;
        const float c = g[i];
        float grad = 0.f;
        if (x + 1 < GW) { const float d = g[i + 1] - c; val += dx * ((double)d * (double)d); grad -= cx * d; }
        if (x > 0) grad += cx * (c - g[i - 1]);
        if (y + 1 < GH) { const float d = g[i + sy] - c; val += dy * ((double)d * (double)d); grad -= cy * d; }
        if (y > 0) grad += cy * (c - g[i - sy]);
        if (z + 1 < L) { const float d = g[i + sz] - c; val += dz * ((double)d * (double)d); grad -= cz * d; }
        if (z > 0) grad += cz * (c - g[i - sz]);
        v_grids[i] += weight * 2.f * grad;
    }
    const double s = block_sum(val, sh4);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the per-workgroup partials in a fixed order: the same bits every run
__global__ __launch_bounds__(BLOCK) void k_bilagrid_tv_sum(int nb, const double *__restrict__ partial, float *__restrict__ tv)
{
    __shared__ double sh4[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += BLOCK) s += partial[i];
    s = block_sum(s, sh4);
    if (threadIdx.x == 0) tv[0] = (float)s;
}

gc::AttrOnce g_bwd_lds;

struct Plan {
    Shape sh;
    int tiles_x, tiles_y;
    int slab_bytes;                           // the largest slab of any tile
};

Plan plan_for(int H, int W, int GW, int GH, int L, int R)
{
    Plan p;
    p.sh = {H, W, GW, GH, L, R, (float)(GW - 1) / (float)W, (float)(GH - 1) / (float)H};
    const int T = 16 * R;
    p.tiles_x = (W + T - 1) / T;
    p.tiles_y = (H + T - 1) / T;
    int nx = 2, ny = 2;
    for (int t = 0; t < p.tiles_x; ++t) { const Box b = tile_box(p.sh, t * T, 0); nx = b.nx > nx ? b.nx : nx; }
    for (int t = 0; t < p.tiles_y; ++t) { const Box b = tile_box(p.sh, 0, t * T); ny = b.ny > ny ? b.ny : ny; }
    const int64_t bytes = (int64_t)NCH * L * ny * nx * 4;
    p.slab_bytes = bytes > (int64_t)1 << 30 ? 1 << 30 : (int)bytes;
    return p;
}

// tile and slab policy, from the shapes: 32 x 32 tiles (a quarter of the flushes per pixel) while they still make MIN_BLOCKS_FOR_R2
// workgroups and their slab fits, else 16 x 16 tiles; slab_bytes > SLAB_MAX_BYTES in the result means no tile's slab fits
Plan choose_plan(int C, int H, int W, int GW, int GH, int L)
{
    const Plan p2 = plan_for(H, W, GW, GH, L, 2);
    if ((int64_t)C * p2.tiles_x * p2.tiles_y >= MIN_BLOCKS_FOR_R2 && p2.slab_bytes <= SLAB_MAX_BYTES) return p2;
    return plan_for(H, W, GW, GH, L, 1);
}

int check_slice(const char *fn, int C, int H, int W, int V, int GW, int GH, int L, const int32_t *view_idx)
{
    if (C < 1 || H < 1 || W < 1 || V < 1) { gc::set_error("%s: C, H, W and V must be at least 1", fn); return GC_EINVAL; }
    if (GW < 2 || GH < 2 || L < 2) { gc::set_error("%s: every grid dimension must be at least 2", fn); return GC_EINVAL; }
    if ((int64_t)C * H * W * 3 >= (1ll << 31) || (int64_t)V * NCH * L * GH * GW >= (1ll << 31)) {
        gc::set_error("%s: 2^31 elements or more", fn);
        return GC_EINVAL;
    }
    if ((H + 15) / 16 > 65535) { gc::set_error("%s: more than 65535 rows of 16-pixel tiles", fn); return GC_EINVAL; }      // gridDim.y
    if (!view_idx) { gc::set_error("%s: null argument", fn); return GC_EINVAL; }
    for (int c = 0; c < C; ++c)
        if (view_idx[c] < 0 || view_idx[c] >= V) { gc::set_error("%s: view_idx[%d] = %d is outside [0, %d)", fn, c, view_idx[c], V); return GC_EINVAL; }
    return GC_OK;
}

}  // namespace

extern "C" {

int gcx_bilagrid_slice_fwd_views(int C, int H, int W, int V, int GW, int GH, int L, const float *grids, const float *rgb,
                                 const int32_t *view_idx, float *out, void *stream)
{
    if (const int rc = check_slice(__func__, C, H, W, V, GW, GH, L, view_idx)) return rc;
    GC_REQUIRE(grids && rgb && out, "null argument");
    const Plan p = choose_plan(C, H, W, GW, GH, L);
    const bool stage = p.slab_bytes <= STAGE_MAX_BYTES;              // (at most 64 KB: no attribute needed)
    for (int c0 = 0; c0 < C; c0 += VIEWS_PER_LAUNCH) {
        const int nc = C - c0 < VIEWS_PER_LAUNCH ? C - c0 : VIEWS_PER_LAUNCH;
        Views vs = {};
        for (int c = 0; c < nc; ++c) vs.v[c] = view_idx[c0 + c];
        const dim3 grid(p.tiles_x, p.tiles_y, nc);
        if (stage) hipLaunchKernelGGL(k_bilagrid_slice_fwd<true>, grid, dim3(BLOCK), p.slab_bytes, gc::S(stream), p.sh, vs, c0, grids, rgb, out);
        else hipLaunchKernelGGL(k_bilagrid_slice_fwd<false>, grid, dim3(BLOCK), 0, gc::S(stream), p.sh, vs, c0, grids, rgb, out);
        if (const int rc = gc::check_launch(__func__)) return rc;
    }
    return GC_OK;
}

int gcx_bilagrid_slice_bwd_views(int C, int H, int W, int V, int GW, int GH, int L, const float *grids, const float *rgb,
                                 const int32_t *view_idx, const float *v_out, float *v_grids, float *v_rgb, void *stream)
{
    if (const int rc = check_slice(__func__, C, H, W, V, GW, GH, L, view_idx)) return rc;
    GC_REQUIRE(grids && rgb && v_out && v_grids && v_rgb, "null argument");
    const Plan p = choose_plan(C, H, W, GW, GH, L);
    const int mode = 2 * (int64_t)p.slab_bytes <= STAGE_MAX_BYTES ? ACC_SLAB_STAGED : p.slab_bytes <= SLAB_MAX_BYTES ? ACC_SLAB : ACC_GLOBAL;
    if (mode == ACC_SLAB) gc::ensure_dynamic_lds(g_bwd_lds, (const void *)k_bilagrid_slice_bwd<ACC_SLAB>, SLAB_MAX_BYTES);
    for (int c0 = 0; c0 < C; c0 += VIEWS_PER_LAUNCH) {
        const int nc = C - c0 < VIEWS_PER_LAUNCH ? C - c0 : VIEWS_PER_LAUNCH;
        Views vs = {};
        for (int c = 0; c < nc; ++c) vs.v[c] = view_idx[c0 + c];
        const dim3 grid(p.tiles_x, p.tiles_y, nc);
        if (mode == ACC_SLAB_STAGED)
            hipLaunchKernelGGL(k_bilagrid_slice_bwd<ACC_SLAB_STAGED>, grid, dim3(BLOCK), 2 * p.slab_bytes, gc::S(stream), p.sh, vs, c0, grids, rgb,
                               v_out, v_grids, v_rgb);
        else if (mode == ACC_SLAB)
            hipLaunchKernelGGL(k_bilagrid_slice_bwd<ACC_SLAB>, grid, dim3(BLOCK), p.slab_bytes, gc::S(stream), p.sh, vs, c0, grids, rgb, v_out,
                               v_grids, v_rgb);
        else
            hipLaunchKernelGGL(k_bilagrid_slice_bwd<ACC_GLOBAL>, grid, dim3(BLOCK), 0, gc::S(stream), p.sh, vs, c0, grids, rgb, v_out, v_grids,
                               v_rgb);
        if (const int rc = gc::check_launch(__func__)) return rc;
    }
    return GC_OK;
}

size_t gcx_bilagrid_tv_workspace_bytes(int V, int GW, int GH, int L)
{
    if (V < 1 || GW < 2 || GH < 2 || L < 2) return 256;
    const int64_t n = (int64_t)V * NCH * L * GH * GW;
    if (n >= (1ll << 31)) return 256;
    return (size_t)((((n + BLOCK - 1) / BLOCK) * 8 + 255) & ~(int64_t)255);
}

int gcx_bilagrid_tv_fwd_bwd(int V, int GW, int GH, int L, const float *grids, float weight, float *tv, float *v_grids, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    GC_REQUIRE(V >= 0, "V must not be negative");
    GC_REQUIRE(GW >= 2 && GH >= 2 && L >= 2, "every grid dimension must be at least 2");
    const int64_t n = (int64_t)V * NCH * L * GH * GW;
    GC_REQUIRE(n < (1ll << 31), "2^31 elements or more");
    if (V == 0) return GC_OK;
    GC_REQUIRE(grids && tv && v_grids && workspace, "null argument");
    GC_REQUIRE(weight == weight, "weight must not be NaN");
    GC_REQUIRE(workspace_bytes >= gcx_bilagrid_tv_workspace_bytes(V, GW, GH, L) && ((uintptr_t)workspace & 7) == 0,
               "workspace too small or not 8-byte aligned");
    const double planes = (double)V * NCH;
    const double cx = 1.0 / (planes * L * GH * (GW - 1)), cy = 1.0 / (planes * L * (GH - 1) * GW), cz = 1.0 / (planes * (L - 1) * GH * GW);
    const int nb = (int)((n + BLOCK - 1) / BLOCK);
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(k_bilagrid_tv, dim3(nb), dim3(BLOCK), 0, gc::S(stream), (int)n, GW, GH, L, grids, weight, cx, cy, cz, v_grids, partial);
    if (const int rc = gc::check_launch(__func__)) return rc;
    hipLaunchKernelGGL(k_bilagrid_tv_sum, dim3(1), dim3(BLOCK), 0, gc::S(stream), nb, partial, tv);
    return gc::check_launch(__func__);
}

}  // extern "C"

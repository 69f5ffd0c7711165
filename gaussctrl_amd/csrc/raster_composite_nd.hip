// raster_composite_nd.hip -- per-tile alpha compositing of colors[N][C] for any channel count C >= 1 (forward + backward) for gfx950.
//
// gsplat 0.1.3's rasterize_gaussians sends C == 3 to rasterize_forward (raster_composite.hip) and every other count to
// nd_rasterize_forward / nd_rasterize_backward: these are the latter.  Same semantics as the 3-channel kernels (SURVEY.md Appendix
// A.4 / A.5) and the same structure: one 16x16 tile per 256-lane workgroup, one wave per 8x8 pixel block, the depth-sorted list staged
// through LDS in batches of 256 splats with the exact per-block culling mask (raster_tile.h), a scalar walk over the ballot of the
// wave's block.  The per-pixel alpha / T / stop arithmetic is the 3-channel kernel's, so final_Ts and final_index are bit-identical.
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
#include "raster_tile.h"

namespace {

constexpr int CH_MAX = 32;

struct SplatQ { float cxy, cyy; };

__device__ __forceinline__ void stage_geometry(int gid, const float *__restrict__ xys, const float *__restrict__ conics,
                                               const float *__restrict__ opacities, SplatA &a, SplatQ &q, unsigned &mk, float tx0, float ty0)
{
    const float2 xy = *reinterpret_cast<const float2 *>(xys + 2 * (int64_t)gid);
    const float c0 = conics[3 * (int64_t)gid], c1 = conics[3 * (int64_t)gid + 1], c2 = conics[3 * (int64_t)gid + 2];
    const float op = opacities[gid];
    a = {xy.x, xy.y, op, c0};
    q = {c1, c2};
    mk = block_mask(xy.x, xy.y, op, c0, c1, c2, tx0, ty0);
}

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
    const int tile = blockIdx.y * tiles_x + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int j = blockIdx.x * TILE + 8 * (wid & 1) + (lane & 7);       // wave = one 8x8 pixel block of the tile
    const int i = blockIdx.y * TILE + 8 * (wid >> 1) + (lane >> 3);
    const bool inside = (i < H) && (j < W);
    const float px = (float)j, py = (float)i;
    const float tx0 = (float)(blockIdx.x * TILE), ty0 = (float)(blockIdx.y * TILE);
    const int start = tile_bins[2 * tile], end = tile_bins[2 * tile + 1];
    bool done = !inside;
    float T = 1.f;
    float acc[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) acc[k] = 0.f;
    int last = 0;
    for (int bs = start; bs < end; bs += BLOCK) {
        if (__syncthreads_and(done)) break;
        const int idx = bs + tid;
        unsigned mk = 0;
        int gid = 0;
        if (idx < end) {
            gid = ids_sorted[idx];
            stage_geometry(gid, xys, conics, opacities, sA[tid], sQ[tid], mk, tx0, ty0);
        }
        sGid[tid] = gid;
        sMask[tid] = (unsigned char)mk;
        __syncthreads();
        const int n = min(BLOCK, end - bs);
        stage_colors<CH>(sCol, sGid, n, tid, colors, C, cb, nc);
        __syncthreads();
        bool wave_done = __all(done);                                  // a finished wave only helps staging
        for (int c = 0; c * 64 < n && !wave_done; ++c) {
            unsigned long long bal = __ballot((sMask[c * 64 + lane] >> wid) & 1);
            while (bal) {                                              // scalar walk over the splats that can touch this block
                const int t = c * 64 + __builtin_ctzll(bal);
                bal &= bal - 1;
                const SplatA a = sA[t];
                const SplatQ q = sQ[t];
                const float dx = a.x - px, dy = a.y - py;
                const float sigma = 0.5f * (a.cxx * dx * dx + q.cyy * dy * dy) + q.cxy * dx * dy;
                const float alpha = fminf(ALPHA_CAP, a.opac * __expf(-sigma));
                const bool hit = !done && !(sigma < 0.f || alpha < ALPHA_MIN);
                const float next_T = T * (1.f - alpha);
                const bool stop = hit && next_T <= T_STOP;
                const bool add = hit && !stop;
                const float vis = add ? alpha * T : 0.f;
                const float *col = sCol + t * CH;
#pragma unroll
                for (int k = 0; k < CH; ++k) acc[k] += col[k] * vis;
                T = add ? next_T : T;
                last = add ? bs + t : last;
                done |= stop;
                if (__all(done)) { wave_done = true; break; }
            }
        }
    }
    if (inside) {
        const int pix = i * W + j;
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
    const int tile = blockIdx.y * tiles_x + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int j = blockIdx.x * TILE + 8 * (wid & 1) + (lane & 7);       // wave = one 8x8 pixel block of the tile
    const int i = blockIdx.y * TILE + 8 * (wid >> 1) + (lane >> 3);
    const bool inside = (i < H) && (j < W);
    const float px = (float)j, py = (float)i;
    const float tx0 = (float)(blockIdx.x * TILE), ty0 = (float)(blockIdx.y * TILE);
    const int start = tile_bins[2 * tile], end = tile_bins[2 * tile + 1];
    if (end <= start) return;
    const int pix = inside ? i * W + j : 0;
    const float T_final = inside ? final_Ts[pix] : 1.f;
    float T = T_final;
    const int bin_final = inside ? final_index[pix] : -1;
    float vo[CH], S[CH];
    float voa = 0.f, bgdot = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        vo[k] = inside && k < nc ? v_out[(int64_t)pix * C + cb + k] : 0.f;
        S[k] = 0.f;
        if (k < nc) bgdot += background[cb + k] * vo[k];
    }
    if (inside && cb == 0 && v_out_alpha) voa = v_out_alpha[pix];
    // wave / workgroup maxima of final_index: nothing beyond them was composited
    int wmax = bin_final;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d, 64));
    wmax = __builtin_amdgcn_readfirstlane(wmax);                       // wave-uniform: keeps the splat walk below in scalar registers
    if (lane == 0) sMax[wid] = wmax;
#pragma unroll
    for (int q = 0; q < NQ; ++q) sG[q * BLOCK + tid] = 0.f;
    __syncthreads();
    const int kmax = __builtin_amdgcn_readfirstlane(max(max(sMax[0], sMax[1]), max(sMax[2], sMax[3])));
    if (kmax < start) return;
    const int col16 = lane & 15;
    for (int batch_end = kmax; batch_end >= start; batch_end -= BLOCK) {
        const int idx = batch_end - tid;
        int gid = -1;
        unsigned mk = 0;
        if (idx >= start) {
            gid = ids_sorted[idx];
            stage_geometry(gid, xys, conics, opacities, sA[tid], sQ[tid], mk, tx0, ty0);
        }
        sGid[tid] = gid;
        sMask[tid] = (unsigned char)mk;
        __syncthreads();
        const int n = min(BLOCK, batch_end - start + 1);
        stage_colors<CH>(sCol, sGid, n, tid, colors, C, cb, nc);
        __syncthreads();
        const int t0 = max(0, batch_end - wmax);                       // wave-uniform: splats behind every pixel's last one
        for (int c = t0 >> 6; c * 64 < n; ++c) {
            unsigned long long bal = __ballot((sMask[c * 64 + lane] >> wid) & 1);
            if (c * 64 < t0) bal &= ~0ull << (t0 - c * 64);
            while (bal) {
                const int t = c * 64 + __builtin_ctzll(bal);
                bal &= bal - 1;
                const int k = batch_end - t;
                const SplatA a = sA[t];
                const SplatQ q = sQ[t];
                const float dx = a.x - px, dy = a.y - py;
                const float sigma = 0.5f * (a.cxx * dx * dx + q.cyy * dy * dy) + q.cxy * dx * dy;
                const float vis = __expf(-sigma);
                const float araw = a.opac * vis;
                const float alpha = fminf(ALPHA_CAP, araw);
                const bool valid = (k <= bin_final) && !(sigma < 0.f || alpha < ALPHA_MIN);
                if (!__any(valid)) continue;
                float g[NQ];
#pragma unroll
                for (int p = 0; p < NQ; ++p) g[p] = 0.f;
                if (valid) {
                    const float ra = __builtin_amdgcn_rcpf(1.f - alpha);      // 1-ulp reciprocal, as k_rasterize_bwd
                    T *= ra;
                    const float fac = alpha * T;
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
                    // alpha clamped at the cap passes no gradient to sigma / opacity
                    const float va = araw > ALPHA_CAP ? 0.f : vis * v_alpha;
                    const float v_sigma = -a.opac * va;
                    g[CH] = 0.5f * v_sigma * dx * dx;
                    g[CH + 1] = v_sigma * dx * dy;
                    g[CH + 2] = 0.5f * v_sigma * dy * dy;
                    g[CH + 3] = v_sigma * (a.cxx * dx + q.cxy * dy);
                    g[CH + 4] = v_sigma * (q.cxy * dx + q.cyy * dy);
                    g[CH + 5] = va;
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
            float v[NQ];
            bool any = false;
#pragma unroll
            for (int p = 0; p < NQ; ++p) { v[p] = sG[p * BLOCK + tid]; sG[p * BLOCK + tid] = 0.f; any |= v[p] != 0.f; }
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

int ch_for(int c) { return c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : c <= 8 ? 8 : c <= 16 ? 16 : 32; }

struct NdArgs {
    int H, W, tiles_x, tiles_y, C;
    const int32_t *ids, *bins;
    const float *xys, *conics, *colors, *opac, *bg;
};

template <int CH>
void launch_fwd(const NdArgs &a, int base, int chunks, float *out_img, float *final_Ts, int32_t *final_index, hipStream_t st)
{
    hipLaunchKernelGGL(k_rasterize_nd_fwd<CH>, dim3(a.tiles_x, a.tiles_y, chunks), dim3(BLOCK), 0, st, a.H, a.W, a.tiles_x, a.C, base,
                       a.ids, a.bins, a.xys, a.conics, a.colors, a.opac, a.bg, out_img, final_Ts, final_index);
}

template <int CH>
void launch_bwd(const NdArgs &a, int base, int chunks, const float *final_Ts, const int32_t *final_index, const float *v_out,
                const float *v_out_alpha, float *v_xy, float *v_conic, float *v_colors, float *v_opacity, hipStream_t st)
{
    hipLaunchKernelGGL(k_rasterize_nd_bwd<CH>, dim3(a.tiles_x, a.tiles_y, chunks), dim3(BLOCK), 0, st, a.H, a.W, a.tiles_x, a.C, base,
                       a.ids, a.bins, a.xys, a.conics, a.colors, a.opac, a.bg, final_Ts, final_index, v_out, v_out_alpha, v_xy, v_conic,
                       v_colors, v_opacity);
}

// the launches of one pass: C / 32 chunks of 32 channels when C > 32, then one chunk of the smallest CH >= the channels left
template <typename F>
void for_each_launch(int C, F &&f)
{
    const int full = C > CH_MAX ? C / CH_MAX : 0, rest = C - full * CH_MAX;
    if (full) f(CH_MAX, 0, full);
    if (rest) f(ch_for(rest), full * CH_MAX, 1);
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
    GC_REQUIRE(img_h > 0 && img_w > 0 && tiles_x == (img_w + TILE - 1) / TILE && tiles_y == (img_h + TILE - 1) / TILE,
               "tile bounds do not match the image size");
    const NdArgs a{img_h, img_w, tiles_x, tiles_y, channels, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background};
    hipStream_t st = gc::S(stream);
    for_each_launch(channels, [&](int ch, int base, int chunks) {
        switch (ch) {
        case 1: launch_fwd<1>(a, base, chunks, out_img, final_Ts, final_index, st); break;
        case 2: launch_fwd<2>(a, base, chunks, out_img, final_Ts, final_index, st); break;
        case 4: launch_fwd<4>(a, base, chunks, out_img, final_Ts, final_index, st); break;
        case 8: launch_fwd<8>(a, base, chunks, out_img, final_Ts, final_index, st); break;
        case 16: launch_fwd<16>(a, base, chunks, out_img, final_Ts, final_index, st); break;
        default: launch_fwd<32>(a, base, chunks, out_img, final_Ts, final_index, st); break;
        }
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
    GC_REQUIRE(img_h > 0 && img_w > 0 && tiles_x == (img_w + TILE - 1) / TILE && tiles_y == (img_h + TILE - 1) / TILE,
               "tile bounds do not match the image size");
    const NdArgs a{img_h, img_w, tiles_x, tiles_y, channels, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background};
    hipStream_t st = gc::S(stream);
    for_each_launch(channels, [&](int ch, int base, int chunks) {
        switch (ch) {
        case 1: launch_bwd<1>(a, base, chunks, final_Ts, final_index, v_out, v_out_alpha, v_xy, v_conic, v_colors, v_opacity, st); break;
        case 2: launch_bwd<2>(a, base, chunks, final_Ts, final_index, v_out, v_out_alpha, v_xy, v_conic, v_colors, v_opacity, st); break;
        case 4: launch_bwd<4>(a, base, chunks, final_Ts, final_index, v_out, v_out_alpha, v_xy, v_conic, v_colors, v_opacity, st); break;
        case 8: launch_bwd<8>(a, base, chunks, final_Ts, final_index, v_out, v_out_alpha, v_xy, v_conic, v_colors, v_opacity, st); break;
        case 16: launch_bwd<16>(a, base, chunks, final_Ts, final_index, v_out, v_out_alpha, v_xy, v_conic, v_colors, v_opacity, st); break;
        default: launch_bwd<32>(a, base, chunks, final_Ts, final_index, v_out, v_out_alpha, v_xy, v_conic, v_colors, v_opacity, st); break;
        }
    });
    return gc::check_launch("gc_rasterize_nd_bwd");
}

}  // extern "C"

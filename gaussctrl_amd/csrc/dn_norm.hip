// dn_norm.hip -- HBM-bound normalisation / elementwise kernels of the SD1.5 UNet / ControlNet / VAE on
// NHWC ("tokens x channels") bf16/f16 tensors (gfx950).  Replaces torch.nn.GroupNorm / LayerNorm / SiLU /
// cat / add and the scheduler + CFG arithmetic diffusers runs for
// gaussctrl/gc_pipeline.py:142-145,209-219 of the reference.
//
// All kernels move 16 bytes per lane per access, statistics in fp32.
//
// GroupNorm    k_gn_partial + k_gn_finalize + k_gn_apply (stand-alone, three launches), k_gn_small (one launch, small maps),
//              k_gn_apply_stats<T, Q8> (from the producer's per-group sums), k_gn_apply_parts<T, Q8> / k_gn_coef_parts (from the
//              producer's slab partials); Q8 = e4m3 output
// LayerNorm    k_layernorm<T, Q8>
// concat       k_concat_add, k_concat_add_stats (+ group sums, atomics), k_concat_add_parts (+ slab partials, plain stores)
// elementwise  k_axpby, k_cast_f32, k_softmax_rows, k_cfg_ddim, k_disp_max / k_disp_write, k_mask_composite
// Written once, used by the kernels above: affine8 / store8 (dn_common.h), gn_coef, SlabThread + slab_reduce16, concat_chunk.
#include "dn_common.h"

namespace {
using namespace dn;

// ------------------------------------------------------------------------------------------ shared pieces
// per-channel GroupNorm coefficients from a group's moments: y = x * a + d
__device__ __forceinline__ void gn_coef(float mean, float rstd, float gamma, float beta, float &a, float &d)
{
    a = rstd * gamma;
    d = beta - mean * a;
}

// 8 (a, d) pairs as stored ([c][2] floats, global or LDS) -> a[8], d[8]
__device__ __forceinline__ void load_coef8(const float *coef, float *a, float *d)
{
    const float4 *cf = reinterpret_cast<const float4 *>(coef);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 ab = cf[j];
        a[2 * j] = ab.x; d[2 * j] = ab.y; a[2 * j + 1] = ab.z; d[2 * j + 1] = ab.w;
    }
}

// Thread coordinates of the slab kernels: grid = (pixel slab, channel slice, batch), a workgroup covers `nchb` 16-byte channel chunks x
// `lanes` pixel lanes; a thread owns chunk `cch` (channels c0 .. c0 + 7) and walks the pixels p0 + pl, + lanes, ... < p1 of its slab.
// Threads with pl >= lanes (256 % nchb of them) are idle.
struct SlabThread {
    int nchb, lanes, cch, pl, c0, p0, p1;
    __device__ __forceinline__ SlabThread(int nchb_, int pix_per_block, int HW)
        : nchb(nchb_), lanes(256 / nchb_), cch((int)threadIdx.x % nchb_), pl((int)threadIdx.x / nchb_), c0((blockIdx.y * nchb_ + cch) * 8),
          p0(blockIdx.x * pix_per_block), p1(min(p0 + pix_per_block, HW)) {}
    __device__ __forceinline__ bool live() const { return pl < lanes; }
};

// per-channel (s1, s2) of every live thread -> sp[pl][cch][16] (interleaved), barrier, then pixel lane 0 adds up its column in the order
// l = 0 .. lanes - 1: acc[2 j] = sum s1[j], acc[2 j + 1] = sum s2[j] (acc is left untouched on the other lanes).  sp: [lanes][nchb][16] floats.
__device__ __forceinline__ void slab_reduce16(float *sp, const SlabThread &st, const float *s1, const float *s2, float *acc)
{
    if (st.live()) {
        float *o = sp + ((size_t)st.pl * st.nchb + st.cch) * 16;
#pragma unroll
        for (int j = 0; j < 8; ++j) { o[2 * j] = s1[j]; o[2 * j + 1] = s2[j]; }
    }
    __syncthreads();
    if (st.pl == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.f;
        for (int l = 0; l < st.lanes; ++l) {
            const float *o = sp + ((size_t)l * st.nchb + st.cch) * 16;
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += o[j];
        }
    }
}

// One 16-byte chunk of [a | b (+ c)]: v (and w = the chunk of c when `add`) -> the chunk as stored, f = its 8 values (after the
// rounding of b + c to T: statistics are taken of the values as stored)
template <class T>
__device__ __forceinline__ uint4 concat_combine(uint4 v, uint4 w, bool add, float *f)
{
    unpack8<T>(v, f);
    if (add) {
        float fc[8];
        unpack8<T>(w, fc);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] += fc[j];
        v = pack8<T>(f);
        unpack8<T>(v, f);
    }
    return v;
}

// the chunk at row m, channels c0 .. c0 + 7 of the concatenation (c may be null)
template <class T>
__device__ __forceinline__ uint4 concat_chunk(const unsigned short *__restrict__ a, int C1, const unsigned short *__restrict__ b,
                                              const unsigned short *__restrict__ c, int C2, size_t m, int c0, float *f)
{
    const uint4 none = make_uint4(0u, 0u, 0u, 0u);
    if (c0 < C1) return concat_combine<T>(*reinterpret_cast<const uint4 *>(a + m * C1 + c0), none, false, f);
    const uint4 v = *reinterpret_cast<const uint4 *>(b + m * C2 + (c0 - C1));
    if (!c) return concat_combine<T>(v, none, false, f);
    return concat_combine<T>(v, *reinterpret_cast<const uint4 *>(c + m * C2 + (c0 - C1)), true, f);
}

// ------------------------------------------------------------------------------------------ GroupNorm
// Three streaming kernels, no atomics, 32-bit index arithmetic:
//   k_gn_partial : per (batch, pixel slab <= 32 per image, channel slice) per-CHANNEL sums of (x - s_c) and (x - s_c)^2 with the
//                  per-channel shift s_c = x[b, pixel 0, c] (shifted sums: no catastrophic cancellation when |mean| >> std)
//   k_gn_finalize: per (batch, group): mean / rstd from the shifted channel sums -> per-channel scale a = rstd*gamma, d = beta - mean*a
//   k_gn_apply   : y = (x * a + d) [SiLU], 16 bytes per lane, coefficients from L1/L2
template <class T>
__global__ __launch_bounds__(256) void k_gn_partial(const unsigned short *__restrict__ x, int HW, int C, int nchb,
                                                    int pix_per_block, float *__restrict__ part)
{
    extern __shared__ float sp[];   // [lanes][nchb][16]
    const int b = blockIdx.z;
    const SlabThread st(nchb, pix_per_block, HW);
    const int c0 = st.c0;
    const unsigned short *xb = x + (size_t)b * HW * C;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    if (st.live()) {
        float sh[8];
        unpack8<T>(*reinterpret_cast<const uint4 *>(xb + c0), sh);
        for (int p = st.p0 + st.pl; p < st.p1; p += st.lanes) {
            float f[8];
            unpack8<T>(*reinterpret_cast<const uint4 *>(xb + (size_t)p * C + c0), f);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = f[j] - sh[j]; s1[j] += d; s2[j] += d * d; }
        }
    }
    float acc[16];
    slab_reduce16(sp, st, s1, s2, acc);
    if (st.pl == 0) {
        float *dst = part + (((size_t)b * gridDim.x + blockIdx.x) * C + c0) * 2;
#pragma unroll
        for (int j = 0; j < 16; j += 4) *reinterpret_cast<float4 *>(dst + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
    }
}

// one workgroup per (batch, group): channel c of the group is handled by lanes l = c - g*cpg (+ 256 k)
template <class T>
__global__ __launch_bounds__(256) void k_gn_finalize(const unsigned short *__restrict__ x, int HW, int C, int G, int nslab,
                                                     const float *__restrict__ part, const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, float eps, float *__restrict__ coef)
{
    __shared__ float red[3][4];
    const int b = blockIdx.x / G, gi = blockIdx.x % G, cpg = C / G, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // every thread: one (channel, slab-subset) share; totals per channel are combined with the channel's shift
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;        // sum x, sum (x-s)^2 parts folded below
    float cs1 = 0.f, cs2 = 0.f, sh = 0.f;
    const int ci = tid % cpg, sub = tid / cpg, nsub = 256 / cpg;   // cpg <= 256
    if (sub < nsub) {
        const int c = gi * cpg + ci;
        sh = T::to_f(x[(size_t)b * HW * C + c]);
        for (int sl = sub; sl < nslab; sl += nsub) {
            const float2 v = *reinterpret_cast<const float2 *>(part + (((size_t)b * nslab + sl) * C + c) * 2);
            cs1 += v.x; cs2 += v.y;
        }
        // this share covers n_s pixels (unknown here) -> keep moments about the shift; pixel counts are added in closed form
        t0 = cs1;                       // sum (x - s_c) over the share
        t1 = cs2;                       // sum (x - s_c)^2
        t2 = (sub == 0) ? sh : 0.f;     // s_c counted once per channel
    }
    // group mean: mu = (sum_c [S1_c + HW * s_c]) / (HW * cpg)
    float a0 = wave_sum_f(t0), a2 = wave_sum_f(t2);
    if (lane == 0) { red[0][wid] = a0; red[2][wid] = a2; }
    __syncthreads();
    const float S1 = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const float SS = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    const float n = (float)HW * (float)cpg;
    const float mu = (S1 + (float)HW * SS) / n;
    // variance: sum_c [S2_c + 2 (s_c - mu) S1_c + HW (s_c - mu)^2]: the last term once per channel
    float q = 0.f;
    if (sub < nsub) {
        const float dlt = sh - mu;
        q = t1 + 2.f * dlt * t0 + ((sub == 0) ? (float)HW * dlt * dlt : 0.f);
    }
    float aq = wave_sum_f(q);
    if (lane == 0) red[1][wid] = aq;
    __syncthreads();
    const float var = fmaxf((red[1][0] + red[1][1] + red[1][2] + red[1][3]) / n, 0.f);
    const float rstd = rsqrtf(var + eps);
    for (int c = gi * cpg + tid; c < (gi + 1) * cpg; c += 256) {
        const float a = rstd * gamma[c];
        *reinterpret_cast<float2 *>(coef + ((size_t)b * C + c) * 2) = make_float2(a, beta[c] - mu * a);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_gn_apply(const unsigned short *__restrict__ x, unsigned short *__restrict__ y,
                                                  unsigned HW, unsigned C, const float *__restrict__ coef, int act, unsigned total_chunks)
{
    const unsigned nch = C / 8, per_img = HW * nch;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < total_chunks; q += gridDim.x * 256u) {
        const unsigned b = q / per_img;
        const unsigned c0 = (q % nch) * 8;
        float f[8], ca[8], cd[8];
        unpack8<T>(*reinterpret_cast<const uint4 *>(x + (size_t)q * 8), f);
        load_coef8(coef + ((size_t)b * C + c0) * 2, ca, cd);
        affine8(f, ca, cd, act);
        store8<T, false>(y + (size_t)q * 8, f, 1.f);
    }
}

// Small tensors (the 16x16 / 8x8 feature maps: a few MB, L2-resident): ONE launch, one workgroup per (batch, group).
// Pass 1: sums of (x - s) and (x - s)^2 about the group's first element s; pass 2 (re-read from L2): normalise, affine, SiLU.
// The three-kernel pipeline above is launch-latency bound there (3 x ~5 us for < 2 us of traffic).
template <class T>
__global__ __launch_bounds__(256) void k_gn_small(const unsigned short *__restrict__ x, unsigned short *__restrict__ y, int HW, int C,
                                                  int G, const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                  int act)
{
    __shared__ float red[2][4];
    const int b = blockIdx.x / G, gi = blockIdx.x % G, cpg = C / G, hp = cpg / 2;     // hp: 4-byte pairs per pixel of this group
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const unsigned *xb = reinterpret_cast<const unsigned *>(x + ((size_t)b * HW * C + (size_t)gi * cpg));
    unsigned *yb = reinterpret_cast<unsigned *>(y + ((size_t)b * HW * C + (size_t)gi * cpg));
    const int n = HW * hp, rowp = C / 2;                                               // pairs in the group; pairs per pixel row
    const float sh = T::to_f((unsigned short)(xb[0] & 0xffff));
    float s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < n; i += 256) {
        const int p = i / hp, c = i - p * hp;
        const unsigned u = xb[(size_t)p * rowp + c];
        const float a = T::to_f((unsigned short)(u & 0xffff)) - sh, d = T::to_f((unsigned short)(u >> 16)) - sh;
        s1 += a + d; s2 += a * a + d * d;
    }
    s1 = wave_sum_f(s1); s2 = wave_sum_f(s2);
    if (lane == 0) { red[0][wid] = s1; red[1][wid] = s2; }
    __syncthreads();
    const float cnt = (float)HW * (float)cpg;
    const float m1 = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / cnt;           // mean of (x - s)
    const float var = fmaxf((red[1][0] + red[1][1] + red[1][2] + red[1][3]) / cnt - m1 * m1, 0.f);
    const float mu = sh + m1, rstd = rsqrtf(var + eps);
    for (int i = tid; i < n; i += 256) {
        const int p = i / hp, c = i - p * hp;
        const unsigned u = xb[(size_t)p * rowp + c];
        const int ch = gi * cpg + 2 * c;
        float v0 = (T::to_f((unsigned short)(u & 0xffff)) - mu) * rstd * gamma[ch] + beta[ch];
        float v1 = (T::to_f((unsigned short)(u >> 16)) - mu) * rstd * gamma[ch + 1] + beta[ch + 1];
        if (act) { v0 = silu(v0); v1 = silu(v1); }
        yb[(size_t)p * rowp + c] = pack2<T>(v0, v1);
    }
}

// GroupNorm from per-(batch, group) sums that the PRODUCER of x accumulated (GEMM epilogue / k_concat_add_stats):
// stats[b][g] = (sum x, sum x^2) over the HW pixels and the C/G channels of group g.  ONE launch: every workgroup (blockIdx.y =
// batch) first turns the batch's G x 2 sums into per-channel coefficients a = rstd_g * gamma_c, d = beta_c - mean_g * a in LDS, then
// streams its share of the image: y = x * a + d [SiLU], 16 bytes per lane.  Replaces k_gn_partial + k_gn_finalize + k_gn_apply.
//
// Q8: the same GroupNorm(+SiLU) with an OCP fp8 (e4m3) OUTPUT for the fp8 convolution path (k_gemm8q): y8[b][p][Cp] bytes, Cp = C rounded
// up to a multiple of 128 (one 3x3 tap per 128-byte k-tile), padding channels written as zero; stored value = y * qscale (a power of
// two: the tensor-wide E8M0 activation scale), saturated to +-448.

// the batch's [G][2] sums -> coef[c] = (a, d) for all C channels, in LDS (ends with a barrier)
__device__ __forceinline__ void gstats_to_coef(float *coef, const float *__restrict__ sb, unsigned HW, unsigned C, unsigned cpg,
                                               const float *__restrict__ gamma, const float *__restrict__ beta, float eps)
{
    const float n = (float)HW * (float)cpg;
    for (unsigned c = threadIdx.x; c < C; c += 256) {
        const unsigned g = c / cpg;
        const float mu = sb[2 * g] / n;
        const float rstd = rsqrtf(fmaxf(sb[2 * g + 1] / n - mu * mu, 0.f) + eps);
        gn_coef(mu, rstd, gamma[c], beta[c], coef[2 * c], coef[2 * c + 1]);
    }
    __syncthreads();
}

template <class T, bool Q8>
__global__ __launch_bounds__(256) void k_gn_apply_stats(const unsigned short *__restrict__ x, void *__restrict__ y, unsigned HW,
                                                        unsigned C, unsigned Cp, int G, const float *__restrict__ stats,
                                                        const float *__restrict__ gamma, const float *__restrict__ beta, float eps, int act,
                                                        float qscale)
{
    extern __shared__ float coef[];          // [C][2]
    const unsigned b = blockIdx.y, tid = threadIdx.x;
    gstats_to_coef(coef, stats + (size_t)b * G * 2, HW, C, C / G, gamma, beta, eps);
    const unsigned nch = C / 8;
    float f[8], ca[8], cd[8];
    if constexpr (Q8) {                      // 8-byte chunks of the Cp output channels, zeros beyond C
        const unsigned nchp = Cp / 8, per_img = HW * nchp;
        const unsigned short *xb = x + (size_t)b * HW * C;
        unsigned char *yb = reinterpret_cast<unsigned char *>(y) + (size_t)b * HW * Cp;
        for (unsigned q = blockIdx.x * 256u + tid; q < per_img; q += gridDim.x * 256u) {
            const unsigned p = q / nchp, ch = q - p * nchp;
            if (ch < nch) {
                const unsigned c0 = ch * 8;
                unpack8<T>(*reinterpret_cast<const uint4 *>(xb + (size_t)p * C + c0), f);
                load_coef8(coef + 2 * c0, ca, cd);
                affine8(f, ca, cd, act);
                store8<T, true>(yb + (size_t)q * 8, f, qscale);
            } else {
                *reinterpret_cast<uint2 *>(yb + (size_t)q * 8) = make_uint2(0u, 0u);
            }
        }
    } else {                                 // 16-byte chunks of the C channels
        const unsigned per_img = HW * nch;
        const unsigned short *xb = x + (size_t)b * per_img * 8;
        unsigned short *yb = reinterpret_cast<unsigned short *>(y) + (size_t)b * per_img * 8;
        for (unsigned q = blockIdx.x * 256u + tid; q < per_img; q += gridDim.x * 256u) {
            const unsigned c0 = (q % nch) * 8;
            unpack8<T>(*reinterpret_cast<const uint4 *>(xb + (size_t)q * 8), f);
            load_coef8(coef + 2 * c0, ca, cd);
            affine8(f, ca, cd, act);
            store8<T, false>(yb + (size_t)q * 8, f, 1.f);
        }
    }
}

// GroupNorm whose statistics pass was done by the PRODUCER of x (gc_gemm_desc.out_chan_parts: the conv / linear epilogue, the split-K reduce
// kernel; gc_dn_concat_add_parts): parts[b][slab][g][half] = (sum x, sum x^2) over the rows of batch b inside row slab `slab` and over the
// channels of group g inside one column tile of the producer (half 1: the rest of a group that straddles two column tiles of `col_tile`
// channels).  Plain stores on the producer side -- no atomics, no zero-init; the few KB of a batch are added up HERE, in the prologue
// of the apply kernel (<= 8 independent 8-byte loads per thread), then the moments and the per-channel coefficients, all in LDS: ONE launch.
// slab_mode 0: slabs are the producer's row tiles of R rows counted over all B * HW rows (a tile that straddles two batches has a slab
// in each); slab_mode 1: slabs restart at every batch.  Raw (unshifted) fp32 sums: relative error of the variance ~ 1e-7 * mean^2 / var.
// (Tried first: per-CHANNEL partials, summed in this prologue -- every one of the ~500 workgroups re-read nslab x C x 8 bytes and re-added
// them in LDS: 64 us instead of 23 us at 64 x 64 x 320 -- and per-channel partials with a separate finalize launch: +1.8 % views/s.)
__device__ __forceinline__ int parts_count(unsigned b, unsigned HW, unsigned R, int mode)
{
    if (mode) return (int)((HW + R - 1) / R);
    const unsigned r0 = b * HW, r1 = r0 + HW - 1;          // B * HW < 2^31 (checked on the host)
    return (int)(r1 / R - r0 / R) + 1;
}

// group moments of batch b into LDS: gs[2 g] = mean_g, gs[2 g + 1] = rstd_g (ends with a barrier).  Thread = (entry e = (group, half) of a
// slab, slab subset): all of a thread's slab loads are in flight together, the subsets meet through plain LDS stores.  (LDS float atomics
// instead: 16 ds_add_f32 per thread cost 6.7 us of a 16 us kernel -- the LDS unit serialises them lane by lane.)
__device__ __forceinline__ void gparts_to_moments(float *gs, float2 *red /* [256] */, unsigned b, unsigned HW, unsigned C, unsigned G,
                                                  const float *__restrict__ parts, int nslab, unsigned R, int mode, unsigned col_tile, float eps)
{
    const unsigned tid = threadIdx.x, cpg = C / G;
    const unsigned E = 2 * G;                                   // entries per slab (G <= 128: E <= 256)
    const unsigned nsub = 256 / E, e = tid % E, sub = tid / E;
    const int ns = parts_count(b, HW, R, mode);
    const float2 *pb = reinterpret_cast<const float2 *>(parts) + (size_t)b * nslab * E + e;
    const unsigned g = e >> 1;
    // half 1 exists only for a group that straddles two column tiles of the producer
    const bool ok = sub < nsub && (!(e & 1) || (g * cpg) / col_tile != ((g + 1) * cpg - 1) / col_tile);
    float s1 = 0.f, s2 = 0.f;
    if (ok) {
        int sl = (int)sub;
        for (; sl + 3 * (int)nsub < ns; sl += 4 * (int)nsub) {
            const float2 v0 = pb[(size_t)sl * E], v1 = pb[(size_t)(sl + nsub) * E], v2 = pb[(size_t)(sl + 2 * nsub) * E], v3 = pb[(size_t)(sl + 3 * nsub) * E];
            s1 += (v0.x + v1.x) + (v2.x + v3.x); s2 += (v0.y + v1.y) + (v2.y + v3.y);
        }
        for (; sl < ns; sl += (int)nsub) { const float2 v = pb[(size_t)sl * E]; s1 += v.x; s2 += v.y; }
    }
    if (sub < nsub) red[sub * E + e] = make_float2(s1, s2);
    __syncthreads();
    const float n = (float)HW * (float)cpg;
    if (tid < G) {
        float t1 = 0.f, t2 = 0.f;
        for (unsigned k = 0; k < nsub; ++k) {
            const float2 a = red[k * E + 2 * tid], c = red[k * E + 2 * tid + 1];
            t1 += a.x + c.x; t2 += a.y + c.y;
        }
        const float mu = t1 / n;
        gs[2 * tid] = mu; gs[2 * tid + 1] = rsqrtf(fmaxf(t2 / n - mu * mu, 0.f) + eps);
    }
    __syncthreads();
}

// Apply pass with the statistics prologue.  A thread owns ONE 16-byte channel chunk and walks the pixels of its slab (slab plan of the
// statistics kernels): its 16 coefficients live in registers -- no coefficient table in the loop (the first version read a [C][2] LDS
// table per chunk: 64-byte lane stride = 16-way bank conflicts, 43 us against 12 us for the plain apply kernel at 64 x 64 x 320 / 640) --
// and gamma / beta and the first pixels of x are requested before the partials (nothing of that depends on the statistics).
template <class T, bool Q8>
__global__ __launch_bounds__(256) void k_gn_apply_parts(const unsigned short *__restrict__ x, unsigned short *__restrict__ y, unsigned HW,
                                                        unsigned C, unsigned G, const float *__restrict__ parts, int nslab, unsigned R, int mode,
                                                        unsigned col_tile, const float *__restrict__ gamma, const float *__restrict__ beta, float eps, int act,
                                                        int nchb, int pix_per_block, unsigned Cp, float qscale)
{
    // Q8: e4m3 output y8[b][p][Cp] bytes (Cp = C rounded up to 128, padding channels written as zero by the thread of the last chunk),
    // stored = value * qscale saturated to +-448: the input of an fp8 convolution / linear (k_gn_apply_stats<T, true> with the producer's partials)
    __shared__ float gs[256];                // [G][2], G <= 128
    __shared__ float2 red[256];
    const unsigned b = blockIdx.z, cpg = C / G;
    const SlabThread st(nchb, pix_per_block, (int)HW);
    const int lanes = st.lanes, pl = st.pl, p0 = st.p0, p1 = st.p1;
    const unsigned c0 = (unsigned)st.c0;
    const bool live = st.live();
    const unsigned short *xb = x + (size_t)b * HW * C + c0;
    unsigned short *yb = y + (size_t)b * HW * C + c0;
    float4 gm[2], bt[2];
    uint4 pre[4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        gm[k] = live ? *reinterpret_cast<const float4 *>(gamma + c0 + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
        bt[k] = live ? *reinterpret_cast<const float4 *>(beta + c0 + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int p = p0 + pl + u * lanes;
        pre[u] = (live && p < p1) ? *reinterpret_cast<const uint4 *>(xb + (size_t)p * C) : make_uint4(0u, 0u, 0u, 0u);
    }
    gparts_to_moments(gs, red, b, HW, C, G, parts, nslab, R, mode, col_tile, eps);
    if (!live) return;
    float ca[8], cd[8];
    const float gmv[8] = {gm[0].x, gm[0].y, gm[0].z, gm[0].w, gm[1].x, gm[1].y, gm[1].z, gm[1].w};
    const float btv[8] = {bt[0].x, bt[0].y, bt[0].z, bt[0].w, bt[1].x, bt[1].y, bt[1].z, bt[1].w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned g = (c0 + j) / cpg;
        gn_coef(gs[2 * g], gs[2 * g + 1], gmv[j], btv[j], ca[j], cd[j]);
    }
    auto one = [&](int p, const uint4 &raw) __attribute__((always_inline)) {
        float f[8];
        unpack8<T>(raw, f);
        affine8(f, ca, cd, act);
        if constexpr (Q8) {
            unsigned char *o8 = reinterpret_cast<unsigned char *>(y) + ((size_t)b * HW + p) * Cp + c0;
            store8<T, true>(o8, f, qscale);
            if (c0 + 8 == C)
                for (unsigned c = C; c < Cp; c += 8) *reinterpret_cast<uint2 *>(o8 + (c - c0)) = make_uint2(0u, 0u);
        } else {
            store8<T, false>(yb + (size_t)p * C, f, 1.f);
        }
    };
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int p = p0 + pl + u * lanes;
        if (p < p1) one(p, pre[u]);
    }
    for (int p = p0 + pl + 4 * lanes; p < p1; p += 4 * lanes) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int pp = p + u * lanes; v[u] = *reinterpret_cast<const uint4 *>(xb + (size_t)(pp < p1 ? pp : p) * C); }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int pp = p + u * lanes; if (pp < p1) one(pp, v[u]); }
    }
}

// the coefficients alone, [B][C][2] to global (input of the fused transformer head): one workgroup per batch
__global__ __launch_bounds__(256) void k_gn_coef_parts(unsigned HW, unsigned C, unsigned G, const float *__restrict__ parts, int nslab, unsigned R, int mode,
                                                       unsigned col_tile, const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                       float *__restrict__ out)
{
    __shared__ float gs[256];
    __shared__ float2 red[256];
    const unsigned b = blockIdx.x, cpg = C / G;
    gparts_to_moments(gs, red, b, HW, C, G, parts, nslab, R, mode, col_tile, eps);
    for (unsigned c = threadIdx.x; c < C; c += 256) {
        const unsigned g = c / cpg;
        float a, d;
        gn_coef(gs[2 * g], gs[2 * g + 1], gamma[c], beta[c], a, d);
        *reinterpret_cast<float2 *>(out + ((size_t)b * C + c) * 2) = make_float2(a, d);
    }
}

// out[b][p][C1+C2] = [a | b (+ c)] with the per-(batch, group) sums of the OUTPUT accumulated on the way (the input of the next
// GroupNorm): slab structure of k_gn_partial -- a thread owns one 16-byte channel chunk and walks the pixels of its slab, partial
// sums are combined over the block's pixel lanes in LDS, one atomic pair per channel per block.
template <class T>
__global__ __launch_bounds__(256) void k_concat_add_stats(const unsigned short *__restrict__ a, int C1, const unsigned short *__restrict__ bsrc,
                                                          const unsigned short *__restrict__ c, int C2, unsigned short *__restrict__ out,
                                                          int HW, int nchb, int pix_per_block, int G, float *__restrict__ stats)
{
    extern __shared__ float sp[];   // [lanes][nchb][16], then [G][2]
    const int b = blockIdx.z, C = C1 + C2, tid = threadIdx.x;
    const SlabThread st(nchb, pix_per_block, HW);
    const int c0 = st.c0;
    const size_t row0 = (size_t)b * HW;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    if (st.live()) {
        for (int p = st.p0 + st.pl; p < st.p1; p += st.lanes) {
            const size_t m = row0 + p;
            float f[8];
            const uint4 v = concat_chunk<T>(a, C1, bsrc, c, C2, m, c0, f);
            if (out) *reinterpret_cast<uint4 *>(out + m * C + c0) = v;
#pragma unroll
            for (int j = 0; j < 8; ++j) { s1[j] += f[j]; s2[j] += f[j] * f[j]; }
        }
    }
    float acc[16];
    slab_reduce16(sp, st, s1, s2, acc);
    __syncthreads();
    float *grp = sp;                 // [G][2] group sums of this block
    for (int i = tid; i < 2 * G; i += 256) grp[i] = 0.f;
    __syncthreads();
    if (st.pl == 0) {
        const int cpg = C / G;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int gi = (c0 + j) / cpg;
            __hip_atomic_fetch_add(grp + 2 * gi, acc[2 * j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(grp + 2 * gi + 1, acc[2 * j + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * G; i += 256) {
        const float v = grp[i];
        if (v != 0.f) unsafeAtomicAdd(stats + (size_t)b * G * 2 + i, v);
    }
}

// out[b][p][C1+C2] = [a | b (+ c)] + the per-CHANNEL partial sums of the output per pixel slab, plain stores (parts[b][slab][C][2],
// slab_mode 1 of gc_dn_groupnorm_apply_parts).  A thread owns one 16-byte channel chunk and walks the pixels of its slab FOUR at a time
// (independent loads in flight; the one-at-a-time walk of k_concat_add_stats over 128-pixel slabs ran 41 us against 9 us for the plain
// concat), slabs of 16 / 32 pixels so that the grid has several workgroups per CU.
template <class T>
__global__ __launch_bounds__(256) void k_concat_add_parts(const unsigned short *__restrict__ a, int C1, const unsigned short *__restrict__ bsrc,
                                                          const unsigned short *__restrict__ c, int C2, unsigned short *__restrict__ out,
                                                          int HW, int nchb, int pix_per_block, int cpg, float *__restrict__ parts)
{
    extern __shared__ float sp[];   // [lanes][nchb][16]
    const int b = blockIdx.z, C = C1 + C2, tid = threadIdx.x;
    const SlabThread st(nchb, pix_per_block, HW);
    const int lanes = st.lanes, cch = st.cch, c0 = st.c0;
    const size_t row0 = (size_t)b * HW;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    if (st.live()) {
        const int p1 = st.p1;
        const bool first = c0 < C1;
        const unsigned short *src = first ? a + c0 : bsrc + (c0 - C1);
        const unsigned short *src2 = (!first && c) ? c + (c0 - C1) : nullptr;
        const int ld = first ? C1 : C2;
        for (int p = st.p0 + st.pl; p < p1; p += 4 * lanes) {
            uint4 v[4], w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pp = p + u * lanes;
                const size_t m = row0 + (pp < p1 ? pp : p);
                v[u] = *reinterpret_cast<const uint4 *>(src + m * ld);
                if (src2) w[u] = *reinterpret_cast<const uint4 *>(src2 + m * ld);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pp = p + u * lanes;
                if (pp >= p1) break;
                float f[8];
                v[u] = concat_combine<T>(v[u], w[u], src2 != nullptr, f);
                *reinterpret_cast<uint4 *>(out + (row0 + pp) * C + c0) = v[u];
#pragma unroll
                for (int j = 0; j < 8; ++j) { s1[j] += f[j]; s2[j] += f[j] * f[j]; }
            }
        }
    }
    float acc[16];
    slab_reduce16(sp, st, s1, s2, acc);
    if (st.pl == 0) {
        float *o = sp + (size_t)cch * 16;          // lane 0's own slot: per-channel (sum, sum^2) of this slab for the group pass
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = acc[j];
    }
    __syncthreads();
    // group g of this workgroup's channel slice = cpg consecutive channels (the slice holds whole groups: checked on the host) -> half 0
    const int gslice = nchb * 8 / cpg, G = C / cpg;
    if (tid < gslice) {
        float s1 = 0.f, s2 = 0.f;
        for (int cc = tid * cpg; cc < (tid + 1) * cpg; ++cc) { s1 += sp[2 * cc]; s2 += sp[2 * cc + 1]; }
        const int gg = blockIdx.y * gslice + tid;
        *reinterpret_cast<float2 *>(parts + (((((size_t)b * gridDim.x + blockIdx.x) * G + gg) * 2) * 2)) = make_float2(s1, s2);
    }
}

// ------------------------------------------------------------------------------------------ LayerNorm
// one wave64 per token row; exact two-pass in registers (C <= 64*8*4).
// Q8: OCP fp8 (e4m3) output, 8 bytes stored per 16-byte input chunk; stored value = y * qscale (power of two: the tensor-wide E8M0
// activation scale of the fp8 GEMM that consumes it), saturated to +-448.
template <class T, bool Q8>
__global__ __launch_bounds__(256) void k_layernorm(const unsigned short *__restrict__ x, void *__restrict__ y,
                                                   int64_t M, int C, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, float eps, float qscale)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nch = C / 8;
    float f[4][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            unpack8<T>(*reinterpret_cast<const uint4 *>(x + row * C + ch * 8), f[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += f[i][j];
        }
    }
    const float mean = wave_sum_f(s) / (float)C;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < nch) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = f[i][j] - mean; v += d * d; }
        }
    const float rstd = rsqrtf(wave_sum_f(v) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (f[i][j] - mean) * rstd * gamma[ch * 8 + j] + beta[ch * 8 + j];
            store8<T, Q8>(reinterpret_cast<unsigned char *>(y) + (row * C + ch * 8) * (Q8 ? 1 : 2), o, qscale);
        }
    }
}

// ------------------------------------------------------------------------------------------ elementwise
// out[M, C1+C2] = [a[M,C1] | b[M,C2] (+ c[M,C2])]   (skip concat of the up blocks, with the ControlNet
// residual add of `down_block_res_samples` folded in)
template <class T>
__global__ __launch_bounds__(256) void k_concat_add(const unsigned short *__restrict__ a, int C1,
                                                    const unsigned short *__restrict__ b, const unsigned short *__restrict__ c,
                                                    int C2, unsigned short *__restrict__ out, unsigned total_chunks)
{
    const unsigned nch = (C1 + C2) / 8;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < total_chunks; q += gridDim.x * 256u) {
        const size_t m = q / nch;
        const unsigned ch = q - (unsigned)m * nch;
        float f[8];
        *reinterpret_cast<uint4 *>(out + m * (int64_t)(C1 + C2) + ch * 8) = concat_chunk<T>(a, C1, b, c, C2, m, (int)(ch * 8), f);
    }
}

// out = a*sa + b*sb (b may be null); act: 0 none, 1 silu
template <class T>
__global__ __launch_bounds__(256) void k_axpby(const unsigned short *__restrict__ a, float sa, const unsigned short *__restrict__ b,
                                               float sb, int act, unsigned short *__restrict__ out, int64_t total_chunks)
{
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total_chunks; q += (int64_t)gridDim.x * 256) {
        float fa[8], fb[8];
        unpack8<T>(*reinterpret_cast<const uint4 *>(a + q * 8), fa);
        if (b) unpack8<T>(*reinterpret_cast<const uint4 *>(b + q * 8), fb);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = fa[j] * sa + (b ? fb[j] * sb : 0.f);
            fa[j] = act ? silu(v) : v;
        }
        *reinterpret_cast<uint4 *>(out + q * 8) = pack8<T>(fa);
    }
}

// fp32 -> T with optional silu (time-embedding vectors)
template <class T>
__global__ __launch_bounds__(256) void k_cast_f32(const float *__restrict__ a, int act, unsigned short *__restrict__ out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v = a[i];
        out[i] = T::from_f(act ? silu(v) : v);
    }
}

// row softmax in place over [M, N] T (VAE mid-block attention scores), one workgroup per row
template <class T>
__global__ __launch_bounds__(256) void k_softmax_rows(unsigned short *__restrict__ s, int64_t N, int64_t ld, float scale)
{
    __shared__ float red[4];
    unsigned short *row = s + (int64_t)blockIdx.x * ld;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float mx = -1e30f;
    for (int64_t i = tid; i < N; i += 256) mx = fmaxf(mx, T::to_f(row[i]) * scale);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    if (lane == 0) red[wid] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int64_t i = tid; i < N; i += 256) sum += __expf(T::to_f(row[i]) * scale - mx);
    sum = wave_sum_f(sum);
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    const float inv = 1.f / (red[0] + red[1] + red[2] + red[3]);
    for (int64_t i = tid; i < N; i += 256) row[i] = T::from_f(__expf(T::to_f(row[i]) * scale - mx) * inv);
}

// CFG combine + DDIM step fused with the re-packing of the next UNet input:
//   eps = eps_u + gs*(eps_c - eps_u); x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t); x' = sqrt(a_p) x0 + sqrt(1-a_p) eps
// eps: fp32 [2f or f][HW][ldE] (conv_out, channels padded to ldE); lat: fp32 master [f][HW][4];
// xin: T [nrep*f][HW][8] (channels 4..7 stay zero) -- the `cat([latents]*2)` of the pipeline.
template <class T>
__global__ __launch_bounds__(256) void k_cfg_ddim(const float *__restrict__ eps, int ldE, int64_t f, int64_t HW, float gs,
                                                  int cfg, float c_x, float c_e, float *__restrict__ lat,
                                                  unsigned short *__restrict__ xin, int nrep)
{
    const int64_t n = f * HW;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float4 eu = *reinterpret_cast<const float4 *>(eps + i * ldE);
        float4 e = eu;
        if (cfg) {
            const float4 ec = *reinterpret_cast<const float4 *>(eps + (n + i) * ldE);
            e = make_float4(eu.x + gs * (ec.x - eu.x), eu.y + gs * (ec.y - eu.y), eu.z + gs * (ec.z - eu.z), eu.w + gs * (ec.w - eu.w));
        }
        float4 x = *reinterpret_cast<float4 *>(lat + i * 4);
        // x' = c_x * x + c_e * eps  with c_x = sqrt(a_p/a_t), c_e = sqrt(1-a_p) - sqrt(a_p (1-a_t)/a_t)
        x = make_float4(c_x * x.x + c_e * e.x, c_x * x.y + c_e * e.y, c_x * x.z + c_e * e.z, c_x * x.w + c_e * e.w);
        *reinterpret_cast<float4 *>(lat + i * 4) = x;
        const uint4 p = make_uint4(pack2<T>(x.x, x.y), pack2<T>(x.z, x.w), 0u, 0u);
        for (int r = 0; r < nrep; ++r) *reinterpret_cast<uint4 *>(xin + (r * n + i) * 8) = p;
    }
}

__global__ __launch_bounds__(256) void k_disp_max(const float *__restrict__ depth, int64_t n, unsigned *__restrict__ mx)
{
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, 1.f / (depth[i] + 1e-5f));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(mx, __float_as_uint(m));     // disparity > 0: uint order == float order
}

template <class T>
__global__ __launch_bounds__(256) void k_disp_write(const float *__restrict__ depth, int64_t n, const unsigned *__restrict__ mx,
                                                    unsigned short *__restrict__ out)
{
    const float inv = 1.f / __uint_as_float(*mx);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float d = (1.f / (depth[i] + 1e-5f)) * inv;
        const unsigned h = T::from_f(d);
        *reinterpret_cast<uint4 *>(out + i * 8) = make_uint4(h | (h << 16), h, 0u, 0u);
    }
}

__global__ __launch_bounds__(256) void k_mask_composite(const float *__restrict__ e, int ld_e, const float *__restrict__ u,
                                                        const float *__restrict__ m, float *__restrict__ out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float w = m ? m[i] : 1.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * i + c] = e[i * ld_e + c] * w + (m ? u[3 * i + c] * (1.f - w) : 0.f);
    }
}

// ------------------------------------------------------------------------------------------ host side
// The launches of entry point `fn`: f(T{}) with T = BF16 / F16 for the dtype code of the C ABI (every launch is written once, in a generic
// lambda), then the launch check
template <class F>
inline int dn_for_type(const char *fn, int dtype, F &&f)
{
    if (dtype == DT_BF16) f(BF16{});
    else if (dtype == DT_F16) f(F16{});
    else { gc::set_error("%s: bad dtype", fn); return GC_EINVAL; }
    return gc::check_launch(fn);
}

inline const unsigned short *in16(const void *p) { return static_cast<const unsigned short *>(p); }
inline unsigned short *out16(void *p) { return static_cast<unsigned short *>(p); }

// channel slices of the slab kernels: the fewest equal slices of <= 256 16-byte chunks
inline void chan_slices(int C, int *ny, int *nchb)
{
    const int nch = C / 8;
    int y = 1;
    while (nch % y != 0 || nch / y > 256) ++y;
    *ny = y; *nchb = nch / y;
}

struct SlabPlan { int nslab, ppb, ny, nchb; };      // pixel slabs of ppb pixels x ny channel slices of nchb chunks

inline SlabPlan slab_plan(int64_t HW, int C, int ppb_wanted)
{
    SlabPlan p;
    chan_slices(C, &p.ny, &p.nchb);
    p.ppb = std::max(ppb_wanted, 256 / p.nchb);      // a slab has at least `lanes` pixels
    p.nslab = (int)((HW + p.ppb - 1) / p.ppb);
    return p;
}
// slab plan of the GroupNorm statistics pass: pixel slabs sized for ~1-2k workgroups, at most 32 slabs per image (keeps the finalize pass tiny)
inline SlabPlan gn_plan(int64_t HW, int C) { return slab_plan(HW, C, (int)((HW + 31) / 32)); }
// slab plan of gc_dn_concat_add_parts and of the apply pass that reads its partials: slabs of 16 / 32 pixels
inline SlabPlan concat_parts_plan(int64_t HW, int C) { return slab_plan(HW, C, HW >= 4096 ? 32 : 16); }

// grid and dynamic LDS bytes (the [lanes][nchb][16] staging of slab_reduce16) of a slab launch
struct SlabGrid { dim3 grid; size_t lds; };
inline SlabGrid slab_grid(int nslab, int ny, int64_t B, int nchb)
{
    return {dim3((unsigned)nslab, (unsigned)ny, (unsigned)B), sizeof(float) * 16 * (size_t)(256 / nchb) * nchb};
}

// stored = value * 2^(127 - byte); the MFMA multiplies by 2^(byte - 127)
inline float qscale_of(int a_scale) { return exp2f((float)(127 - a_scale)); }

// workgroups per image of k_gn_apply_stats: enough to fill the chip, few enough that the coefficient prologue (a few KB from L2 per
// workgroup) stays small
inline dim3 apply_stats_grid(int64_t per_img, int64_t B)
{
    const int64_t cap = std::max<int64_t>(1, (256 * 4 + B - 1) / B);
    return dim3((unsigned)std::min((per_img + 255) / 256, cap), (unsigned)B);
}

inline unsigned ew_grid(int64_t items) { return (unsigned)std::min<int64_t>((items + 255) / 256, 256 * 8); }

// k_gn_partial + k_gn_finalize: x -> per-channel partial sums `part` -> coefficients coef[B][C][2]
template <class T>
void launch_gn_partial_finalize(const void *x, int64_t B, int64_t HW, int C, int G, const float *gamma, const float *beta, float eps, const SlabPlan &p,
                                float *part, float *coef, hipStream_t s)
{
    const SlabGrid sg = slab_grid(p.nslab, p.ny, B, p.nchb);
    hipLaunchKernelGGL((k_gn_partial<T>), sg.grid, dim3(256), sg.lds, s, in16(x), (int)HW, C, p.nchb, p.ppb, part);
    hipLaunchKernelGGL((k_gn_finalize<T>), dim3((unsigned)(B * G)), dim3(256), 0, s, in16(x), (int)HW, C, G, p.nslab, part, gamma, beta, eps, coef);
}

}  // namespace

extern "C" {

size_t gc_dn_groupnorm_workspace_bytes(int64_t B, int64_t HW, int C)
{
    return sizeof(float) * 2 * (size_t)B * (size_t)C * (size_t)(gn_plan(HW, C).nslab + 1);
}

int gc_dn_groupnorm(int dtype, const void *x, void *y, int64_t B, int64_t HW, int C, int G, const float *gamma,
                    const float *beta, float eps, int act, float *stats_ws, void *stream)
{
    GC_REQUIRE(C % 8 == 0 && C % G == 0 && stats_ws, "groupnorm: C must be a multiple of 8 and of G; workspace required");
    GC_REQUIRE(C / G <= 256 && B * HW * (C / 8) < (int64_t)1 << 31, "groupnorm: group too wide / tensor too large");
    hipStream_t s = gc::S(stream);
    // act bit 8: batch-invariant planning -- the one-launch form (other summation order) is chosen from the per-frame size only
    const int64_t Bsel = (act & 0x100) ? 1 : B;
    act &= 0xff;
    if ((C / G) % 2 == 0 && Bsel * HW * (int64_t)C <= ((int64_t)1 << 20) && Bsel * G >= 64) {      // <= 2 MB (the 8x8 maps): one launch, 5 vs 12 us
        return dn_for_type(__func__, dtype, [&](auto t) {
            hipLaunchKernelGGL((k_gn_small<decltype(t)>), dim3((unsigned)(B * G)), dim3(256), 0, s, in16(x), out16(y), (int)HW, C, G, gamma, beta, eps, act);
        });
    }
    const SlabPlan p = gn_plan(HW, C);
    float *part = stats_ws, *coef = stats_ws + 2 * (size_t)B * C * p.nslab;
    const int64_t chunks = B * HW * (C / 8);
    return dn_for_type(__func__, dtype, [&](auto t) {
        launch_gn_partial_finalize<decltype(t)>(x, B, HW, C, G, gamma, beta, eps, p, part, coef, s);
        hipLaunchKernelGGL((k_gn_apply<decltype(t)>), dim3(ew_grid(chunks)), dim3(256), 0, s, in16(x), out16(y), (unsigned)HW, (unsigned)C, coef, act,
                           (unsigned)chunks);
    });
}

int gc_dn_groupnorm_coef(int dtype, const void *x, int64_t B, int64_t HW, int C, int G, const float *gamma, const float *beta, float eps,
                         float *stats_ws, float *coef, void *stream)
{
    GC_REQUIRE(C % 8 == 0 && C % G == 0 && stats_ws && coef, "groupnorm_coef: C must be a multiple of 8 and of G; workspace and output required");
    GC_REQUIRE(C / G <= 256 && B * HW * (C / 8) < (int64_t)1 << 31, "groupnorm_coef: group too wide / tensor too large");
    return dn_for_type(__func__, dtype, [&](auto t) {
        launch_gn_partial_finalize<decltype(t)>(x, B, HW, C, G, gamma, beta, eps, gn_plan(HW, C), stats_ws, coef, gc::S(stream));
    });
}

int gc_dn_groupnorm_apply(int dtype, const void *x, void *y, int64_t B, int64_t HW, int C, int G, const float *gamma,
                          const float *beta, float eps, int act, const float *group_stats, void *stream)
{
    GC_REQUIRE(C % 8 == 0 && C % G == 0 && group_stats && gamma && beta, "groupnorm_apply: C must be a multiple of 8 and of G; statistics required");
    GC_REQUIRE(HW * (int64_t)(C / 8) < (int64_t)1 << 31 && B <= 65535, "groupnorm_apply: tensor too large");
    const size_t lds = sizeof(float) * 2 * (size_t)C;
    const dim3 grid = apply_stats_grid(HW * (C / 8), B);
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_gn_apply_stats<decltype(t), false>), grid, dim3(256), lds, gc::S(stream), in16(x), y, (unsigned)HW, (unsigned)C, 0u, G,
                           group_stats, gamma, beta, eps, act, 1.f);
    });
}

int gc_dn_groupnorm_apply_fp8(int dtype, const void *x, void *y8, int64_t B, int64_t HW, int C, int C_padded, int G, const float *gamma,
                              const float *beta, float eps, int act, const float *group_stats, int a_scale, void *stream)
{
    GC_REQUIRE(C % 8 == 0 && C % G == 0 && group_stats && gamma && beta, "groupnorm_apply_fp8: C must be a multiple of 8 and of G; statistics required");
    GC_REQUIRE(C_padded >= C && C_padded % 128 == 0, "groupnorm_apply_fp8: padded channel count must be a multiple of 128");
    GC_REQUIRE(HW * (int64_t)(C_padded / 8) < (int64_t)1 << 31 && B <= 65535 && a_scale > 0 && a_scale < 255, "groupnorm_apply_fp8: bad size / scale");
    const size_t lds = sizeof(float) * 2 * (size_t)C;
    const dim3 grid = apply_stats_grid(HW * (C_padded / 8), B);
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_gn_apply_stats<decltype(t), true>), grid, dim3(256), lds, gc::S(stream), in16(x), y8, (unsigned)HW, (unsigned)C,
                           (unsigned)C_padded, G, group_stats, gamma, beta, eps, act, qscale_of(a_scale));
    });
}

int gc_dn_layernorm(int dtype, const void *x, void *y, int64_t M, int C, const float *gamma, const float *beta,
                    float eps, void *stream)
{
    GC_REQUIRE(C % 8 == 0 && C <= 2048, "layernorm: C must be a multiple of 8 and <= 2048");
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_layernorm<decltype(t), false>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, gc::S(stream), in16(x), y, M, C, gamma, beta, eps, 1.f);
    });
}

int gc_dn_layernorm_fp8(int dtype, const void *x, void *y8, int64_t M, int C, const float *gamma, const float *beta,
                        float eps, int a_scale, void *stream)
{
    GC_REQUIRE(C % 16 == 0 && C <= 2048, "layernorm_fp8: C must be a multiple of 16 and <= 2048");
    GC_REQUIRE(a_scale > 0 && a_scale < 255 && M > 0 && x && y8 && gamma && beta, "layernorm_fp8: bad scale / null argument");
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_layernorm<decltype(t), true>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, gc::S(stream), in16(x), y8, M, C, gamma, beta, eps,
                           qscale_of(a_scale));
    });
}

int gc_dn_concat_add(int dtype, const void *a, int C1, const void *b, const void *c, int C2, void *out, int64_t M, int64_t rows_per_batch,
                     float *group_stats, int gn_groups, void *stream)
{
    GC_REQUIRE(C1 % 8 == 0 && C2 % 8 == 0, "concat: channel counts must be multiples of 8");
    if (group_stats) {      // copy + per-(batch, group) sums of the output, added into the caller-zeroed group_stats[B][gn_groups][2]
        GC_REQUIRE(rows_per_batch > 0 && M % rows_per_batch == 0 && M / rows_per_batch <= 65535, "concat: M must be B * rows_per_batch");
        GC_REQUIRE(gn_groups >= 1 && gn_groups <= 64 && (C1 + C2) % gn_groups == 0, "concat: gn_groups must divide C1 + C2");
        const SlabPlan p = gn_plan(rows_per_batch, C1 + C2);
        const SlabGrid sg = slab_grid(p.nslab, p.ny, M / rows_per_batch, p.nchb);
        return dn_for_type(__func__, dtype, [&](auto t) {
            hipLaunchKernelGGL((k_concat_add_stats<decltype(t)>), sg.grid, dim3(256), sg.lds, gc::S(stream), in16(a), C1, in16(b), in16(c), C2, out16(out),
                               (int)rows_per_batch, p.nchb, p.ppb, gn_groups, group_stats);
        });
    }
    const int64_t chunks = M * ((C1 + C2) / 8);
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_concat_add<decltype(t)>), dim3(ew_grid(chunks)), dim3(256), 0, gc::S(stream), in16(a), C1, in16(b), in16(c), C2, out16(out),
                           (unsigned)chunks);
    });
}

int gc_dn_groupnorm_coef_parts(int64_t B, int64_t HW, int C, int G, const float *gamma, const float *beta, float eps, const float *parts,
                               int64_t rows_per_slab, int nslab, int slab_mode, int col_tile, float *coef, void *stream)
{
    GC_REQUIRE(C % G == 0 && G <= 128 && parts && gamma && beta && coef && rows_per_slab > 0 && nslab > 0 && col_tile > 0 && B * HW < (int64_t)1 << 31,
               "groupnorm_coef_parts: bad arguments");
    hipLaunchKernelGGL(k_gn_coef_parts, dim3((unsigned)B), dim3(256), 0, gc::S(stream), (unsigned)HW, (unsigned)C, (unsigned)G, parts, nslab,
                       (unsigned)rows_per_slab, slab_mode, (unsigned)col_tile, gamma, beta, eps, coef);
    return gc::check_launch("gc_dn_groupnorm_coef_parts");
}

int gc_dn_groupnorm_apply_parts(int dtype, const void *x, void *y, int64_t B, int64_t HW, int C, int G, const float *gamma, const float *beta,
                                float eps, int act, const float *parts, int64_t rows_per_slab, int nslab, int slab_mode, int col_tile, void *stream)
{
    GC_REQUIRE(C % 8 == 0 && C % G == 0 && G <= 128 && parts && gamma && beta, "groupnorm_apply_parts: C must be a multiple of 8 and of G; partials required");
    GC_REQUIRE(HW * (int64_t)C < (int64_t)1 << 31 && B * HW < (int64_t)1 << 31 && B <= 65535 && rows_per_slab > 0 && nslab > 0 && col_tile > 0,
               "groupnorm_apply_parts: bad sizes");
    const SlabPlan p = concat_parts_plan(HW, C);      // the walk of gc_dn_concat_add_parts; `nslab` / `rows_per_slab` describe the PRODUCER's partials
    const dim3 grid = slab_grid(p.nslab, p.ny, B, p.nchb).grid;
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_gn_apply_parts<decltype(t), false>), grid, dim3(256), 0, gc::S(stream), in16(x), out16(y), (unsigned)HW, (unsigned)C, (unsigned)G,
                           parts, nslab, (unsigned)rows_per_slab, slab_mode, (unsigned)col_tile, gamma, beta, eps, act, p.nchb, p.ppb, 0u, 1.f);
    });
}

int gc_dn_groupnorm_apply_parts_fp8(int dtype, const void *x, void *y8, int64_t B, int64_t HW, int C, int C_padded, int G, const float *gamma,
                                    const float *beta, float eps, int act, const float *parts, int64_t rows_per_slab, int nslab, int slab_mode,
                                    int col_tile, int a_scale, void *stream)
{
    GC_REQUIRE(C % 8 == 0 && C % G == 0 && G <= 128 && parts && gamma && beta, "groupnorm_apply_parts_fp8: C must be a multiple of 8 and of G; partials required");
    GC_REQUIRE(C_padded >= C && C_padded % 128 == 0 && a_scale > 0 && a_scale < 255, "groupnorm_apply_parts_fp8: padded channel count % 128 == 0; E8M0 scale byte");
    GC_REQUIRE(HW * (int64_t)C_padded < (int64_t)1 << 31 && B * HW < (int64_t)1 << 31 && B <= 65535 && rows_per_slab > 0 && nslab > 0 && col_tile > 0,
               "groupnorm_apply_parts_fp8: bad sizes");
    const SlabPlan p = concat_parts_plan(HW, C);
    const dim3 grid = slab_grid(p.nslab, p.ny, B, p.nchb).grid;
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_gn_apply_parts<decltype(t), true>), grid, dim3(256), 0, gc::S(stream), in16(x), out16(y8), (unsigned)HW, (unsigned)C, (unsigned)G,
                           parts, nslab, (unsigned)rows_per_slab, slab_mode, (unsigned)col_tile, gamma, beta, eps, act, p.nchb, p.ppb, (unsigned)C_padded,
                           qscale_of(a_scale));
    });
}

int gc_dn_concat_parts_layout(int64_t rows_per_batch, int C, int gn_groups, int64_t *rows_per_slab, int *nslab, int *col_tile)
{
    GC_REQUIRE(rows_per_slab && nslab && col_tile && rows_per_batch > 0 && C % 8 == 0 && gn_groups >= 1, "concat_parts_layout: bad arguments");
    *rows_per_slab = 0; *nslab = 0; *col_tile = 0;
    const SlabPlan p = concat_parts_plan(rows_per_batch, C);
    if (C % gn_groups != 0 || (p.nchb * 8) % (C / gn_groups) != 0 || p.nchb * 8 / (C / gn_groups) > 256) return GC_OK;     // a channel slice must hold whole groups
    *rows_per_slab = p.ppb; *nslab = p.nslab; *col_tile = p.nchb * 8;
    return GC_OK;
}

int gc_dn_concat_add_parts(int dtype, const void *a, int C1, const void *b, const void *c, int C2, void *out, int64_t M, int64_t rows_per_batch,
                           int gn_groups, float *parts, void *stream)
{
    GC_REQUIRE(gn_groups >= 1 && (C1 + C2) % gn_groups == 0, "concat_parts: gn_groups must divide C1 + C2");
    const int cpg = (C1 + C2) / gn_groups;
    GC_REQUIRE(C1 % 8 == 0 && C2 % 8 == 0 && parts && out, "concat_parts: channel counts must be multiples of 8; output and partials buffer required");
    GC_REQUIRE(rows_per_batch > 0 && M % rows_per_batch == 0 && M / rows_per_batch <= 65535, "concat_parts: M must be B * rows_per_batch");
    const SlabPlan p = concat_parts_plan(rows_per_batch, C1 + C2);
    GC_REQUIRE((p.nchb * 8) % cpg == 0 && p.nchb * 8 / cpg <= 256, "concat_parts: a channel slice must hold whole groups (see gc_dn_concat_parts_layout)");
    const SlabGrid sg = slab_grid(p.nslab, p.ny, M / rows_per_batch, p.nchb);
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_concat_add_parts<decltype(t)>), sg.grid, dim3(256), sg.lds, gc::S(stream), in16(a), C1, in16(b), in16(c), C2, out16(out),
                           (int)rows_per_batch, p.nchb, p.ppb, cpg, parts);
    });
}

int gc_dn_group_stats(int dtype, const void *x, int64_t B, int64_t HW, int C, int G, float *group_stats, void *stream)
{
    GC_REQUIRE(C % 8 == 0 && G >= 1 && G <= 64 && C % G == 0 && group_stats && B <= 65535, "group_stats: C % 8 == 0, G | C, statistics buffer required");
    const SlabPlan p = gn_plan(HW, C);
    const SlabGrid sg = slab_grid(p.nslab, p.ny, B, p.nchb);
    const unsigned short *none = nullptr;
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_concat_add_stats<decltype(t)>), sg.grid, dim3(256), sg.lds, gc::S(stream), in16(x), C, none, none, 0, (unsigned short *)nullptr,
                           (int)HW, p.nchb, p.ppb, G, group_stats);
    });
}

int gc_dn_axpby(int dtype, const void *a, float sa, const void *b, float sb, int act, void *out, int64_t n, void *stream)
{
    GC_REQUIRE(n % 8 == 0, "axpby: element count must be a multiple of 8");
    const int64_t chunks = n / 8;
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_axpby<decltype(t)>), dim3(ew_grid(chunks)), dim3(256), 0, gc::S(stream), in16(a), sa, in16(b), sb, act, out16(out), chunks);
    });
}

int gc_dn_cast_f32(int dtype, const float *a, int act, void *out, int64_t n, void *stream)
{
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_cast_f32<decltype(t)>), dim3(ew_grid(n)), dim3(256), 0, gc::S(stream), a, act, out16(out), n);
    });
}

int gc_dn_softmax_rows(int dtype, void *s, int64_t M, int64_t N, int64_t ld, float scale, void *stream)
{
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_softmax_rows<decltype(t)>), dim3((unsigned)M), dim3(256), 0, gc::S(stream), out16(s), N, ld, scale);
    });
}

int gc_dn_depth_to_disparity(int dtype, const float *depth, int64_t HW, void *out, unsigned *max_ws, void *stream)
{
    hipStream_t s = gc::S(stream);
    if (hipMemsetAsync(max_ws, 0, 4, s) != hipSuccess) return GC_ELAUNCH;
    // 64 workgroups: the maximum ends in ONE word, and 4096 waves doing an atomicMax on it cost 48 us (~12 ns each), 256 cost ~3 us
    hipLaunchKernelGGL(k_disp_max, dim3(std::min<unsigned>(ew_grid(HW), 64u)), dim3(256), 0, s, depth, HW, max_ws);
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_disp_write<decltype(t)>), dim3(ew_grid(HW)), dim3(256), 0, s, depth, HW, max_ws, out16(out));
    });
}

int gc_dn_mask_composite(const float *edited, int ld_e, const float *unedited, const float *mask, float *out, int64_t HW,
                         void *stream)
{
    GC_REQUIRE(edited && out && (mask == nullptr || unedited != nullptr), "mask_composite: bad arguments");
    hipLaunchKernelGGL(k_mask_composite, dim3(ew_grid(HW)), dim3(256), 0, gc::S(stream), edited, ld_e, unedited, mask, out, HW);
    return gc::check_launch("gc_dn_mask_composite");
}

int gc_dn_cfg_ddim_step(int dtype, const float *eps, int ld_eps, int64_t frames, int64_t HW, float guidance, int cfg,
                        float alpha_t, float alpha_prev, float *latents, void *xin, int nrep, void *stream)
{
    GC_REQUIRE(ld_eps >= 4 && ld_eps % 4 == 0 && alpha_t > 0.f, "cfg_ddim: bad arguments");
    const float c_x = sqrtf(alpha_prev / alpha_t);
    const float c_e = sqrtf(1.f - alpha_prev) - sqrtf(alpha_prev * (1.f - alpha_t) / alpha_t);
    const int64_t n = frames * HW;
    return dn_for_type(__func__, dtype, [&](auto t) {
        hipLaunchKernelGGL((k_cfg_ddim<decltype(t)>), dim3(ew_grid(n)), dim3(256), 0, gc::S(stream), eps, ld_eps, frames, HW, guidance, cfg, c_x, c_e, latents,
                           out16(xin), nrep);
    });
}

}  // extern "C"

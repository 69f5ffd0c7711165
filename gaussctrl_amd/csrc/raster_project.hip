// raster_project.hip -- per-Gaussian front end of the splat rasterizer for gfx950.
//
// Replaces gsplat 0.1.3's project_gaussians / spherical_harmonics (+ their backward) as called from
// /root/reference/gaussctrl/gc_model.py:140-154,166 and adds the fused "one pass over the 59-float
// parameter record" kernels used by the product path (gc_model.py:138-169,181 in one launch).
//
// HBM-bound, 1 lane per Gaussian, wave64, no LDS needed: the record is read once with 16-byte loads
// where alignment allows.  This translation unit is compiled with -ffp-contract=off: the projection
// arithmetic is written as explicit IEEE binary32 operations in a fixed order so that the integer
// outputs (radii, tile boxes, num_tiles_hit -> sort keys) are bit-identical to the CPU oracle.
#include "common.h"
#include "../../include/gaussctrl_antialias.h"
#include "../../include/gaussctrl_pose.h"
#include <type_traits>

namespace {

constexpr int TILE = 16;

struct Cam {
    float V[12];   // row-major 3x4 world->camera
    float P[16];   // row-major 4x4 full projection
    float fx, fy, cx, cy;
    int H, W, tiles_x, tiles_y;
    float clip, glob;
    float ox, oy, oz;   // camera origin (world) for view directions
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(hi, fmaxf(lo, v)); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct Rot {
    float R[9];
    float qn[4];
    float inv_norm;
};

__device__ __forceinline__ void quat_to_rotmat(float w, float x, float y, float z, Rot &o)
{
    float n2 = ((w * w + x * x) + y * y) + z * z;
    float s = 1.f / sqrtf(n2);
    w = w * s; x = x * s; y = y * s; z = z * s;
    o.qn[0] = w; o.qn[1] = x; o.qn[2] = y; o.qn[3] = z; o.inv_norm = s;
    o.R[0] = 1.f - 2.f * (y * y + z * z);
    o.R[1] = 2.f * (x * y - w * z);
    o.R[2] = 2.f * (x * z + w * y);
    o.R[3] = 2.f * (x * y + w * z);
    o.R[4] = 1.f - 2.f * (x * x + z * z);
    o.R[5] = 2.f * (y * z - w * x);
    o.R[6] = 2.f * (x * z - w * y);
    o.R[7] = 2.f * (y * z + w * x);
    o.R[8] = 1.f - 2.f * (x * x + y * y);
}

__device__ __forceinline__ void scale_rot_to_cov3d(float s0, float s1, float s2, float glob, const float *R,
                                                   float *c, float *m)
{
    float sx = glob * s0, sy = glob * s1, sz = glob * s2;
    m[0] = R[0] * sx; m[1] = R[1] * sy; m[2] = R[2] * sz;
    m[3] = R[3] * sx; m[4] = R[4] * sy; m[5] = R[5] * sz;
    m[6] = R[6] * sx; m[7] = R[7] * sy; m[8] = R[8] * sz;
    c[0] = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    c[1] = (m[0] * m[3] + m[1] * m[4]) + m[2] * m[5];
    c[2] = (m[0] * m[6] + m[1] * m[7]) + m[2] * m[8];
    c[3] = (m[3] * m[3] + m[4] * m[4]) + m[5] * m[5];
    c[4] = (m[3] * m[6] + m[4] * m[7]) + m[5] * m[8];
    c[5] = (m[6] * m[6] + m[7] * m[7]) + m[8] * m[8];
}

struct Proj {
    float cov3d[6];
    float xy[2];
    float depth;
    float conic[3];
    int radius;
    int tiles_hit;
    float comp;        // AA only: opacity compensation rho (0 when culled)
};

// SURVEY.md Appendix A.1; op order mirrors oracle/raster_ref.c::project_one exactly.
// AA (rasterize_mode "antialiased" of later splatfacto / gsplat versions, the Mip-Splatting opacity compensation): also
// o.comp = rho = sqrt(max(0, det(cov2d) / det(cov2d + 0.3 I))), formed from the un-blurred a0, d0 themselves ((a - 0.3)(d - 0.3) would cancel
// for the sub-pixel splats the mode exists for); 0 for a culled Gaussian.  Every other output is the classic one bit for bit: a0 + 0.3f is
// the same IEEE operation whether a0 has a name or not (-ffp-contract=off).
template <bool AA = false>
__device__ __forceinline__ bool project_one(const Cam &cam, float p0, float p1, float p2, float s0, float s1,
                                            float s2, float qw, float qx, float qy, float qz, Proj &o)
{
    const float *V = cam.V, *P = cam.P;
    o.radius = 0; o.tiles_hit = 0; o.depth = 0.f; o.xy[0] = o.xy[1] = 0.f;
    o.conic[0] = o.conic[1] = o.conic[2] = 0.f;
    if (AA) o.comp = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) o.cov3d[k] = 0.f;
    float tx = ((V[0] * p0 + V[1] * p1) + V[2] * p2) + V[3];
    float ty = ((V[4] * p0 + V[5] * p1) + V[6] * p2) + V[7];
    float tz = ((V[8] * p0 + V[9] * p1) + V[10] * p2) + V[11];
    if (tz <= cam.clip) return false;
    Rot rot; float m[9];
    quat_to_rotmat(qw, qx, qy, qz, rot);
    scale_rot_to_cov3d(s0, s1, s2, cam.glob, rot.R, o.cov3d, m);
    float lim_x = 1.3f * (0.5f * (float)cam.W / cam.fx);
    float lim_y = 1.3f * (0.5f * (float)cam.H / cam.fy);
    float txc = tz * clampf(tx / tz, -lim_x, lim_x);
    float tyc = tz * clampf(ty / tz, -lim_y, lim_y);
    float rz = 1.f / tz;
    float rz2 = rz * rz;
    float j00 = cam.fx * rz, j02 = -(cam.fx * txc) * rz2;
    float j11 = cam.fy * rz, j12 = -(cam.fy * tyc) * rz2;
    float t00 = j00 * V[0] + j02 * V[8], t01 = j00 * V[1] + j02 * V[9], t02 = j00 * V[2] + j02 * V[10];
    float t10 = j11 * V[4] + j12 * V[8], t11 = j11 * V[5] + j12 * V[9], t12 = j11 * V[6] + j12 * V[10];
    const float *c = o.cov3d;
    float u00 = (t00 * c[0] + t01 * c[1]) + t02 * c[2];
    float u01 = (t00 * c[1] + t01 * c[3]) + t02 * c[4];
    float u02 = (t00 * c[2] + t01 * c[4]) + t02 * c[5];
    float u10 = (t10 * c[0] + t11 * c[1]) + t12 * c[2];
    float u11 = (t10 * c[1] + t11 * c[3]) + t12 * c[4];
    float u12 = (t10 * c[2] + t11 * c[4]) + t12 * c[5];
    float a0 = (u00 * t00 + u01 * t01) + u02 * t02, a = a0 + 0.3f;
    float b = (u00 * t10 + u01 * t11) + u02 * t12;
    float d0 = (u10 * t10 + u11 * t11) + u12 * t12, d = d0 + 0.3f;
    float det = a * d - b * b;
    if (det == 0.f) return false;
    float rho = 0.f;
    if (AA) rho = sqrtf(fmaxf(0.f, (a0 * d0 - b * b) / det));      // (fmaxf drops a NaN: inf / inf of an overflowing covariance gives 0)
    float inv_det = 1.f / det;
    // written before the tile-box cull, like gsplat / the oracle (unobservable for culled splats)
    o.conic[0] = d * inv_det; o.conic[1] = -b * inv_det; o.conic[2] = a * inv_det;
    float mid = 0.5f * (a + d);
    float disc = sqrtf(fmaxf(0.1f, mid * mid - det));
    float v1 = mid + disc, v2 = mid - disc;
    float radius = ceilf(3.f * sqrtf(fmaxf(v1, v2)));
    float hx = ((P[0] * p0 + P[1] * p1) + P[2] * p2) + P[3];
    float hy = ((P[4] * p0 + P[5] * p1) + P[6] * p2) + P[7];
    float hw = ((P[12] * p0 + P[13] * p1) + P[14] * p2) + P[15];
    float rw = 1.f / (hw + 1e-6f);
    float px = (0.5f * (float)cam.W) * (hx * rw) + cam.cx - 0.5f;
    float py = (0.5f * (float)cam.H) * (hy * rw) + cam.cy - 0.5f;
    float tcx = px / (float)TILE, tcy = py / (float)TILE, tr = radius / (float)TILE;
    int minx = clampi((int)(tcx - tr), 0, cam.tiles_x), maxx = clampi((int)(tcx + tr + 1.f), 0, cam.tiles_x);
    int miny = clampi((int)(tcy - tr), 0, cam.tiles_y), maxy = clampi((int)(tcy + tr + 1.f), 0, cam.tiles_y);
    int area = (maxx - minx) * (maxy - miny);
    if (area <= 0) return false;
    o.tiles_hit = area; o.depth = tz; o.radius = (int)radius;
    o.xy[0] = px; o.xy[1] = py;
    if (AA) o.comp = rho;
    return true;
}

struct ProjGrad {
    float vm[3], vs[3], vq[4];
    float rho;         // AA only: the compensation of this view, recomputed
};

// True VJP of project_one w.r.t. (mean, scale, raw quat); mirrors oracle orc_project_gaussians_bwd.
// AA: v_rho, the cotangent of the compensation (v_opac * sigmoid(logit)), joins the cotangent of the blurred covariance [[a, b], [b, d]].
// rho is RECOMPUTED here instead of read back from the forward's `compensation` array: T and Sigma are in registers anyway, the 21
// multiply-adds are project_one's own (same operations in the same order under -ffp-contract=off, so the same bits), it saves the 4-byte
// load per Gaussian and view, and it gives the un-blurred a0, d0, from which the derivative has no cancelling term.  With h = 0.3,
// rho^2 = det0 / det and det - det0 = h (a0 + d0 + h):
//     d rho^2 / da = h (d d0 + b^2) / det^2,   d rho^2 / dd = h (a a0 + b^2) / det^2,   d rho^2 / db = -2 b h (a0 + d0 + h) / det^2
// (the forms (s X00 - h detX), (s X11 - h detX), 2 s X01 with s = 1 - rho^2 of the conic X, multiplied out), d rho = d rho^2 / (2 rho).
// b stands for BOTH off-diagonal entries, so each of them takes half of d/db -- the convention of G01 = 0.5 g1 below.  rho == 0 (or a zero
// cotangent, which is all a splat below 1/255 can receive) contributes nothing, and nothing is divided by it.
// one row of a camera matrix applied to (p, 1), in double, rounded to float32 once
__device__ __forceinline__ float dot3(const float *m, float p0, float p1, float p2)
{
    return (float)((((double)m[0] * (double)p0 + (double)m[1] * (double)p1) + (double)m[2] * (double)p2) + (double)m[3]);
}

// POSE (gcx_pose_bwd_views, include/gaussctrl_pose.h): also the cotangents of the two camera matrices, from the values formed here anyway --
// pose[0..11] = v_V [3][4] (the camera-space mean t = V (p, 1) with its depth, and T = J V[:, :3]), pose[12..23] = rows 0, 1, 3 of v_P (the pixel
// centre; row 2 of P is never read).  With AA the v_rho term already sits inside vT.  POSE = false compiles to the code it always was.
template <bool AA = false, bool POSE = false>
__device__ __forceinline__ void project_one_bwd(const Cam &cam, float p0, float p1, float p2, float s0, float s1,
                                                float s2, float qw, float qx, float qy, float qz,
                                                float X00, float X01, float X11, float vx, float vy, float vz,
                                                float g0, float g1, float g2, ProjGrad &o, float v_rho = 0.f, float *pose = nullptr)
{
    const float *V = cam.V, *P = cam.P;
    float hx = ((P[0] * p0 + P[1] * p1) + P[2] * p2) + P[3];
    float hy = ((P[4] * p0 + P[5] * p1) + P[6] * p2) + P[7];
    float hw = ((P[12] * p0 + P[13] * p1) + P[14] * p2) + P[15];
    if (POSE) {      // the camera sums are led by the Gaussians nearest the camera, whose hw (and tz below) cancel from terms fifty times their
                     // size and enter squared in the denominator: formed in double from the same float32 inputs, rounded once (dot3)
        hx = dot3(P, p0, p1, p2); hy = dot3(P + 4, p0, p1, p2); hw = dot3(P + 12, p0, p1, p2);
    }
    float rw = 1.f / (hw + 1e-6f);
    float vnx = 0.5f * (float)cam.W * vx, vny = 0.5f * (float)cam.H * vy;
    float vhx = vnx * rw, vhy = vny * rw, vhw = -(vnx * hx + vny * hy) * rw * rw;
    o.vm[0] = P[0] * vhx + P[4] * vhy + P[12] * vhw;
    o.vm[1] = P[1] * vhx + P[5] * vhy + P[13] * vhw;
    o.vm[2] = P[2] * vhx + P[6] * vhy + P[14] * vhw;
    o.vm[0] += V[8] * vz; o.vm[1] += V[9] * vz; o.vm[2] += V[10] * vz;
    float G00 = g0, G01 = 0.5f * g1, G11 = g2;
    float a00 = X00 * G00 + X01 * G01, a01 = X00 * G01 + X01 * G11;
    float a10 = X01 * G00 + X11 * G01, a11 = X01 * G01 + X11 * G11;
    float C00 = -(a00 * X00 + a01 * X01), C01 = -(a00 * X01 + a01 * X11), C11 = -(a10 * X01 + a11 * X11);
    float tx = ((V[0] * p0 + V[1] * p1) + V[2] * p2) + V[3];
    float ty = ((V[4] * p0 + V[5] * p1) + V[6] * p2) + V[7];
    float tz = ((V[8] * p0 + V[9] * p1) + V[10] * p2) + V[11];
    if (POSE) { tx = dot3(V, p0, p1, p2); ty = dot3(V + 4, p0, p1, p2); tz = dot3(V + 8, p0, p1, p2); }
    float lim_x = 1.3f * (0.5f * (float)cam.W / cam.fx), lim_y = 1.3f * (0.5f * (float)cam.H / cam.fy);
    float rx = tx / tz, ry = ty / tz;
    float rxc = clampf(rx, -lim_x, lim_x), ryc = clampf(ry, -lim_y, lim_y);
    bool clx = (rx != rxc), cly = (ry != ryc);
    float txc = tz * rxc, tyc = tz * ryc;
    float rz = 1.f / tz, rz2 = rz * rz;
    float fx = cam.fx, fy = cam.fy;
    float j00 = fx * rz, j02 = -(fx * txc) * rz2, j11 = fy * rz, j12 = -(fy * tyc) * rz2;
    float T[6] = {j00 * V[0] + j02 * V[8], j00 * V[1] + j02 * V[9], j00 * V[2] + j02 * V[10],
                  j11 * V[4] + j12 * V[8], j11 * V[5] + j12 * V[9], j11 * V[6] + j12 * V[10]};
    Rot rot; float M[9], c3[6];
    quat_to_rotmat(qw, qx, qy, qz, rot);
    scale_rot_to_cov3d(s0, s1, s2, cam.glob, rot.R, c3, M);
    float S[9] = {c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]};
    if (AA) {
        float u00 = (T[0] * c3[0] + T[1] * c3[1]) + T[2] * c3[2];
        float u01 = (T[0] * c3[1] + T[1] * c3[3]) + T[2] * c3[4];
        float u02 = (T[0] * c3[2] + T[1] * c3[4]) + T[2] * c3[5];
        float u10 = (T[3] * c3[0] + T[4] * c3[1]) + T[5] * c3[2];
        float u11 = (T[3] * c3[1] + T[4] * c3[3]) + T[5] * c3[4];
        float u12 = (T[3] * c3[2] + T[4] * c3[4]) + T[5] * c3[5];
        float a0 = (u00 * T[0] + u01 * T[1]) + u02 * T[2];
        float b = (u00 * T[3] + u01 * T[4]) + u02 * T[5];
        float d0 = (u10 * T[3] + u11 * T[4]) + u12 * T[5];
        float a = a0 + 0.3f, d = d0 + 0.3f;
        float det = a * d - b * b;
        float rho = sqrtf(fmaxf(0.f, (a0 * d0 - b * b) / det));      // det != 0: the forward kept this Gaussian
        o.rho = rho;
        if (rho > 0.f && v_rho != 0.f) {
            float k = (0.5f * v_rho / rho) * (0.3f / (det * det));
            C00 += k * (d * d0 + b * b);
            C11 += k * (a * a0 + b * b);
            C01 -= k * (b * ((a0 + d0) + 0.3f));
        }
    }
    float GT[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { GT[k] = C00 * T[k] + C01 * T[3 + k]; GT[3 + k] = C01 * T[k] + C11 * T[3 + k]; }
    float vS[9], vT[6], vM[9], vR[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) vS[3 * r + k] = T[r] * GT[k] + T[3 + r] * GT[3 + k];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            vT[3 * r + k] = 2.f * (GT[3 * r] * S[k] + GT[3 * r + 1] * S[3 + k] + GT[3 * r + 2] * S[6 + k]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            vM[3 * r + k] = 2.f * (vS[3 * r] * M[k] + vS[3 * r + 1] * M[3 + k] + vS[3 * r + 2] * M[6 + k]);
    float sc[3] = {s0, s1, s2};
    const float *R = rot.R;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) vR[3 * r + k] = vM[3 * r + k] * (cam.glob * sc[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.vs[k] = cam.glob * (R[k] * vM[k] + R[3 + k] * vM[3 + k] + R[6 + k] * vM[6 + k]);
    float w = rot.qn[0], x = rot.qn[1], y = rot.qn[2], z = rot.qn[3];
    float vqn[4];
    vqn[0] = 2.f * (x * (vR[7] - vR[5]) + y * (vR[2] - vR[6]) + z * (vR[3] - vR[1]));
    vqn[1] = 2.f * (-2.f * x * (vR[4] + vR[8]) + y * (vR[1] + vR[3]) + z * (vR[2] + vR[6]) + w * (vR[7] - vR[5]));
    vqn[2] = 2.f * (x * (vR[1] + vR[3]) - 2.f * y * (vR[0] + vR[8]) + z * (vR[5] + vR[7]) + w * (vR[2] - vR[6]));
    vqn[3] = 2.f * (x * (vR[2] + vR[6]) + y * (vR[5] + vR[7]) - 2.f * z * (vR[0] + vR[4]) + w * (vR[3] - vR[1]));
    float dotq = rot.qn[0] * vqn[0] + rot.qn[1] * vqn[1] + rot.qn[2] * vqn[2] + rot.qn[3] * vqn[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) o.vq[k] = (vqn[k] - rot.qn[k] * dotq) * rot.inv_norm;
    float vj00 = vT[0] * V[0] + vT[1] * V[1] + vT[2] * V[2];
    float vj02 = vT[0] * V[8] + vT[1] * V[9] + vT[2] * V[10];
    float vj11 = vT[3] * V[4] + vT[4] * V[5] + vT[5] * V[6];
    float vj12 = vT[3] * V[8] + vT[4] * V[9] + vT[5] * V[10];
    float v_rz = fx * vj00 + fy * vj11 - 2.f * rz * (fx * txc * vj02 + fy * tyc * vj12);
    float v_txc = -fx * rz2 * vj02, v_tyc = -fy * rz2 * vj12;
    float v_tz = -rz2 * v_rz, v_tx = 0.f, v_ty = 0.f;
    if (clx) v_tz += rxc * v_txc; else v_tx += v_txc;
    if (cly) v_tz += ryc * v_tyc; else v_ty += v_tyc;
    o.vm[0] += V[0] * v_tx + V[4] * v_ty + V[8] * v_tz;
    o.vm[1] += V[1] * v_tx + V[5] * v_ty + V[9] * v_tz;
    o.vm[2] += V[2] * v_tx + V[6] * v_ty + V[10] * v_tz;
    if (POSE) {
        const float p[3] = {p0, p1, p2};
        const float vt[3] = {v_tx, v_ty, v_tz + vz}, vh[3] = {vhx, vhy, vhw};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { pose[4 * r + k] = vt[r] * p[k]; pose[12 + 4 * r + k] = vh[r] * p[k]; }
            pose[4 * r + 3] = vt[r]; pose[12 + 4 * r + 3] = vh[r];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pose[k] += j00 * vT[k];
            pose[4 + k] += j11 * vT[3 + k];
            pose[8 + k] += j02 * vT[k] + j12 * vT[3 + k];
        }
    }
}

// ---------------------------------------------------------------- SH (Appendix A.2)
__device__ __forceinline__ void sh_basis(int n, float x, float y, float z, float *B)
{
    const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
#pragma unroll
    for (int k = 0; k < 16; ++k) B[k] = 0.f;
    B[0] = C0;
    if (n < 1) return;
    B[1] = -C1 * y; B[2] = C1 * z; B[3] = -C1 * x;
    if (n < 2) return;
    float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    B[4] = 1.0925484305920792f * xy; B[5] = -1.0925484305920792f * yz;
    B[6] = 0.31539156525252005f * (2.f * zz - xx - yy);
    B[7] = -1.0925484305920792f * xz; B[8] = 0.5462742152960396f * (xx - yy);
    if (n < 3) return;
    B[9] = -0.5900435899266435f * y * (3.f * xx - yy);
    B[10] = 2.890611442640554f * xy * z;
    B[11] = -0.4570457994644658f * y * (4.f * zz - xx - yy);
    B[12] = 0.3731763325901154f * z * (2.f * zz - 3.f * xx - 3.f * yy);
    B[13] = -0.4570457994644658f * x * (4.f * zz - xx - yy);
    B[14] = 1.445305721320277f * z * (xx - yy);
    B[15] = -0.5900435899266435f * x * (xx - 3.f * yy);
}

// ---------------------------------------------------------------- kernels: gsplat operator surface
__global__ __launch_bounds__(256) void k_project_fwd(int64_t N, Cam cam, const float *__restrict__ means,
                                                     const float *__restrict__ scales, const float *__restrict__ quats,
                                                     float *__restrict__ cov3d, float *__restrict__ xys,
                                                     float *__restrict__ depths, int32_t *__restrict__ radii,
                                                     float *__restrict__ conics, int32_t *__restrict__ tiles_hit)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    Proj o;
    project_one(cam, means[3 * i], means[3 * i + 1], means[3 * i + 2], scales[3 * i], scales[3 * i + 1],
                scales[3 * i + 2], quats[4 * i], quats[4 * i + 1], quats[4 * i + 2], quats[4 * i + 3], o);
#pragma unroll
    for (int k = 0; k < 6; ++k) cov3d[6 * i + k] = o.cov3d[k];
    xys[2 * i] = o.xy[0]; xys[2 * i + 1] = o.xy[1];
    depths[i] = o.depth; radii[i] = o.radius; tiles_hit[i] = o.tiles_hit;
    conics[3 * i] = o.conic[0]; conics[3 * i + 1] = o.conic[1]; conics[3 * i + 2] = o.conic[2];
}

__global__ __launch_bounds__(256) void k_project_bwd(int64_t N, Cam cam, const float *__restrict__ means,
                                                     const float *__restrict__ scales, const float *__restrict__ quats,
                                                     const int32_t *__restrict__ radii, const float *__restrict__ conics,
                                                     const float *__restrict__ v_xy, const float *__restrict__ v_depth,
                                                     const float *__restrict__ v_conic, float *__restrict__ v_mean,
                                                     float *__restrict__ v_scale, float *__restrict__ v_quat)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    ProjGrad g;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.vm[k] = 0.f; g.vs[k] = 0.f; }
#pragma unroll
    for (int k = 0; k < 4; ++k) g.vq[k] = 0.f;
    if (radii[i] > 0)
        project_one_bwd(cam, means[3 * i], means[3 * i + 1], means[3 * i + 2], scales[3 * i], scales[3 * i + 1],
                        scales[3 * i + 2], quats[4 * i], quats[4 * i + 1], quats[4 * i + 2], quats[4 * i + 3],
                        conics[3 * i], conics[3 * i + 1], conics[3 * i + 2], v_xy[2 * i], v_xy[2 * i + 1],
                        v_depth ? v_depth[i] : 0.f, v_conic[3 * i], v_conic[3 * i + 1], v_conic[3 * i + 2], g);
#pragma unroll
    for (int k = 0; k < 3; ++k) { v_mean[3 * i + k] = g.vm[k]; v_scale[3 * i + k] = g.vs[k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) v_quat[4 * i + k] = g.vq[k];
}

__global__ __launch_bounds__(256) void k_sh_fwd(int64_t N, int K, int n, const float *__restrict__ dirs,
                                                const float *__restrict__ coeffs, float *__restrict__ colors)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float B[16];
    sh_basis(n, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], B);
    int Ku = (n + 1) * (n + 1);
    float acc[3] = {0.f, 0.f, 0.f};
    const float *c = coeffs + (size_t)i * K * 3;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < Ku) {
            acc[0] += B[k] * c[3 * k]; acc[1] += B[k] * c[3 * k + 1]; acc[2] += B[k] * c[3 * k + 2];
        }
    colors[3 * i] = acc[0]; colors[3 * i + 1] = acc[1]; colors[3 * i + 2] = acc[2];
}

__global__ __launch_bounds__(256) void k_sh_bwd(int64_t N, int K, int n, const float *__restrict__ dirs,
                                                const float *__restrict__ v_colors, float *__restrict__ v_coeffs)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float B[16];
    sh_basis(n, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], B);
    int Ku = (n + 1) * (n + 1);
    float v0 = v_colors[3 * i], v1 = v_colors[3 * i + 1], v2 = v_colors[3 * i + 2];
    float *o = v_coeffs + (size_t)i * K * 3;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < K) {
            float b = k < Ku ? B[k] : 0.f;
            o[3 * k] = b * v0; o[3 * k + 1] = b * v1; o[3 * k + 2] = b * v2;
        }
}

// ---------------------------------------------------------------- fused product path: the shared per-view pieces
// One pass over the 59-float record (236 B/Gaussian read, 48 B written).  Mirrors the reference
// op-by-op: exp(scales), q/|q| (gc_model.py:144), project, viewdirs (gc_model.py:163-164),
// SH, clamp(+0.5,min 0) (:167) -- or sigmoid(features_dc) when config.sh_degree == 0 (:169, n_use = -1) -- and sigmoid(opacity) (:181).
//
// The single-view kernels (k_project_sh_fwd / _bwd) and the C-views-per-launch kernels (k_project_sh_fwd_views / _bwd_views) are built from the
// pieces of this section: view c of a batch is bit-identical to the single-view kernel on camera c because both run the SAME code (compiled with
// -ffp-contract=off, so inlining cannot change a bit).  A kernel owns only its memory schedule: loads, barrier, and where the view sums live.
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + __expf(-x)); }

// The camera-independent part of a Gaussian.  load_record only ISSUES the loads (a kernel may put other traffic before their first use).
struct Record {
    float p[3];      // mean
    float s[3];      // log-scale as loaded; exp(.) after activate
    float q[4], qn;  // quaternion as loaded; q/|q| after activate (the outer normalisation, gc_model.py:144), with |q| in qn
    float op;        // opacity logit as loaded; sigmoid(.) after activate
    float d[3];      // features_dc (DC only: the backward does not need it)
};

template <bool DC>
__device__ __forceinline__ void load_record(Record &r, int64_t i, const float *means, const float *log_scales, const float *quats,
        const float *op_logit, const float *f_dc)
{
    r.p[0] = means[3 * i]; r.p[1] = means[3 * i + 1]; r.p[2] = means[3 * i + 2];
    r.s[0] = log_scales[3 * i]; r.s[1] = log_scales[3 * i + 1]; r.s[2] = log_scales[3 * i + 2];
    const float4 q = *reinterpret_cast<const float4 *>(quats + 4 * i);
    r.q[0] = q.x; r.q[1] = q.y; r.q[2] = q.z; r.q[3] = q.w; r.qn = 0.f;
    r.op = op_logit[i];
    r.d[0] = DC ? f_dc[3 * i] : 0.f; r.d[1] = DC ? f_dc[3 * i + 1] : 0.f; r.d[2] = DC ? f_dc[3 * i + 2] : 0.f;
}

__device__ __forceinline__ void activate(Record &r)
{
    r.s[0] = expf(r.s[0]); r.s[1] = expf(r.s[1]); r.s[2] = expf(r.s[2]);
    r.qn = sqrtf(((r.q[0] * r.q[0] + r.q[1] * r.q[1]) + r.q[2] * r.q[2]) + r.q[3] * r.q[3]);
    r.q[0] = r.q[0] / r.qn; r.q[1] = r.q[1] / r.qn; r.q[2] = r.q[2] / r.qn; r.q[3] = r.q[3] / r.qn;
    r.op = sigmoidf(r.op);
}

// HBM access: one lane per Gaussian, but the 45-float features_rest record (180 of the 236 bytes) is NOT read lane-by-lane --
// a 180-byte lane stride makes every load instruction touch 64 different cache lines (rocprofv3 FETCH_SIZE of the round-1 kernel:
// 3.6x the algorithmic bytes).  The workgroup's 256 records are one contiguous 46 KB block: it is streamed with 16-byte-per-lane
// loads into LDS, and each lane then reads ITS record from LDS at a 45-dword stride (odd: bank-conflict free).  The 46 KB of LDS
// allow 3 workgroups per CU.  The caller places the barrier.
template <int R>
__device__ __forceinline__ void stage_rest_in(float *srest, const float *f_rest, int64_t N, int64_t i0, int tid)
{
    const int64_t cnt = ((N - i0 < 256 ? N - i0 : 256)) * R;        // floats of this workgroup's block
    const float *src = f_rest + i0 * R;                              // 256 * R * 4 bytes per block: 16-byte aligned
    for (int64_t j = tid; j < cnt / 4; j += 256) reinterpret_cast<float4 *>(srest)[j] = reinterpret_cast<const float4 *>(src)[j];
    for (int64_t j = (cnt / 4) * 4 + tid; j < cnt; j += 256) srest[j] = src[j];
}

// The way back: the features_rest gradient rows the lanes left in LDS are written with 16-byte-per-lane stores (a lane-strided 45-float
// store has the same 64-lines-per-instruction problem), or, ACC, added to what is there.  Barrier included.
template <int R, bool ACC>
__device__ __forceinline__ void flush_rest_out(const float *svr, float *v_rest, int64_t N, int64_t i0, int tid)
{
    if (R == 0) return;
    __syncthreads();
    const int64_t cnt = ((N - i0 < 256 ? N - i0 : 256)) * R;
    float *dst = v_rest + i0 * R;
    for (int64_t j = tid; j < cnt / 4; j += 256) {
        float4 v = reinterpret_cast<const float4 *>(svr)[j];
        if (ACC) { const float4 o = reinterpret_cast<const float4 *>(dst)[j]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        reinterpret_cast<float4 *>(dst)[j] = v;
    }
    for (int64_t j = (cnt / 4) * 4 + tid; j < cnt; j += 256) dst[j] = ACC ? dst[j] + svr[j] : svr[j];
}

// Tight tile box of the fused path (round 3).  gsplat bins a Gaussian into every tile of the box around a CIRCLE of 3 sqrt(lambda_max);
// a pixel can only pass the compositing test alpha = opacity * exp(-sigma) >= 1/255 inside the ellipse sigma <= tau = ln(255 opacity),
// whose axis-aligned bounding box has half extents sqrt(2 tau cyy / det), sqrt(2 tau cxx / det) (conic = inverse covariance).  For
// anisotropic or faint Gaussians that box is much smaller: intersected with gsplat's box it drops 31 % of the (tile, Gaussian) pairs
// of the synthetic scenes (the exact per-tile test: 37 %) at O(1) per Gaussian.  tau carries the margin of raster_composite.hip's block
// test and the extents a relative + absolute slack, far above the rounding of either side; every tile that is dropped contains no pixel
// that passes the per-pixel test, so images and gradients are bit-identical to the gsplat box.  Packed min_x | max_x << 8 | min_y << 16 |
// max_y << 24 (exclusive maxima; tiles_x, tiles_y <= 255); 0 = no tile.
__device__ __forceinline__ uint32_t tight_tile_box(const Cam &cam, const Proj &o, float opacity)
{
    const float px = o.xy[0], py = o.xy[1];
    const float tcx = px / (float)TILE, tcy = py / (float)TILE, tr = (float)o.radius / (float)TILE;      // gsplat's box (same expressions as project_one)
    int minx = clampi((int)(tcx - tr), 0, cam.tiles_x), maxx = clampi((int)(tcx + tr + 1.f), 0, cam.tiles_x);
    int miny = clampi((int)(tcy - tr), 0, cam.tiles_y), maxy = clampi((int)(tcy + tr + 1.f), 0, cam.tiles_y);
    const float cxx = o.conic[0], cxy = o.conic[1], cyy = o.conic[2];
    const float det = cxx * cyy - cxy * cxy;
    const float tau = logf(255.f * opacity) * 1.001f + 0.01f;
    if (tau < 0.f) return 0u;                                            // can never reach 1/255 anywhere
    if (cxx > 0.f && cyy > 0.f && det > 0.f && tau >= 0.f) {             // (NaN / degenerate conic: keep gsplat's box)
        const float ex = sqrtf(2.f * tau * cyy / det) * 1.0001f + 1e-3f, ey = sqrtf(2.f * tau * cxx / det) * 1.0001f + 1e-3f;
        const float x0 = ceilf(px - ex), x1 = floorf(px + ex), y0 = ceilf(py - ey), y1 = floorf(py + ey);      // pixel centres inside
        if (!(x0 <= x1 && y0 <= y1)) return 0u;
        const int tx0 = (int)floorf(x0 / (float)TILE), tx1 = (int)floorf(x1 / (float)TILE) + 1;
        const int ty0 = (int)floorf(y0 / (float)TILE), ty1 = (int)floorf(y1 / (float)TILE) + 1;
        minx = minx > tx0 ? minx : tx0; maxx = maxx < tx1 ? maxx : tx1;
        miny = miny > ty0 ? miny : ty0; maxy = maxy < ty1 ? maxy : ty1;
    }
    if (maxx <= minx || maxy <= miny) return 0u;
    return (uint32_t)minx | ((uint32_t)maxx << 8) | ((uint32_t)miny << 16) | ((uint32_t)maxy << 24);
}

// Projects Gaussian `id` for one camera and stores the view's projection state at element index o (o = id for a single view, view * N + id
// in a batch).  tile_box (optional): the tight box, and the tiles_hit it implies -- nth and the box the emission walks shrink together.
// depth_pairs (optional): the depth-order sort's input pair.  Returns project_one's verdict.
// AA: the view's effective opacity sigmoid(logit) * rho goes to opac[o] and rho to compensation[o] (both per view), and the tight box is the
// effective opacity's -- smaller, by the same argument: no dropped tile holds a pixel that passes alpha >= 1/255.
template <bool AA = false>
__device__ __forceinline__ bool store_view(const Cam &cam, const Record &r, int64_t o, int64_t id, float *xys, float *depths, int32_t *radii,
        float *conics, int32_t *tiles_hit, uint32_t *tile_box, uint2 *depth_pairs, float *opac = nullptr, float *compensation = nullptr)
{
    Proj pr;
    const bool ok = project_one<AA>(cam, r.p[0], r.p[1], r.p[2], r.s[0], r.s[1], r.s[2], r.q[0], r.q[1], r.q[2], r.q[3], pr);
    xys[2 * o] = pr.xy[0]; xys[2 * o + 1] = pr.xy[1];
    const float op_v = AA ? r.op * pr.comp : r.op;
    if (AA) { opac[o] = op_v; compensation[o] = pr.comp; }
    if (tile_box) {
        uint32_t box = 0;
        if (ok) box = tight_tile_box(cam, pr, op_v);
        tile_box[o] = box;
        pr.tiles_hit = (int)(((box >> 8) & 255u) - (box & 255u)) * (int)((box >> 24) - ((box >> 16) & 255u));
    }
    depths[o] = pr.depth; radii[o] = pr.radius; tiles_hit[o] = pr.tiles_hit;
    conics[3 * o] = pr.conic[0]; conics[3 * o + 1] = pr.conic[1]; conics[3 * o + 2] = pr.conic[2];
    if (depth_pairs) depth_pairs[o] = make_uint2(pr.radius > 0 ? __float_as_uint(pr.depth) : 0xFFFFFFFFu, (uint32_t)id);
    return ok;
}

// Unit vector from the camera origin to the mean (gc_model.py:163-164) -> SH basis up to degree n_use.
__device__ __forceinline__ void view_basis(const Cam &cam, const Record &r, int n_use, float *B)
{
    float dx = r.p[0] - cam.ox, dy = r.p[1] - cam.oy, dz = r.p[2] - cam.oz;
    float dn = sqrtf((dx * dx + dy * dy) + dz * dz);
    dx = dx / dn; dy = dy / dn; dz = dz / dn;
    sh_basis(n_use, dx, dy, dz, B);
}

// Colour of the Gaussian for one camera; rest = the lane's features_rest row in LDS (read only when n_use > 0).  0 when !ok.
template <int K>
__device__ __forceinline__ float3 shade(const Cam &cam, const Record &r, const float *rest, int n_use, bool ok)
{
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (ok) {
        if (n_use < 0) {          // config.sh_degree == 0: rgbs = sigmoid(features_dc)   (gc_model.py:169)
            c0 = sigmoidf(r.d[0]); c1 = sigmoidf(r.d[1]); c2 = sigmoidf(r.d[2]);
        } else {
            float B[16];
            view_basis(cam, r, n_use, B);
            c0 = B[0] * r.d[0]; c1 = B[0] * r.d[1]; c2 = B[0] * r.d[2];
            int Ku = (n_use + 1) * (n_use + 1);
#pragma unroll
            for (int k = 1; k < K; ++k)
                if (k < Ku) {
                    c0 += B[k] * rest[3 * (k - 1)]; c1 += B[k] * rest[3 * (k - 1) + 1]; c2 += B[k] * rest[3 * (k - 1) + 2];
                }
            c0 = fmaxf(c0 + 0.5f, 0.f); c1 = fmaxf(c1 + 0.5f, 0.f); c2 = fmaxf(c2 + 0.5f, 0.f);
        }
    }
    return make_float3(c0, c1, c2);
}

// Leaf-gradient stores: written, or (ACC) added to what is there; put4 is one 16-byte access.
template <bool ACC> __device__ __forceinline__ void put(float *p, float v) { *p = ACC ? *p + v : v; }
template <bool ACC>
__device__ __forceinline__ void put4(float *p, const float *v)
{
    float4 v4 = make_float4(v[0], v[1], v[2], v[3]);
    if (ACC) { const float4 o = *reinterpret_cast<const float4 *>(p); v4.x += o.x; v4.y += o.y; v4.z += o.z; v4.w += o.w; }
    *reinterpret_cast<float4 *>(p) = v4;
}

// Gradient of one view to the leaves of one Gaussian the view did not cull (radii > 0), all per-view inputs at element index o; in two parts
// so that a kernel may store the first before it computes the second.  GeomGrad: the VJP of store_view, to means / log-scales / quaternion /
// opacity logit.  DEPTH (gc_project_sh_bwd_depth_views): v_depths feeds project_one_bwd's depth argument (depth = row 2 of the view matrix
// applied to the mean); without it the argument is the literal 0 it always was.
struct GeomGrad { float vm[3], gls[3], gq[4], gop; };

template <bool DEPTH, bool AA = false>
__device__ __forceinline__ void geom_vjp(const Cam &cam, const Record &r, int64_t o, const float *conics, const float *v_xy, const float *v_conic,
                                         const float *v_opac, const float *v_depths, GeomGrad &g)
{
    ProjGrad pg;
    project_one_bwd<AA>(cam, r.p[0], r.p[1], r.p[2], r.s[0], r.s[1], r.s[2], r.q[0], r.q[1], r.q[2], r.q[3], conics[3 * o], conics[3 * o + 1],
                        conics[3 * o + 2], v_xy[2 * o], v_xy[2 * o + 1], DEPTH ? v_depths[o] : 0.f, v_conic[3 * o], v_conic[3 * o + 1],
                        v_conic[3 * o + 2], pg, AA ? v_opac[o] * r.op : 0.f);      // AA: v_opac is of the view's sigmoid(logit) * rho
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.vm[k] = pg.vm[k]; g.gls[k] = pg.vs[k] * r.s[k]; }
    // outer normalisation q/|q| (gc_model.py:144)
    const float dq = r.q[0] * pg.vq[0] + r.q[1] * pg.vq[1] + r.q[2] * pg.vq[2] + r.q[3] * pg.vq[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) g.gq[k] = (pg.vq[k] - r.q[k] * dq) / r.qn;
    g.gop = AA ? (v_opac[o] * pg.rho) * r.op * (1.f - r.op) : v_opac[o] * r.op * (1.f - r.op);
}

// ColourGrad: the VJP of shade.  It needs only the FORWARD colours (rgbs): the clamp(min = 0) mask is rgbs > 0 and the sigmoid mode's
// derivative is s (1 - s), so the 192-byte SH record is not re-read.  gdc goes to features_dc; the features_rest row is B[k] * v[.] for
// 1 <= k < Ku and 0 beyond (rest_row).
struct ColourGrad { float gdc[3], v[3], B[16]; int Ku; };

__device__ __forceinline__ void colour_vjp(const Cam &cam, const Record &r, int64_t o, int n_use, const float *rgbs, const float *v_rgbs,
                                           ColourGrad &g)
{
    const float c[3] = {rgbs[3 * o], rgbs[3 * o + 1], rgbs[3 * o + 2]};
    if (n_use < 0) {        // d sigmoid(features_dc)
#pragma unroll
        for (int k = 0; k < 3; ++k) { g.gdc[k] = v_rgbs[3 * o + k] * c[k] * (1.f - c[k]); g.v[k] = 0.f; }
#pragma unroll
        for (int k = 0; k < 16; ++k) g.B[k] = 0.f;
        g.Ku = 0;
    } else {
        view_basis(cam, r, n_use, g.B);
        g.Ku = (n_use + 1) * (n_use + 1);
        // clamp(SH + 0.5, min 0) (gc_model.py:167): the gradient passes where the forward colour is positive
#pragma unroll
        for (int k = 0; k < 3; ++k) { g.v[k] = c[k] > 0.f ? v_rgbs[3 * o + k] : 0.f; g.gdc[k] = g.B[0] * g.v[k]; }
    }
}

// The view's features_rest gradient row into the lane's LDS row: assigned, or (ADD) added to the running sum.
template <int K, bool ADD>
__device__ __forceinline__ void rest_row(float *vr, const ColourGrad &g)
{
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const float b = k < g.Ku ? g.B[k] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) vr[3 * (k - 1) + c] = ADD ? vr[3 * (k - 1) + c] + b * g.v[c] : b * g.v[c];
    }
}

// ---------------------------------------------------------------- kernels: fused product path, one camera
// AA: opac is the view's effective opacity and compensation its rho (store_view); the AA = false instantiation never touches `compensation`.
template <int K, bool AA = false>
__global__ __launch_bounds__(256) void k_project_sh_fwd(int64_t N, Cam cam, int n_use, const float *__restrict__ means,
        const float *__restrict__ log_scales, const float *__restrict__ quats, const float *__restrict__ op_logit, const float *__restrict__ f_dc,
        const float *__restrict__ f_rest, float *__restrict__ xys, float *__restrict__ depths, int32_t *__restrict__ radii,
        float *__restrict__ conics, int32_t *__restrict__ tiles_hit, float *__restrict__ rgbs, float *__restrict__ opac,
        uint32_t *__restrict__ tile_box, float *__restrict__ compensation)
{
    constexpr int R = (K - 1) * 3;                         // floats of features_rest per Gaussian
    __shared__ __attribute__((aligned(16))) float srest[R > 0 ? 256 * R : 4];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + tid;
    // the lane's own record is requested BEFORE the cooperative staging of the SH block, so that the two HBM round trips overlap
    // (3 workgroups per CU -- the 46 KB of LDS -- leave little else to hide them behind), and projected before the barrier
    Record r;
    load_record<true>(r, i < N ? i : N - 1, means, log_scales, quats, op_logit, f_dc);
    if (R > 0 && n_use > 0) stage_rest_in<R>(srest, f_rest, N, i0, tid);
    bool ok = false;
    if (i < N) {
        activate(r);
        ok = store_view<AA>(cam, r, i, i, xys, depths, radii, conics, tiles_hit, tile_box, nullptr, opac, compensation);
        if (!AA) opac[i] = r.op;
    }
    if (R > 0 && n_use > 0) __syncthreads();
    if (i >= N) return;
    const float3 c = shade<K>(cam, r, srest + tid * R, n_use, ok);
    rgbs[3 * i] = c.x; rgbs[3 * i + 1] = c.y; rgbs[3 * i + 2] = c.z;
}

// Backward of the above.  ACC: the six outputs are accumulated into (+=) instead of written -- gradient accumulation over the views of a
// batch without a separate read-add-write pass per tensor (the caller owns zeroing / the first view runs with ACC = false).
// AA: v_opac is the cotangent of the view's effective opacity (geom_vjp / project_one_bwd).
template <int K, bool ACC, bool DEPTH = false, bool AA = false>
__global__ __launch_bounds__(256) void k_project_sh_bwd(int64_t N, Cam cam, int n_use, const float *__restrict__ means,
        const float *__restrict__ log_scales, const float *__restrict__ quats, const float *__restrict__ op_logit, const float *__restrict__ rgbs,
        const int32_t *__restrict__ radii, const float *__restrict__ conics, const float *__restrict__ v_xy, const float *__restrict__ v_conic,
        const float *__restrict__ v_rgbs, const float *__restrict__ v_opac, float *__restrict__ v_means, float *__restrict__ v_ls,
        float *__restrict__ v_quats, float *__restrict__ v_oplogit, float *__restrict__ v_dc, float *__restrict__ v_rest,
        const float *__restrict__ v_depths)
{
    constexpr int R = (K - 1) * 3;
    __shared__ __attribute__((aligned(16))) float svr[R > 0 ? 256 * R : 4];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + tid;
    float *vr = svr + tid * R;
    if (i < N) {
        if (radii[i] <= 0) {
            if (!ACC) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { v_means[3 * i + k] = 0.f; v_ls[3 * i + k] = 0.f; v_dc[3 * i + k] = 0.f; }
                *reinterpret_cast<float4 *>(v_quats + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
                v_oplogit[i] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < R; ++k) vr[k] = 0.f;
        } else {
            Record r;
            load_record<false>(r, i, means, log_scales, quats, op_logit, nullptr);
            activate(r);
            GeomGrad g;
            geom_vjp<DEPTH, AA>(cam, r, i, conics, v_xy, v_conic, v_opac, v_depths, g);
#pragma unroll
            for (int k = 0; k < 3; ++k) { put<ACC>(v_means + 3 * i + k, g.vm[k]); put<ACC>(v_ls + 3 * i + k, g.gls[k]); }
            put4<ACC>(v_quats + 4 * i, g.gq);
            put<ACC>(v_oplogit + i, g.gop);
            ColourGrad c;
            colour_vjp(cam, r, i, n_use, rgbs, v_rgbs, c);
#pragma unroll
            for (int k = 0; k < 3; ++k) put<ACC>(v_dc + 3 * i + k, c.gdc[k]);
            rest_row<K, false>(vr, c);
        }
    }
    flush_rest_out<R, ACC>(svr, v_rest, N, i0, tid);
}

// ---------------------------------------------------------------- kernels: C views per launch (round 5)
// The 236-byte parameter record of a Gaussian does not depend on the camera: a launch over C views reads it ONCE (the SH block staged
// through LDS once) and projects / shades it for every view of the batch, instead of C launches that each stream the whole record again --
// 236 + C * 60 bytes per Gaussian instead of C * 296.  Per view it runs store_view and shade, the code of the single-view kernel: every output
// of view c is bit-identical to what gc_project_sh_fwd[_boxes] writes for that camera.  Per-view outputs are [C][N][..]; `opac` (sigmoid of
// the opacity logit, camera independent) is written once, [N]; depth_pairs (optional) are the depth-order sort's input pairs.
// AA: opac and compensation are per view, [C][N] (what the compositing kernels take with shared_opacities = 0).
constexpr int MAXV = 8;
struct CamBatch { Cam cam[MAXV]; int C; };

template <int K, bool AA = false>
__global__ __launch_bounds__(256) void k_project_sh_fwd_views(int64_t N, CamBatch cb, int n_use, const float *__restrict__ means,
        const float *__restrict__ log_scales, const float *__restrict__ quats, const float *__restrict__ op_logit, const float *__restrict__ f_dc,
        const float *__restrict__ f_rest, float *__restrict__ xys, float *__restrict__ depths, int32_t *__restrict__ radii,
        float *__restrict__ conics, int32_t *__restrict__ tiles_hit, float *__restrict__ rgbs, float *__restrict__ opac,
        uint32_t *__restrict__ tile_box, uint2 *__restrict__ depth_pairs, float *__restrict__ compensation)
{
    constexpr int R = (K - 1) * 3;
    __shared__ __attribute__((aligned(16))) float srest[R > 0 ? 256 * R : 4];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + tid;
    Record r;
    load_record<true>(r, i < N ? i : N - 1, means, log_scales, quats, op_logit, f_dc);
    if (R > 0 && n_use > 0) {      // staged once for all views: the barrier stands before the view loop
        stage_rest_in<R>(srest, f_rest, N, i0, tid);
        __syncthreads();
    }
    if (i >= N) return;
    activate(r);
    if (!AA) opac[i] = r.op;
    for (int v = 0; v < cb.C; ++v) {
        const Cam &cam = cb.cam[v];
        const int64_t o = (int64_t)v * N + i;
        const bool ok = store_view<AA>(cam, r, o, i, xys, depths, radii, conics, tiles_hit, tile_box, depth_pairs, opac, compensation);
        const float3 c = shade<K>(cam, r, srest + tid * R, n_use, ok);
        rgbs[3 * o] = c.x; rgbs[3 * o + 1] = c.y; rgbs[3 * o + 2] = c.z;
    }
}

// Backward over C views: the parameter record is read once, the per-view VJPs (geom_vjp + colour_vjp, the code of the single-view kernel) are summed
// in registers IN VIEW ORDER -- ((g_0 + g_1) + g_2) ..., the order C accumulating single-view launches produce -- and the 59 gradient floats
// are written (or, ACC, added to what is there) ONCE per batch: N * (56 + C * 64) bytes read + N * 236 written instead of C * N * 344.
template <int K, bool ACC, bool DEPTH = false, bool AA = false>
__global__ __launch_bounds__(256) void k_project_sh_bwd_views(int64_t N, CamBatch cb, int n_use, const float *__restrict__ means,
        const float *__restrict__ log_scales, const float *__restrict__ quats, const float *__restrict__ op_logit, const float *__restrict__ rgbs,
        const int32_t *__restrict__ radii, const float *__restrict__ conics, const float *__restrict__ v_xy, const float *__restrict__ v_conic,
        const float *__restrict__ v_rgbs, const float *__restrict__ v_opac, float *__restrict__ v_means, float *__restrict__ v_ls,
        float *__restrict__ v_quats, float *__restrict__ v_oplogit, float *__restrict__ v_dc, float *__restrict__ v_rest,
        const float *__restrict__ v_depths /* [C][N], DEPTH only */)
{
    constexpr int R = (K - 1) * 3;
    __shared__ __attribute__((aligned(16))) float svr[R > 0 ? 256 * R : 4];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + tid;
    float *vr = svr + tid * R;
    if (i < N) {
        float am[3] = {0.f, 0.f, 0.f}, as[3] = {0.f, 0.f, 0.f}, aq[4] = {0.f, 0.f, 0.f, 0.f}, aop = 0.f, adc[3] = {0.f, 0.f, 0.f};
        // (the 45 features_rest sums live in the lane's own LDS row -- the staging buffer of the coalesced store below; in registers the
        // kernel needs 173 VGPRs = 2 workgroups per CU, with them in LDS the 46 KB of LDS is the limit again: 3 per CU)
#pragma unroll
        for (int k = 0; k < R; ++k) vr[k] = 0.f;
        bool first = true;          // the first contributing view ASSIGNS (0 + g would turn a -0 into +0: keep the single-view bits)
        Record r;
        load_record<false>(r, i, means, log_scales, quats, op_logit, nullptr);
        activate(r);
        for (int v = 0; v < cb.C; ++v) {
            const int64_t o = (int64_t)v * N + i;
            if (radii[o] <= 0) continue;
            GeomGrad g;
            geom_vjp<DEPTH, AA>(cb.cam[v], r, o, conics, v_xy, v_conic, v_opac, v_depths, g);
            ColourGrad c;
            colour_vjp(cb.cam[v], r, o, n_use, rgbs, v_rgbs, c);
            if (first) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { am[k] = g.vm[k]; as[k] = g.gls[k]; adc[k] = c.gdc[k]; }
#pragma unroll
                for (int k = 0; k < 4; ++k) aq[k] = g.gq[k];
                aop = g.gop;
                rest_row<K, false>(vr, c);
                first = false;
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) { am[k] = am[k] + g.vm[k]; as[k] = as[k] + g.gls[k]; adc[k] = adc[k] + c.gdc[k]; }
#pragma unroll
                for (int k = 0; k < 4; ++k) aq[k] = aq[k] + g.gq[k];
                aop = aop + g.gop;
                rest_row<K, true>(vr, c);
            }
        }
        if (!ACC || !first) {       // (ACC and no view contributed: nothing to add)
#pragma unroll
            for (int k = 0; k < 3; ++k) { put<ACC>(v_means + 3 * i + k, am[k]); put<ACC>(v_ls + 3 * i + k, as[k]); put<ACC>(v_dc + 3 * i + k, adc[k]); }
            put4<ACC>(v_quats + 4 * i, aq);
            put<ACC>(v_oplogit + i, aop);
        }
    }
    flush_rest_out<R, ACC>(svr, v_rest, N, i0, tid);
}

// ---------------------------------------------------------------- kernels: camera (pose) gradient over C views (include/gaussctrl_pose.h)
// The 24 camera cotangents of project_one_bwd<AA, true>, summed over the Gaussians of each view.  The CamBatch walk of k_project_sh_bwd_views: the
// record is read once and serves every view of the launch.  A workgroup covers POSE_ITEMS * 256 consecutive Gaussians; per (Gaussian, view) a
// wave folds its 64 x 24 values to 24 with a reduce-scatter (each of the first three steps halves the values a lane still owns: 12 + 6 + 3
// exchanges, then 3 x 3 butterfly steps -- 30 cross-lane moves instead of 144) and adds them to its own LDS row; the four rows are added in wave
// order into one float32 partial per (workgroup, view) in the caller's workspace, [C][workgroups][24].  k_pose_sum adds a view's partials in a
// fixed order in double.  No atomics anywhere: the same bits every run.  A view in which no lane of a wave kept its Gaussian costs that wave
// one ballot.
constexpr int POSE_ITEMS = 4, POSE_VALS = 24;

__device__ __forceinline__ void pose_wave_fold(float *v /* [24] -> the lane's 3 totals in v[0..2] */, int lane)
{
    const bool up5 = (lane & 32) != 0, up4 = (lane & 16) != 0, up3 = (lane & 8) != 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) {      // 24 -> 12: the upper half-wave keeps values 12..23
        const float keep = up5 ? v[12 + j] : v[j], send = up5 ? v[j] : v[12 + j];
        v[j] = keep + __shfl_xor(send, 32);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {       // 12 -> 6
        const float keep = up4 ? v[6 + j] : v[j], send = up4 ? v[j] : v[6 + j];
        v[j] = keep + __shfl_xor(send, 16);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {       // 6 -> 3
        const float keep = up3 ? v[3 + j] : v[j], send = up3 ? v[j] : v[3 + j];
        v[j] = keep + __shfl_xor(send, 8);
    }
#pragma unroll
    for (int off = 4; off >= 1; off >>= 1)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = v[j] + __shfl_xor(v[j], off);
}

template <bool AA>
__global__ __launch_bounds__(256) void k_pose_bwd_views(int64_t N, CamBatch cb, int64_t nblk, const float *__restrict__ means,
        const float *__restrict__ log_scales, const float *__restrict__ quats, const float *__restrict__ op_logit,
        const int32_t *__restrict__ radii, const float *__restrict__ conics, const float *__restrict__ v_xy, const float *__restrict__ v_conic,
        const float *__restrict__ v_opac, const float *__restrict__ v_depths /* may be NULL */, float *__restrict__ partials /* this launch's views */)
{
    __shared__ float acc[4][MAXV][POSE_VALS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < 4 * MAXV * POSE_VALS; j += 256) (&acc[0][0][0])[j] = 0.f;
    __syncthreads();
    // the three values this lane ends a fold with: 12 (bit 5) + 6 (bit 4) + 3 (bit 3) of its lane number; lanes 0, 8, .., 56 store them
    const int slot = ((lane >> 5) & 1) * 12 + ((lane >> 4) & 1) * 6 + ((lane >> 3) & 1) * 3;
    const int64_t i0 = (int64_t)blockIdx.x * (256 * POSE_ITEMS);
    for (int it = 0; it < POSE_ITEMS; ++it) {
        const int64_t i = i0 + (int64_t)it * 256 + tid;
        if (i0 + (int64_t)it * 256 >= N) break;                       // (uniform over the workgroup)
        const bool live = i < N;
        Record r;
        load_record<false>(r, live ? i : N - 1, means, log_scales, quats, op_logit, nullptr);
        activate(r);
        for (int v = 0; v < cb.C; ++v) {
            const int64_t o = (int64_t)v * N + (live ? i : N - 1);
            const bool kept = live && radii[o] > 0;
            if (__ballot(kept) == 0ull) continue;                     // (uniform over the wave)
            float pose[POSE_VALS];
#pragma unroll
            for (int k = 0; k < POSE_VALS; ++k) pose[k] = 0.f;
            if (kept) {
                ProjGrad pg;
                project_one_bwd<AA, true>(cb.cam[v], r.p[0], r.p[1], r.p[2], r.s[0], r.s[1], r.s[2], r.q[0], r.q[1], r.q[2], r.q[3],
                                          conics[3 * o], conics[3 * o + 1], conics[3 * o + 2], v_xy[2 * o], v_xy[2 * o + 1],
                                          v_depths ? v_depths[o] : 0.f, v_conic[3 * o], v_conic[3 * o + 1], v_conic[3 * o + 2], pg,
                                          AA ? v_opac[o] * r.op : 0.f, pose);
            }
            pose_wave_fold(pose, lane);
            if ((lane & 7) == 0) {                                    // the wave's own row: no other wave touches it, program order suffices
                float *a = &acc[wave][v][slot];
                a[0] = a[0] + pose[0]; a[1] = a[1] + pose[1]; a[2] = a[2] + pose[2];
            }
        }
    }
    __syncthreads();
    if (tid < cb.C * POSE_VALS) {
        const int v = tid / POSE_VALS, k = tid % POSE_VALS;
        partials[((int64_t)v * nblk + blockIdx.x) * POSE_VALS + k] = ((acc[0][v][k] + acc[1][v][k]) + acc[2][v][k]) + acc[3][v][k];
    }
}

// One workgroup per view: thread (s, k) = (tid / 24, tid % 24), s < 10, adds the partials s, s + 10, s + 20, ... of value k in double; thread k
// then adds the ten slice sums in slice order and rounds to float32 once.
__global__ __launch_bounds__(256) void k_pose_sum(int64_t nblk, const float *__restrict__ partials, float *__restrict__ out)
{
    constexpr int SLICES = 10;
    __shared__ double part[SLICES][POSE_VALS];
    const int tid = threadIdx.x, s = tid / POSE_VALS, k = tid % POSE_VALS;
    const float *p = partials + (int64_t)blockIdx.x * nblk * POSE_VALS;
    if (s < SLICES) {
        double sum = 0.0;
        for (int64_t b = s; b < nblk; b += SLICES) sum = sum + (double)p[b * POSE_VALS + k];
        part[s][k] = sum;
    }
    __syncthreads();
    if (tid < POSE_VALS) {
        double sum = part[0][tid];
#pragma unroll
        for (int j = 1; j < SLICES; ++j) sum = sum + part[j][tid];
        out[(int64_t)blockIdx.x * POSE_VALS + tid] = (float)sum;
    }
}

// img_out == img_raw: in place.  Otherwise the un-clamped image stays where the compositing wrote it (the backward needs it for the
// clamp's gradient mask) and the clamped one goes to img_out: no separate copy pass.
__global__ __launch_bounds__(256) void k_finalize(int64_t npix, const float *img_raw, float *img_out, float *__restrict__ extra,
                                                  const float *__restrict__ final_T, float *__restrict__ alpha)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    float a = 1.f - final_T[i];
    alpha[i] = a;
    const float r = img_raw[3 * i], g = img_raw[3 * i + 1], b = img_raw[3 * i + 2];
    img_out[3 * i] = fminf(r, 1.f); img_out[3 * i + 1] = fminf(g, 1.f); img_out[3 * i + 2] = fminf(b, 1.f);
    if (extra) extra[i] = a > 0.f ? extra[i] / a : 1000.f;
}

Cam make_cam(const float *viewmat, const float *projmat, float fx, float fy, float cx, float cy, int H, int W,
             int tx, int ty, float clip, float glob, const float *origin)
{
    Cam c;
    for (int k = 0; k < 12; ++k) c.V[k] = viewmat[k];
    for (int k = 0; k < 16; ++k) c.P[k] = projmat[k];
    c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.H = H; c.W = W; c.tiles_x = tx; c.tiles_y = ty;
    c.clip = clip; c.glob = glob;
    c.ox = origin ? origin[0] : 0.f; c.oy = origin ? origin[1] : 0.f; c.oz = origin ? origin[2] : 0.f;
    return c;
}


// ---------------------------------------------------------------- host side of the fused product path
// What the entry points of one direction share, in the order of their C parameter lists; the extern "C" wrappers fill one and name themselves.
struct FwdArgs {
    int64_t N;
    const float *means, *log_scales, *quats, *opacity_logits, *features_dc, *features_rest;
    int sh_degree, degrees_to_use, img_h, img_w, tiles_x, tiles_y;
    float clip_thresh, *xys, *depths;
    int32_t *radii; float *conics; int32_t *num_tiles_hit;
    float *rgbs, *opac;
    uint32_t *tile_boxes;                                                 // NULL: gsplat's boxes
    void *stream;
    float *compensation = nullptr;                                        // non-NULL: antialiased mode, opac and compensation per view
};

struct BwdArgs {
    int64_t N;
    const float *means, *log_scales, *quats, *opacity_logits, *rgbs;      // rgbs ... v_opac: per view, [C][N][..] for the batched entries
    int sh_degree, degrees_to_use, img_h, img_w;
    const int32_t *radii;
    const float *conics, *v_xy, *v_conic, *v_rgbs, *v_opac;
    float *v_means, *v_log_scales, *v_quats, *v_opacity_logits, *v_features_dc, *v_features_rest;
    const float *v_depths;                                                // NULL: the entries without a depth gradient
    void *stream;
    bool antialiased = false;                                             // v_opac is of the per-view effective opacity
};

struct CamArgs { const float *viewmat, *projmat, *origin; float fx, fy, cx, cy; };      // one camera, HOST pointers

// one view of a `cams` array: viewmat[12] | projmat[16] | cam_origin[3] | fx fy cx cy (GC_VIEW_CAM_FLOATS = 35)
CamArgs packed_cam(const float *c) { return CamArgs{c, c + 12, c + 28, c[31], c[32], c[33], c[34]}; }

Cam make_cam(const CamArgs &c, int H, int W, int tx, int ty, float clip) { return make_cam(c.viewmat, c.projmat, c.fx, c.fy, c.cx, c.cy, H, W, tx, ty, clip, 1.f, c.origin); }

CamBatch make_cams(const float *cams, int v0, int nv, int img_h, int img_w, int tx, int ty, float clip)
{
    CamBatch cb;
    cb.C = nv;
    for (int v = 0; v < nv; ++v) cb.cam[v] = make_cam(packed_cam(cams + (size_t)(v0 + v) * 35), img_h, img_w, tx, ty, clip);
    return cb;
}

// The template instantiation for a run-time choice: f is called with a std::integral_constant.
template <class F>
void for_sh_degree(int sh_degree, F f)       // f(K): K = (sh_degree + 1)^2 SH bases
{
    switch (sh_degree) {
    case 0: f(std::integral_constant<int, 1>{}); break;
    case 1: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 9>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
    }
}

template <class F>
void for_flag(bool b, F f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

// Launches for one camera (Cam) or one group of views (CamBatch); o = element offset of the group's first view in the per-view arrays.
template <int K, bool AA> constexpr auto project_sh_fwd_kernel(const Cam &) { return k_project_sh_fwd<K, AA>; }
template <int K, bool AA> constexpr auto project_sh_fwd_kernel(const CamBatch &) { return k_project_sh_fwd_views<K, AA>; }
template <int K, bool ACC, bool DEPTH, bool AA> constexpr auto project_sh_bwd_kernel(const Cam &) { return k_project_sh_bwd<K, ACC, DEPTH, AA>; }
template <int K, bool ACC, bool DEPTH, bool AA> constexpr auto project_sh_bwd_kernel(const CamBatch &) { return k_project_sh_bwd_views<K, ACC, DEPTH, AA>; }


template <class CamT, class... Pairs>       // Pairs: the batched kernel's trailing depth_pairs
void launch_project_sh_fwd(const FwdArgs &a, const CamT &cam, size_t o, Pairs... pairs)
{
    for_sh_degree(a.sh_degree, [&](auto K) { for_flag(a.compensation != nullptr, [&](auto AA) {
        hipLaunchKernelGGL((project_sh_fwd_kernel<decltype(K)::value, decltype(AA)::value>(cam)), dim3(gc::cdiv(a.N, 256)), dim3(256), 0,
                           gc::S(a.stream), a.N, cam, a.degrees_to_use, a.means, a.log_scales, a.quats, a.opacity_logits, a.features_dc,
                           a.features_rest, a.xys + 2 * o, a.depths + o, a.radii + o, a.conics + 3 * o, a.num_tiles_hit + o, a.rgbs + 3 * o,
                           a.compensation ? a.opac + o : a.opac, a.tile_boxes ? a.tile_boxes + o : nullptr, pairs...,
                           a.compensation ? a.compensation + o : nullptr);
    }); });
}

template <class CamT>
void launch_project_sh_bwd(const BwdArgs &a, const CamT &cam, bool acc, size_t o)
{
    for_sh_degree(a.sh_degree, [&](auto K) { for_flag(acc, [&](auto ACC) { for_flag(a.v_depths != nullptr, [&](auto DEPTH) { for_flag(a.antialiased, [&](auto AA) {
        hipLaunchKernelGGL((project_sh_bwd_kernel<decltype(K)::value, decltype(ACC)::value, decltype(DEPTH)::value, decltype(AA)::value>(cam)),
                           dim3(gc::cdiv(a.N, 256)), dim3(256), 0, gc::S(a.stream), a.N, cam, a.degrees_to_use, a.means, a.log_scales,
                           a.quats, a.opacity_logits, a.rgbs + 3 * o, a.radii + o, a.conics + 3 * o, a.v_xy + 2 * o, a.v_conic + 3 * o,
                           a.v_rgbs + 3 * o, a.v_opac + o, a.v_means, a.v_log_scales, a.v_quats, a.v_opacity_logits, a.v_features_dc,
                           a.v_features_rest, a.v_depths ? a.v_depths + o : nullptr);
    }); }); }); });
}

int project_sh_fwd_impl(const char *what, const FwdArgs &a, const CamArgs &c)
{
    GC_REQUIRE(a.sh_degree >= 0 && a.sh_degree <= 3 && a.degrees_to_use >= -1 && a.degrees_to_use <= a.sh_degree, "SH degree must be 0..3 (degrees_to_use -1: sigmoid colour mode)");
    GC_REQUIRE(c.viewmat && c.projmat && c.origin, "camera pointers are host pointers and must not be NULL");
    if (a.N == 0) return GC_OK;
    launch_project_sh_fwd(a, make_cam(c, a.img_h, a.img_w, a.tiles_x, a.tiles_y, a.clip_thresh), 0);
    return gc::check_launch(what);
}

int project_sh_bwd_impl(const char *what, bool accumulate, const BwdArgs &a, const CamArgs &c)
{
    GC_REQUIRE(a.sh_degree >= 0 && a.sh_degree <= 3 && a.degrees_to_use >= -1 && a.degrees_to_use <= a.sh_degree, "SH degree must be 0..3 (degrees_to_use -1: sigmoid colour mode)");
    GC_REQUIRE(c.viewmat && c.projmat && c.origin, "camera pointers are host pointers and must not be NULL");
    if (a.N == 0) return GC_OK;
    launch_project_sh_bwd(a, make_cam(c, a.img_h, a.img_w, 0, 0, 0.f), accumulate, 0);
    return gc::check_launch(what);
}

// Views are processed in groups of 8 (one launch per group: the cameras travel as kernel arguments); a later group adds to the first one's sums.
int project_sh_bwd_views_impl(const char *what, int C, int accumulate, const BwdArgs &a, const float *cams)
{
    GC_REQUIRE(a.sh_degree >= 0 && a.sh_degree <= 3 && a.degrees_to_use >= -1 && a.degrees_to_use <= a.sh_degree, "SH degree must be 0..3 (degrees_to_use -1: sigmoid colour mode)");
    GC_REQUIRE(cams && C >= 1, "cams is a host pointer and must not be NULL");
    if (a.N == 0) return GC_OK;
    for (int v0 = 0; v0 < C; v0 += MAXV)
        launch_project_sh_bwd(a, make_cams(cams, v0, C - v0 < MAXV ? C - v0 : MAXV, a.img_h, a.img_w, 0, 0, 0.f), accumulate || v0 > 0,
                              (size_t)v0 * (size_t)a.N);
    return gc::check_launch(what);
}

int64_t pose_workgroups(int64_t N) { return N > 0 ? (N + 256 * POSE_ITEMS - 1) / (256 * POSE_ITEMS) : 0; }

}  // namespace

extern "C" {

/* ---- Camera (pose) gradient of the front end: include/gaussctrl_pose.h.  One float32 partial [24] per (view, workgroup of 1024 Gaussians). */
size_t gcx_pose_bwd_views_workspace_bytes(int64_t N, int C)
{
    if (N <= 0 || C < 1) return 0;
    return (size_t)C * (size_t)pose_workgroups(N) * POSE_VALS * sizeof(float);
}

int gcx_pose_bwd_views(int64_t N, int C, int antialiased, const float *means, const float *log_scales, const float *quats,
        const float *opacity_logits, const float *cams, int img_h, int img_w, const int32_t *radii, const float *conics, const float *v_xy,
        const float *v_conic, const float *v_opac, const float *v_depths, void *workspace, float *out, void *stream)
{
    GC_REQUIRE(N >= 0 && C >= 1 && cams, "N >= 0, C >= 1; cams is a host pointer and must not be NULL");
    GC_REQUIRE((int64_t)C * N * 3 < (1ll << 31), "C * N * 3 must be < 2^31 elements");
    GC_REQUIRE(img_h > 0 && img_w > 0, "the image must not be empty");
    GC_REQUIRE(out, "out is NULL");
    if (N == 0) {
        if (hipMemsetAsync(out, 0, (size_t)C * 2 * 12 * sizeof(float), gc::S(stream)) != hipSuccess) return gc::check_launch("gcx_pose_bwd_views");
        return GC_OK;
    }
    GC_REQUIRE(means && log_scales && quats && opacity_logits && radii && conics, "an input pointer is NULL");
    GC_REQUIRE(v_xy && v_conic && (v_opac || !antialiased), "a cotangent pointer is NULL (v_opac may be NULL only when antialiased == 0)");
    GC_REQUIRE(workspace, "workspace is NULL");
    const int64_t nblk = pose_workgroups(N);
    float *partials = (float *)workspace;
    for (int v0 = 0; v0 < C; v0 += MAXV) {
        const CamBatch cb = make_cams(cams, v0, C - v0 < MAXV ? C - v0 : MAXV, img_h, img_w, 0, 0, 0.f);
        const size_t o = (size_t)v0 * (size_t)N;
        for_flag(antialiased != 0, [&](auto AA) {
            hipLaunchKernelGGL((k_pose_bwd_views<decltype(AA)::value>), dim3((unsigned)nblk), dim3(256), 0, gc::S(stream), N, cb, nblk, means,
                               log_scales, quats, opacity_logits, radii + o, conics + 3 * o, v_xy + 2 * o, v_conic + 3 * o,
                               v_opac ? v_opac + o : nullptr, v_depths ? v_depths + o : nullptr, partials + (size_t)v0 * nblk * POSE_VALS);
        });
    }
    hipLaunchKernelGGL(k_pose_sum, dim3((unsigned)C), dim3(256), 0, gc::S(stream), nblk, (const float *)partials, out);
    return gc::check_launch("gcx_pose_bwd_views");
}

int gc_project_gaussians_fwd(int64_t N, const float *means3d, const float *scales, float glob_scale,
                             const float *quats, const float *viewmat, const float *projmat, float fx, float fy,
                             float cx, float cy, int img_h, int img_w, int tiles_x, int tiles_y, float clip_thresh,
                             float *cov3d, float *xys, float *depths, int32_t *radii, float *conics,
                             int32_t *num_tiles_hit, void *stream)
{
    GC_REQUIRE(N >= 0 && viewmat && projmat, "bad arguments");
    if (N == 0) return GC_OK;
    Cam cam = make_cam(viewmat, projmat, fx, fy, cx, cy, img_h, img_w, tiles_x, tiles_y, clip_thresh, glob_scale, nullptr);
    hipLaunchKernelGGL(k_project_fwd, dim3(gc::cdiv(N, 256)), dim3(256), 0, gc::S(stream), N, cam, means3d, scales,
                       quats, cov3d, xys, depths, radii, conics, num_tiles_hit);
    return gc::check_launch("gc_project_gaussians_fwd");
}

int gc_project_gaussians_bwd(int64_t N, const float *means3d, const float *scales, float glob_scale,
                             const float *quats, const float *viewmat, const float *projmat, float fx, float fy,
                             float cx, float cy, int img_h, int img_w, const int32_t *radii, const float *conics,
                             const float *v_xy, const float *v_depth, const float *v_conic, float *v_mean3d,
                             float *v_scale, float *v_quat, void *stream)
{
    GC_REQUIRE(N >= 0 && viewmat && projmat, "bad arguments");
    if (N == 0) return GC_OK;
    Cam cam = make_cam(viewmat, projmat, fx, fy, cx, cy, img_h, img_w, 0, 0, 0.f, glob_scale, nullptr);
    hipLaunchKernelGGL(k_project_bwd, dim3(gc::cdiv(N, 256)), dim3(256), 0, gc::S(stream), N, cam, means3d, scales,
                       quats, radii, conics, v_xy, v_depth, v_conic, v_mean3d, v_scale, v_quat);
    return gc::check_launch("gc_project_gaussians_bwd");
}

int gc_sh_fwd(int64_t N, int degree, int degrees_to_use, const float *viewdirs, const float *coeffs, float *colors,
              void *stream)
{
    GC_REQUIRE(degree >= 0 && degree <= 3 && degrees_to_use >= 0 && degrees_to_use <= degree, "SH degree must be 0..3");
    if (N == 0) return GC_OK;
    int K = (degree + 1) * (degree + 1);
    hipLaunchKernelGGL(k_sh_fwd, dim3(gc::cdiv(N, 256)), dim3(256), 0, gc::S(stream), N, K, degrees_to_use, viewdirs,
                       coeffs, colors);
    return gc::check_launch("gc_sh_fwd");
}

int gc_sh_bwd(int64_t N, int degree, int degrees_to_use, const float *viewdirs, const float *v_colors,
              float *v_coeffs, void *stream)
{
    GC_REQUIRE(degree >= 0 && degree <= 3 && degrees_to_use >= 0 && degrees_to_use <= degree, "SH degree must be 0..3");
    if (N == 0) return GC_OK;
    int K = (degree + 1) * (degree + 1);
    hipLaunchKernelGGL(k_sh_bwd, dim3(gc::cdiv(N, 256)), dim3(256), 0, gc::S(stream), N, K, degrees_to_use, viewdirs,
                       v_colors, v_coeffs);
    return gc::check_launch("gc_sh_bwd");
}

int gc_project_sh_fwd(int64_t N, const float *means, const float *log_scales, const float *quats, const float *opacity_logits,
        const float *features_dc, const float *features_rest, int sh_degree, int degrees_to_use, const float *viewmat, const float *projmat,
        const float *cam_origin, float fx, float fy, float cx, float cy, int img_h, int img_w, int tiles_x, int tiles_y, float clip_thresh,
        float *xys, float *depths, int32_t *radii, float *conics, int32_t *num_tiles_hit, float *rgbs, float *opac, void *stream)
{
    const FwdArgs a{N, means, log_scales, quats, opacity_logits, features_dc, features_rest, sh_degree, degrees_to_use, img_h, img_w, tiles_x,
                    tiles_y, clip_thresh, xys, depths, radii, conics, num_tiles_hit, rgbs, opac, nullptr, stream};
    return project_sh_fwd_impl("gc_project_sh_fwd", a, CamArgs{viewmat, projmat, cam_origin, fx, fy, cx, cy});
}

/* The same with TIGHT tile boxes: tile_boxes[N] (packed, see tight_tile_box) and num_tiles_hit count only the tiles of the bounding box
 * of the alpha >= 1/255 ellipse inside gsplat's box; feed both to gc_raster_depth_order / gc_raster_bin_tiles_boxes. */
int gc_project_sh_fwd_boxes(int64_t N, const float *means, const float *log_scales, const float *quats, const float *opacity_logits,
        const float *features_dc, const float *features_rest, int sh_degree, int degrees_to_use, const float *viewmat, const float *projmat,
        const float *cam_origin, float fx, float fy, float cx, float cy, int img_h, int img_w, int tiles_x, int tiles_y, float clip_thresh,
        float *xys, float *depths, int32_t *radii, float *conics, int32_t *num_tiles_hit, float *rgbs, float *opac, uint32_t *tile_boxes,
        void *stream)
{
    GC_REQUIRE(tile_boxes && tiles_x <= 255 && tiles_y <= 255, "tile_boxes required; packed boxes hold at most 255 x 255 tiles (use gc_project_sh_fwd beyond)");
    const FwdArgs a{N, means, log_scales, quats, opacity_logits, features_dc, features_rest, sh_degree, degrees_to_use, img_h, img_w, tiles_x,
                    tiles_y, clip_thresh, xys, depths, radii, conics, num_tiles_hit, rgbs, opac, tile_boxes, stream};
    return project_sh_fwd_impl("gc_project_sh_fwd_boxes", a, CamArgs{viewmat, projmat, cam_origin, fx, fy, cx, cy});
}

int gc_project_sh_bwd(int64_t N, const float *means, const float *log_scales, const float *quats, const float *opacity_logits, const float *rgbs,
        int sh_degree, int degrees_to_use, const float *viewmat, const float *projmat, const float *cam_origin, float fx, float fy, float cx,
        float cy, int img_h, int img_w, const int32_t *radii, const float *conics, const float *v_xy, const float *v_conic, const float *v_rgbs,
        const float *v_opac, float *v_means, float *v_log_scales, float *v_quats, float *v_opacity_logits, float *v_features_dc,
        float *v_features_rest, void *stream)
{
    const BwdArgs a{N, means, log_scales, quats, opacity_logits, rgbs, sh_degree, degrees_to_use, img_h, img_w, radii, conics, v_xy, v_conic, v_rgbs,
                    v_opac, v_means, v_log_scales, v_quats, v_opacity_logits, v_features_dc, v_features_rest, nullptr, stream};
    return project_sh_bwd_impl("gc_project_sh_bwd", false, a, CamArgs{viewmat, projmat, cam_origin, fx, fy, cx, cy});
}

/* Same, but the six outputs are ACCUMULATED into (+=): gradient accumulation over the views of a batch inside the kernel. */
int gc_project_sh_bwd_accumulate(int64_t N, const float *means, const float *log_scales, const float *quats, const float *opacity_logits,
        const float *rgbs, int sh_degree, int degrees_to_use, const float *viewmat, const float *projmat, const float *cam_origin, float fx, float fy,
        float cx, float cy, int img_h, int img_w, const int32_t *radii, const float *conics, const float *v_xy, const float *v_conic,
        const float *v_rgbs, const float *v_opac, float *v_means, float *v_log_scales, float *v_quats, float *v_opacity_logits, float *v_features_dc,
        float *v_features_rest, void *stream)
{
    const BwdArgs a{N, means, log_scales, quats, opacity_logits, rgbs, sh_degree, degrees_to_use, img_h, img_w, radii, conics, v_xy, v_conic, v_rgbs,
                    v_opac, v_means, v_log_scales, v_quats, v_opacity_logits, v_features_dc, v_features_rest, nullptr, stream};
    return project_sh_bwd_impl("gc_project_sh_bwd_accumulate", true, a, CamArgs{viewmat, projmat, cam_origin, fx, fy, cx, cy});
}

/* ---- C views per launch (round 5).  cams: HOST float array [C][GC_VIEW_CAM_FLOATS = 35] = viewmat[12] | projmat[16] | cam_origin[3] |
 * fx fy cx cy per view; all views share H, W and the tile grid.  Views are processed in groups of 8 (one launch per group: the cameras
 * travel as kernel arguments); outputs are [C][N][..] except opac [N].  tile_boxes / depth_pairs optional (NULL). */
int gc_project_sh_fwd_views(int64_t N, int C, const float *means, const float *log_scales, const float *quats, const float *opacity_logits,
        const float *features_dc, const float *features_rest, int sh_degree, int degrees_to_use, const float *cams, int img_h, int img_w, int tiles_x,
        int tiles_y, float clip_thresh, float *xys, float *depths, int32_t *radii, float *conics, int32_t *num_tiles_hit, float *rgbs, float *opac,
        uint32_t *tile_boxes, uint32_t *depth_pairs, void *stream)
{
    GC_REQUIRE(sh_degree >= 0 && sh_degree <= 3 && degrees_to_use >= -1 && degrees_to_use <= sh_degree, "SH degree must be 0..3 (degrees_to_use -1: sigmoid colour mode)");
    GC_REQUIRE(cams && C >= 1, "cams is a host pointer and must not be NULL");
    GC_REQUIRE(!tile_boxes || (tiles_x <= 255 && tiles_y <= 255), "packed boxes hold at most 255 x 255 tiles");
    if (N == 0) return GC_OK;
    const FwdArgs a{N, means, log_scales, quats, opacity_logits, features_dc, features_rest, sh_degree, degrees_to_use, img_h, img_w, tiles_x,
                    tiles_y, clip_thresh, xys, depths, radii, conics, num_tiles_hit, rgbs, opac, tile_boxes, stream};
    for (int v0 = 0; v0 < C; v0 += MAXV)
        launch_project_sh_fwd(a, make_cams(cams, v0, C - v0 < MAXV ? C - v0 : MAXV, img_h, img_w, tiles_x, tiles_y, clip_thresh),
                              (size_t)v0 * (size_t)N, depth_pairs ? (uint2 *)depth_pairs + (size_t)v0 * (size_t)N : nullptr);
    return gc::check_launch("gc_project_sh_fwd_views");
}

/* Backward over C views: rgbs / radii / conics / v_xy / v_conic / v_rgbs / v_opac are [C][N][..]; the six leaf gradients are the SUM over
 * the views, written (accumulate = 0) or added to the buffers' contents (accumulate = 1) once per group of 8 views. */
int gc_project_sh_bwd_views(int64_t N, int C, int accumulate, const float *means, const float *log_scales, const float *quats,
        const float *opacity_logits, const float *rgbs, int sh_degree, int degrees_to_use, const float *cams, int img_h, int img_w,
        const int32_t *radii, const float *conics, const float *v_xy, const float *v_conic, const float *v_rgbs, const float *v_opac, float *v_means,
        float *v_log_scales, float *v_quats, float *v_opacity_logits, float *v_features_dc, float *v_features_rest, void *stream)
{
    const BwdArgs a{N, means, log_scales, quats, opacity_logits, rgbs, sh_degree, degrees_to_use, img_h, img_w, radii, conics, v_xy, v_conic, v_rgbs,
                    v_opac, v_means, v_log_scales, v_quats, v_opacity_logits, v_features_dc, v_features_rest, nullptr, stream};
    return project_sh_bwd_views_impl("gc_project_sh_bwd_views", C, accumulate, a, cams);
}

/* The same with a gradient on the projected depths: v_depths [C][N] (the v_extra of gc_rasterize_bwd_depth_views) enters each view's VJP as
 * d depth / d mean = row 2 of that view's matrix; a culled Gaussian (radii == 0) contributes nothing.  C = 1 runs the single-view kernel. */
int gc_project_sh_bwd_depth_views(int64_t N, int C, int accumulate, const float *means, const float *log_scales, const float *quats,
        const float *opacity_logits, const float *rgbs, int sh_degree, int degrees_to_use, const float *cams, int img_h, int img_w,
        const int32_t *radii, const float *conics, const float *v_xy, const float *v_conic, const float *v_rgbs, const float *v_opac, float *v_means,
        float *v_log_scales, float *v_quats, float *v_opacity_logits, float *v_features_dc, float *v_features_rest, const float *v_depths,
        void *stream)
{
    GC_REQUIRE(v_depths, "v_depths is required (gc_project_sh_bwd_views is the form without it)");
    const BwdArgs a{N, means, log_scales, quats, opacity_logits, rgbs, sh_degree, degrees_to_use, img_h, img_w, radii, conics, v_xy, v_conic, v_rgbs,
                    v_opac, v_means, v_log_scales, v_quats, v_opacity_logits, v_features_dc, v_features_rest, v_depths, stream};
    if (C == 1 && cams) return project_sh_bwd_impl("gc_project_sh_bwd_depth_views", accumulate != 0, a, packed_cam(cams));
    return project_sh_bwd_views_impl("gc_project_sh_bwd_depth_views", C, accumulate, a, cams);
}

/* ---- Antialiased rasterize_mode (include/gaussctrl_antialias.h).  The forward over C views with the per-view opacity compensation: opac
 * [C][N] = sigmoid(logit) * rho, compensation [C][N] = rho; everything else is what gc_project_sh_fwd_views writes, except that the tight
 * boxes are the effective opacity's.  C = 1 without depth_pairs runs the single-view kernel (same per-view code, same bits). */
int gc_project_sh_fwd_aa_views(int64_t N, int C, const float *means, const float *log_scales, const float *quats, const float *opacity_logits,
        const float *features_dc, const float *features_rest, int sh_degree, int degrees_to_use, const float *cams, int img_h, int img_w, int tiles_x,
        int tiles_y, float clip_thresh, float *xys, float *depths, int32_t *radii, float *conics, int32_t *num_tiles_hit, float *rgbs, float *opac,
        float *compensation, uint32_t *tile_boxes, uint32_t *depth_pairs, void *stream)
{
    GC_REQUIRE(N >= 0 && C >= 1 && cams, "N >= 0, C >= 1; cams is a host pointer and must not be NULL");
    GC_REQUIRE(sh_degree >= 0 && sh_degree <= 3 && degrees_to_use >= -1 && degrees_to_use <= sh_degree, "SH degree must be 0..3 (degrees_to_use -1: sigmoid colour mode)");
    GC_REQUIRE(img_h > 0 && img_w > 0 && tiles_x > 0 && tiles_y > 0, "image and tile grid must not be empty");
    GC_REQUIRE(!tile_boxes || (tiles_x <= 255 && tiles_y <= 255), "packed boxes hold at most 255 x 255 tiles");
    if (N == 0) return GC_OK;
    GC_REQUIRE(means && log_scales && quats && opacity_logits && features_dc && (features_rest || sh_degree == 0), "a parameter pointer is NULL");
    GC_REQUIRE(xys && depths && radii && conics && num_tiles_hit && rgbs && opac && compensation, "an output pointer is NULL");
    FwdArgs a{N, means, log_scales, quats, opacity_logits, features_dc, features_rest, sh_degree, degrees_to_use, img_h, img_w, tiles_x,
              tiles_y, clip_thresh, xys, depths, radii, conics, num_tiles_hit, rgbs, opac, tile_boxes, stream};
    a.compensation = compensation;
    if (C == 1 && !depth_pairs)
        launch_project_sh_fwd(a, make_cam(packed_cam(cams), img_h, img_w, tiles_x, tiles_y, clip_thresh), 0);
    else
        for (int v0 = 0; v0 < C; v0 += MAXV)
            launch_project_sh_fwd(a, make_cams(cams, v0, C - v0 < MAXV ? C - v0 : MAXV, img_h, img_w, tiles_x, tiles_y, clip_thresh),
                                  (size_t)v0 * (size_t)N, depth_pairs ? (uint2 *)depth_pairs + (size_t)v0 * (size_t)N : nullptr);
    return gc::check_launch("gc_project_sh_fwd_aa_views");
}

/* Its backward: the arguments of gc_project_sh_bwd_depth_views, v_opac [C][N] being the cotangent of the per-view effective opacity (what the
 * compositing backward returns with shared_opacities = 0).  v_depths may be NULL (no depth term).  `compensation` is the forward's array: it is
 * validated and part of the contract, but the kernels recompute rho from the covariance they rebuild anyway (see project_one_bwd). */
int gc_project_sh_bwd_aa_views(int64_t N, int C, int accumulate, const float *means, const float *log_scales, const float *quats,
        const float *opacity_logits, const float *rgbs, int sh_degree, int degrees_to_use, const float *cams, int img_h, int img_w,
        const int32_t *radii, const float *conics, const float *compensation, const float *v_xy, const float *v_conic, const float *v_rgbs,
        const float *v_opac, float *v_means, float *v_log_scales, float *v_quats, float *v_opacity_logits, float *v_features_dc,
        float *v_features_rest, const float *v_depths, void *stream)
{
    GC_REQUIRE(N >= 0 && C >= 1 && cams, "N >= 0, C >= 1; cams is a host pointer and must not be NULL");
    GC_REQUIRE(sh_degree >= 0 && sh_degree <= 3 && degrees_to_use >= -1 && degrees_to_use <= sh_degree, "SH degree must be 0..3 (degrees_to_use -1: sigmoid colour mode)");
    if (N == 0) return GC_OK;
    GC_REQUIRE(means && log_scales && quats && opacity_logits && rgbs && radii && conics && compensation, "an input pointer is NULL");
    GC_REQUIRE(v_xy && v_conic && v_rgbs && v_opac, "a cotangent pointer is NULL");
    GC_REQUIRE(v_means && v_log_scales && v_quats && v_opacity_logits && v_features_dc && (v_features_rest || sh_degree == 0), "an output pointer is NULL");
    BwdArgs a{N, means, log_scales, quats, opacity_logits, rgbs, sh_degree, degrees_to_use, img_h, img_w, radii, conics, v_xy, v_conic, v_rgbs,
              v_opac, v_means, v_log_scales, v_quats, v_opacity_logits, v_features_dc, v_features_rest, v_depths, stream};
    a.antialiased = true;
    if (C == 1) return project_sh_bwd_impl("gc_project_sh_bwd_aa_views", accumulate != 0, a, packed_cam(cams));
    return project_sh_bwd_views_impl("gc_project_sh_bwd_aa_views", C, accumulate, a, cams);
}

int gc_raster_finalize(int64_t num_pixels, float *out_img, float *out_extra, const float *final_Ts, float *alpha,
                       void *stream)
{
    if (num_pixels == 0) return GC_OK;
    hipLaunchKernelGGL(k_finalize, dim3(gc::cdiv(num_pixels, 256)), dim3(256), 0, gc::S(stream), num_pixels, (const float *)out_img, out_img,
                       out_extra, final_Ts, alpha);
    return gc::check_launch("gc_raster_finalize");
}

int gc_raster_finalize_into(int64_t num_pixels, const float *img_raw, float *img_clamped, float *out_extra, const float *final_Ts,
                            float *alpha, void *stream)
{
    if (num_pixels == 0) return GC_OK;
    GC_REQUIRE(img_raw && img_clamped && img_raw != img_clamped, "needs two distinct image buffers (gc_raster_finalize is the in-place form)");
    hipLaunchKernelGGL(k_finalize, dim3(gc::cdiv(num_pixels, 256)), dim3(256), 0, gc::S(stream), num_pixels, img_raw, img_clamped,
                       out_extra, final_Ts, alpha);
    return gc::check_launch("gc_raster_finalize_into");
}

}  // extern "C"

/*
 * frame_math.h -- cv::Mat's float arithmetic on the device as pinned in DESIGN.md "Pinned semantics", every operation
 * stated with a rounding intrinsic so that nothing contracts, and Frame::isInFrustum (Frame.cc:274-330) of one
 * MapPoint built from it: the one definition behind k_frustum and k_local_frustum (local_kernels.hip). The same
 * sequence on the host: frustum.c; in Python: tests/frustum_py.py. Likewise Frame::UnprojectStereo of one keypoint
 * (unproject_point: k_unproject and the stereo branches below) and one match of LocalMapping::CreateNewMapPoints
 * (triangulate_match, LocalMapping.cc:284-450 with MapPoint::UpdateNormalAndDepth: k_create_map_points,
 * triangulate_kernels.hip; on the host triangulate.c, in Python tests/triangulate_py.py).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbslam_amd.h"
#include "orb_math.h"

namespace orbamd {

/* (A x)[r] + c of the small-matrix gemm: a0 x0 + a1 x1 + a2 x2 in float, then (float)((double)t + (double)c) */
__device__ __forceinline__ float gemm_row(float a0, float a1, float a2, float x0, float x1, float x2, float c) {
    const float t = __fadd_rn(__fadd_rn(__fmul_rn(a0, x0), __fmul_rn(a1, x1)), __fmul_rn(a2, x2));
    return __double2float_rn(__dadd_rn((double)t, (double)c));
}

/* (-A.t() x)[i] of a row-major 3x4 [R | t] block (GEMM_1_T): s = 0; s += (double)A[k][i] * (double)x[k]; -1.0 * s */
__device__ __forceinline__ float gemm_t_neg(const float* T, int i, float x0, float x1, float x2) {
    double s = __dadd_rn(0.0, __dmul_rn((double)T[i], (double)x0));
    s = __dadd_rn(s, __dmul_rn((double)T[4 + i], (double)x1));
    s = __dadd_rn(s, __dmul_rn((double)T[8 + i], (double)x2));
    return __double2float_rn(__dmul_rn(-1.0, s));
}

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

/* a frame's pose for isInFrustum: rows 0..2 of mTcw, mOw = -mRcw.t() * mtcw, and whether all twelve are finite */
struct FrustumPose {
    float T[12];
    float Ow[3];
    bool ok;
};
__device__ __forceinline__ FrustumPose frustum_pose(const float* Tcw) {
    FrustumPose p;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        p.T[k] = Tcw[k];
        ok = ok && finite_f(p.T[k]);
    }
    p.ok = ok;
#pragma unroll
    for (int i = 0; i < 3; i++) p.Ow[i] = gemm_t_neg(p.T, i, p.T[3], p.T[7], p.T[11]);
    return p;
}

struct FrustumResult {
    float u, v, xr, view_cos;
    int level;
};

/* Frame::isInFrustum + MapPoint::PredictScale of one point: 1 = in view (r filled), 0 = rejected by a test of the
 * reference, -1 = excluded by the contract (include/orbslam_amd.h: the reference's behaviour is undefined there);
 * r is all zeros unless 1 is returned. */
__device__ __forceinline__ int frustum_point(const orbm_track_geom& g, float log_scale_factor, const FrustumPose& p,
                                             float cos_limit, const float* P, const float* Pn, float min_dist,
                                             float max_dist, FrustumResult& r) {
    r.u = r.v = r.xr = r.view_cos = 0.0f;
    r.level = 0;
    const float X = P[0], Y = P[1], Z = P[2], n0 = Pn[0], n1 = Pn[1], n2 = Pn[2];
    if (!p.ok || !finite_f(X) || !finite_f(Y) || !finite_f(Z) || !finite_f(n0) || !finite_f(n1) || !finite_f(n2) ||
        !finite_f(min_dist) || !finite_f(max_dist))
        return -1;
    const float PcX = gemm_row(p.T[0], p.T[1], p.T[2], X, Y, Z, p.T[3]);
    const float PcY = gemm_row(p.T[4], p.T[5], p.T[6], X, Y, Z, p.T[7]);
    const float PcZ = gemm_row(p.T[8], p.T[9], p.T[10], X, Y, Z, p.T[11]);
    if (!finite_f(PcX) || !finite_f(PcY) || !finite_f(PcZ)) return -1;
    if (PcZ < 0.0f) return 0;
    if (PcZ == 0.0f) return -1;
    const float invz = __fdiv_rn(1.0f, PcZ);
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(g.fx, PcX), invz), g.cx);
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(g.fy, PcY), invz), g.cy);
    if (!finite_f(u) || !finite_f(v)) return -1;
    if (u < g.min_x || u > g.max_x) return 0;
    if (v < g.min_y || v > g.max_y) return 0;
    const float po0 = __fsub_rn(X, p.Ow[0]), po1 = __fsub_rn(Y, p.Ow[1]), po2 = __fsub_rn(Z, p.Ow[2]);
    double s = __dadd_rn(0.0, __dmul_rn((double)po0, (double)po0));
    s = __dadd_rn(s, __dmul_rn((double)po1, (double)po1));
    s = __dadd_rn(s, __dmul_rn((double)po2, (double)po2));
    const float dist = __double2float_rn(__dsqrt_rn(s));
    if (!finite_f(dist) || dist == 0.0f) return -1;
    if (dist < __fmul_rn(0.8f, min_dist) || dist > __fmul_rn(1.2f, max_dist)) return 0;
    double d = __dadd_rn(0.0, __dmul_rn((double)po0, (double)n0));
    d = __dadd_rn(d, __dmul_rn((double)po1, (double)n1));
    d = __dadd_rn(d, __dmul_rn((double)po2, (double)n2));
    const float view_cos = __double2float_rn(__ddiv_rn(d, (double)dist));
    if (!finite_f(view_cos)) return -1;
    if (view_cos < cos_limit) return 0;
    const float ratio = __fdiv_rn(max_dist, dist);
    if (!logf_domain(ratio)) return -1;
    const float fl = ceilf(__fdiv_rn(glibc_logf(ratio), log_scale_factor));
    r.level = fl < 0.0f ? 0 : fl >= (float)g.nlevels ? g.nlevels - 1 : (int)fl;
    r.u = u;
    r.v = v;
    r.xr = __fsub_rn(u, __fmul_rn(g.bf, invz));
    r.view_cos = view_cos;
    return 1;
}

/* Frame::UnprojectStereo (Frame.cc:667-681) of one keypoint with z > 0: x3Dc = ((u - cx) z invfx, (v - cy) z invfy,
 * z), p = mRwc * x3Dc + mOw (row i of mRwc = column i of mRcw) */
__device__ __forceinline__ void unproject_point(float cx, float cy, float invfx, float invfy, const float* T,
                                                const float* Ow, float u, float v, float z, float* p) {
    const float x = __fmul_rn(__fmul_rn(__fsub_rn(u, cx), z), invfx);
    const float y = __fmul_rn(__fmul_rn(__fsub_rn(v, cy), z), invfy);
    p[0] = gemm_row(T[0], T[4], T[8], x, y, z, Ow[0]);
    p[1] = gemm_row(T[1], T[5], T[9], x, y, z, Ow[1]);
    p[2] = gemm_row(T[2], T[6], T[10], x, y, z, Ow[2]);
}

__device__ __forceinline__ double dot3_d(float a0, float a1, float a2, float b0, float b1, float b2) {
    double s = __dadd_rn(0.0, __dmul_rn((double)a0, (double)b0));
    s = __dadd_rn(s, __dmul_rn((double)a1, (double)b1));
    return __dadd_rn(s, __dmul_rn((double)a2, (double)b2));
}
__device__ __forceinline__ double dot4_d(const float* a, const float* b) {
    double s = __dadd_rn(0.0, __dmul_rn((double)a[0], (double)b[0]));
    s = __dadd_rn(s, __dmul_rn((double)a[1], (double)b[1]));
    s = __dadd_rn(s, __dmul_rn((double)a[2], (double)b[2]));
    return __dadd_rn(s, __dmul_rn((double)a[3], (double)b[3]));
}

/* vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a 4x4 float A, given as At = A.t(): OpenCV 3.x's
 * one-sided Jacobi (include/orbslam_amd.h states it). The (i, j, k) loops are unrolled so that At, Vt and W stay in
 * registers; only the sweep loop remains. */
__device__ __forceinline__ void svd4_null(float (&At)[4][4], float* x) {
    float Vt[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int k = 0; k < 4; k++) Vt[i][k] = i == k ? 1.0f : 0.0f;
        W[i] = dot4_d(At[i], At[i]);
    }
    const double eps = (double)(2 * 1.1920928955078125e-7f);
#pragma unroll 1
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = i + 1; j < 4; j++) {
                double a = W[i], b = W[j];
                double p = dot4_d(At[i], At[j]);
                if (!(fabs(p) <= __dmul_rn(eps, __dsqrt_rn(__dmul_rn(a, b))))) {
                    p = __dmul_rn(p, 2.0);
                    const double beta = __dsub_rn(a, b);
                    const double gamma = __dsqrt_rn(__dadd_rn(__dmul_rn(p, p), __dmul_rn(beta, beta)));
                    float c, s;
                    if (beta < 0) {
                        const double delta = __dmul_rn(__dsub_rn(gamma, beta), 0.5);
                        s = __double2float_rn(__dsqrt_rn(__ddiv_rn(delta, gamma)));
                        c = __double2float_rn(__ddiv_rn(p, __dmul_rn(__dmul_rn(gamma, (double)s), 2.0)));
                    } else {
                        c = __double2float_rn(__dsqrt_rn(__ddiv_rn(__dadd_rn(gamma, beta), __dmul_rn(gamma, 2.0))));
                        s = __double2float_rn(__ddiv_rn(p, __dmul_rn(__dmul_rn(gamma, (double)c), 2.0)));
                    }
                    a = b = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float t0 = __fadd_rn(__fmul_rn(c, At[i][k]), __fmul_rn(s, At[j][k]));
                        const float t1 = __fadd_rn(__fmul_rn(-s, At[i][k]), __fmul_rn(c, At[j][k]));
                        At[i][k] = t0;
                        At[j][k] = t1;
                        a = __dadd_rn(a, __dmul_rn((double)t0, (double)t0));
                        b = __dadd_rn(b, __dmul_rn((double)t1, (double)t1));
                        const float v0 = __fadd_rn(__fmul_rn(c, Vt[i][k]), __fmul_rn(s, Vt[j][k]));
                        const float v1 = __fadd_rn(__fmul_rn(-s, Vt[i][k]), __fmul_rn(c, Vt[j][k]));
                        Vt[i][k] = v0;
                        Vt[j][k] = v1;
                    }
                    W[i] = a;
                    W[j] = b;
                    changed = true;
                }
            }
        }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) W[i] = __dsqrt_rn(dot4_d(At[i], At[i]));
    // selection sort, descending, strict <: row j moves to i; only the Vt rows are still needed
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; k++)
            if (wj < W[k]) {
                j = k;
                wj = W[k];
            }
#pragma unroll
        for (int k = i + 1; k < 4; k++)
            if (j == k) {
                const double w = W[i];
                W[i] = W[k];
                W[k] = w;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const float t = Vt[i][m];
                    Vt[i][m] = Vt[k][m];
                    Vt[k][m] = t;
                }
            }
    }
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = Vt[3][m];
}

struct TriPoint {
    float x[3], normal[3], min_dist, max_dist;
};

/* positive and finite */
__device__ __forceinline__ bool pos_finite(float v) { return v > 0 && finite_f(v); }

/* One match of LocalMapping::CreateNewMapPoints (LocalMapping.cc:288-444) of a pair with finite poses that passed
 * the baseline test: returns the ORBM_TRI_* outcome, r filled iff a point was created. T1 / T2 = rows 0..2 of the
 * keyframes' mTcw, Ow1 / Ow2 their mOw (frustum_pose), sf / sigma2 = mvScaleFactors / mvLevelSigma2 (16 entries each);
 * the kernel keeps all six in LDS, so these uniform values do not sit in scalar registers across the Jacobi sweeps. */
__device__ __forceinline__ int triangulate_match(const orbm_tri_geom& g, const float* sf, const float* sigma2,
                                                 const float* T1, const float* Ow1, const float* T2, const float* Ow2,
                                                 float u1, float v1, int o1, float ur1, float d1, float u2, float v2,
                                                 int o2, float ur2, float d2, TriPoint& r) {
    if ((unsigned)o1 >= (unsigned)g.nlevels || (unsigned)o2 >= (unsigned)g.nlevels || !finite_f(u1) || !finite_f(v1) ||
        !finite_f(u2) || !finite_f(v2) || !finite_f(ur1) || !finite_f(ur2))
        return ORBM_TRI_EXCLUDED;
    const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
    if ((st1 || st2) && !pos_finite(g.b)) return ORBM_TRI_EXCLUDED;
    if ((st1 && !pos_finite(d1)) || (st2 && !pos_finite(d2))) return ORBM_TRI_EXCLUDED;
    const float invfx = __fdiv_rn(1.0f, g.fx), invfy = __fdiv_rn(1.0f, g.fy);
    const float xn1x = __fmul_rn(__fsub_rn(u1, g.cx), invfx), xn1y = __fmul_rn(__fsub_rn(v1, g.cy), invfy);
    const float xn2x = __fmul_rn(__fsub_rn(u2, g.cx), invfx), xn2y = __fmul_rn(__fsub_rn(v2, g.cy), invfy);
    float ray1[3], ray2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {  // row i of Rwc = column i of Rcw
        ray1[i] = __fadd_rn(__fadd_rn(__fmul_rn(T1[i], xn1x), __fmul_rn(T1[4 + i], xn1y)), __fmul_rn(T1[8 + i], 1.0f));
        ray2[i] = __fadd_rn(__fadd_rn(__fmul_rn(T2[i], xn2x), __fmul_rn(T2[4 + i], xn2y)), __fmul_rn(T2[8 + i], 1.0f));
    }
    const double nn1 = __dsqrt_rn(dot3_d(ray1[0], ray1[1], ray1[2], ray1[0], ray1[1], ray1[2]));
    const double nn2 = __dsqrt_rn(dot3_d(ray2[0], ray2[1], ray2[2], ray2[0], ray2[1], ray2[2]));
    const float cosRays = __double2float_rn(
        __ddiv_rn(dot3_d(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]), __dmul_rn(nn1, nn2)));
    if (!finite_f(cosRays)) return ORBM_TRI_EXCLUDED;
    float cs1 = __fadd_rn(cosRays, 1.0f), cs2 = cs1;
    if (st1 || st2) {  // :311-314: KF2's term only when KF1 is monocular
        float sn, cs;
        glibc_sincosf(__fmul_rn(2.0f, glibc_atan2f(__fmul_rn(g.b, 0.5f), st1 ? d1 : d2)), &sn, &cs);
        if (st1)
            cs1 = cs;
        else
            cs2 = cs;
    }
    const float csmin = cs2 < cs1 ? cs2 : cs1;
    int made;
    if (cosRays < csmin && cosRays > 0.0f && (st1 || st2 || (double)cosRays < 0.9998)) {
        float At[4][4], x4[4];  // At[k] = column k of A (:322-326)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            At[k][0] = __fsub_rn(__fmul_rn(xn1x, T1[8 + k]), T1[k]);
            At[k][1] = __fsub_rn(__fmul_rn(xn1y, T1[8 + k]), T1[4 + k]);
            At[k][2] = __fsub_rn(__fmul_rn(xn2x, T2[8 + k]), T2[k]);
            At[k][3] = __fsub_rn(__fmul_rn(xn2y, T2[8 + k]), T2[4 + k]);
        }
        svd4_null(At, x4);
        if (!finite_f(x4[0]) || !finite_f(x4[1]) || !finite_f(x4[2]) || !finite_f(x4[3])) return ORBM_TRI_EXCLUDED;
        if (x4[3] == 0.0f) return ORBM_TRI_W_ZERO;
        const float sc = __double2float_rn(__ddiv_rn(1.0, (double)x4[3]));
#pragma unroll
        for (int k = 0; k < 3; k++) r.x[k] = __fmul_rn(x4[k], sc);
        made = ORBM_TRI_TRIANGULATED;
    } else if (st1 && cs1 < cs2) {
        unproject_point(g.cx, g.cy, invfx, invfy, T1, Ow1, u1, v1, d1, r.x);
        made = ORBM_TRI_STEREO1;
    } else if (st2 && cs2 < cs1) {
        unproject_point(g.cx, g.cy, invfx, invfy, T2, Ow2, u2, v2, d2, r.x);
        made = ORBM_TRI_STEREO2;
    } else {
        return ORBM_TRI_LOW_PARALLAX;
    }
    const float X = r.x[0], Y = r.x[1], Z = r.x[2];
    if (!finite_f(X) || !finite_f(Y) || !finite_f(Z)) return ORBM_TRI_EXCLUDED;
    float c1[3], c2[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        c1[q] = __double2float_rn(__dadd_rn(dot3_d(T1[4 * q], T1[4 * q + 1], T1[4 * q + 2], X, Y, Z), (double)T1[4 * q + 3]));
        c2[q] = __double2float_rn(__dadd_rn(dot3_d(T2[4 * q], T2[4 * q + 1], T2[4 * q + 2], X, Y, Z), (double)T2[4 * q + 3]));
    }
    if (!finite_f(c1[0]) || !finite_f(c1[1]) || !finite_f(c1[2]) || !finite_f(c2[0]) || !finite_f(c2[1]) ||
        !finite_f(c2[2]))
        return ORBM_TRI_EXCLUDED;
    if (c1[2] <= 0) return ORBM_TRI_Z1;
    if (c2[2] <= 0) return ORBM_TRI_Z2;
#pragma unroll
    for (int w = 0; w < 2; w++) {
        const float* c = w ? c2 : c1;
        const float u = w ? u2 : u1, v = w ? v2 : v1, ur = w ? ur2 : ur1;
        const float s2 = sigma2[w ? o2 : o1];
        const float invz = __double2float_rn(__ddiv_rn(1.0, (double)c[2]));
        const float pu = __fadd_rn(__fmul_rn(__fmul_rn(g.fx, c[0]), invz), g.cx);
        const float pv = __fadd_rn(__fmul_rn(__fmul_rn(g.fy, c[1]), invz), g.cy);
        const float ex = __fsub_rn(pu, u), ey = __fsub_rn(pv, v);
        float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
        double th = 5.991;
        if (w ? st2 : st1) {
            const float er = __fsub_rn(__fsub_rn(pu, __fmul_rn(g.bf, invz)), ur);  // KF1's mbf for both (:380, :406)
            e2 = __fadd_rn(e2, __fmul_rn(er, er));
            th = 7.8;
        }
        if (!finite_f(e2)) return ORBM_TRI_EXCLUDED;
        if ((double)e2 > __dmul_rn(th, (double)s2)) return w ? ORBM_TRI_REPROJ2 : ORBM_TRI_REPROJ1;
    }
    const float a0 = __fsub_rn(X, Ow1[0]), a1 = __fsub_rn(Y, Ow1[1]), a2 = __fsub_rn(Z, Ow1[2]);
    const float b0 = __fsub_rn(X, Ow2[0]), b1 = __fsub_rn(Y, Ow2[1]), b2 = __fsub_rn(Z, Ow2[2]);
    const double nd1 = __dsqrt_rn(dot3_d(a0, a1, a2, a0, a1, a2)), nd2 = __dsqrt_rn(dot3_d(b0, b1, b2, b0, b1, b2));
    const float dist1 = __double2float_rn(nd1), dist2 = __double2float_rn(nd2);
    if (!finite_f(dist1) || !finite_f(dist2)) return ORBM_TRI_EXCLUDED;
    if (dist1 == 0 || dist2 == 0) return ORBM_TRI_DIST_ZERO;
    const float ratioDist = __fdiv_rn(dist2, dist1);
    const float ratioOctave = __fdiv_rn(sf[o1], sf[o2]);
    const float ratioFactor = __fmul_rn(1.5f, sf[1]);
    if (!finite_f(ratioDist)) return ORBM_TRI_EXCLUDED;
    if (__fmul_rn(ratioDist, ratioFactor) < ratioOctave || ratioDist > __fmul_rn(ratioOctave, ratioFactor))
        return ORBM_TRI_SCALE_RATIO;
    const float s1 = __double2float_rn(__ddiv_rn(1.0, nd1)), s2 = __double2float_rn(__ddiv_rn(1.0, nd2));
    r.normal[0] = __fmul_rn(__fadd_rn(__fadd_rn(0.0f, __fmul_rn(a0, s1)), __fmul_rn(b0, s2)), 0.5f);
    r.normal[1] = __fmul_rn(__fadd_rn(__fadd_rn(0.0f, __fmul_rn(a1, s1)), __fmul_rn(b1, s2)), 0.5f);
    r.normal[2] = __fmul_rn(__fadd_rn(__fadd_rn(0.0f, __fmul_rn(a2, s1)), __fmul_rn(b2, s2)), 0.5f);
    r.max_dist = __fmul_rn(dist1, sf[o1]);
    r.min_dist = __fdiv_rn(r.max_dist, sf[g.nlevels - 1]);
    return made;
}

/* Optimizer::PoseOptimization's double arithmetic (so3_sincos, the SE3 helpers, ldlt6_solve, pose_edge_eval and
 * Levenberg's bookkeeping): pose_math.h, one statement shared with the host unit pose_optimize.c, here with the
 * rounding intrinsics. */
#define PM_DEVICE 1
#define PM_FN __device__ __forceinline__
#include "pose_math.h"
#undef PM_DEVICE
#undef PM_FN
#undef PM_UNROLL
#undef pmM
#undef pmA
#undef pmS
#undef pmD
#undef pmQ

}  // namespace orbamd

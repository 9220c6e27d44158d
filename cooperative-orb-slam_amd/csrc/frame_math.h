/*
 * frame_math.h -- cv::Mat's float arithmetic on the device as pinned in DESIGN.md "Pinned semantics", every operation
 * stated with a rounding intrinsic so that nothing contracts, and Frame::isInFrustum (Frame.cc:274-330) of one
 * MapPoint built from it: the one definition behind k_frustum and k_local_frustum (local_kernels.hip). The same
 * sequence on the host: frustum.c; in Python: tests/frustum_py.py.
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

}  // namespace orbamd

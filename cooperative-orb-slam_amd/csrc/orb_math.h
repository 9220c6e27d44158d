/*
 * orb_math.h -- bit-exact scalar math shared by the gfx950 kernels.
 *
 * Every float operation the reference performs on the hot path is reproduced with
 * explicitly rounded intrinsics (no FMA contraction; the library is also built with
 * -ffp-contract=off), so device results equal the host oracle bit for bit.
 *
 *  - glibc_cosf/glibc_sinf: the float cos/sin that computeOrbDescriptor calls
 *    (ORBextractor.cc:113, `cos(angle)` on a float = glibc cosf). Restated from glibc 2.35's
 *    sincosf algorithm (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c): double evaluation,
 *    constants read from libm's __sincosf_table. Verified equal to the host libm (both the
 *    FMA and the SSE2 ifunc variants) for every float in [0, 2*pi] (tools/check_trig.c).
 *  - glibc_logf: the float log of MapPoint::PredictScale (MapPoint.cc:385-417, inside Frame::isInFrustum). Restated
 *    from glibc 2.35's logf (sysdeps/ieee754/flt-32/e_logf.c), constants read from libm's __logf_data. Verified
 *    equal to the host libm for every positive normal float (tools/check_logf.c).
 *  - glibc_atan2f: the float atan2 of cosParallaxStereo in LocalMapping::CreateNewMapPoints (LocalMapping.cc:312), first
 *    quadrant only. Restated from glibc 2.35's atanf / atan2f (s_atanf.c, e_atan2f.c, the fdlibm float forms), all in
 *    float. Verified equal to the host libm on every third positive finite float and on 8.4e6 first-quadrant pairs
 *    (tools/check_atan2f.c).
 *  - fast_atan2: cv::fastAtan2 (OpenCV 3.x scalar form), called by IC_Angle
 *    (ORBextractor.cc:103).
 *  - so3_sincos, the double sin / cos of SE3Quat::exp in Optimizer::PoseOptimization, is not here but in pose_math.h:
 *    it is the project's own routine, not a restatement of libm's, and is shared with the plain-C host unit.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbamd {

__device__ __forceinline__ int cv_round(float v) { return __float2int_rn(v); }

__device__ __forceinline__ float fast_atan2(float y, float x) {
    const float r2d = (float)(180 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * r2d, p3 = -0.3258083974640975f * r2d,
                p5 = 0.1555786518463281f * r2d, p7 = -0.04432655554792128f * r2d;
    const float eps = (float)2.220446049250313080847e-16; /* (float)DBL_EPSILON */
    float ax = fabsf(x), ay = fabsf(y), a, c, c2, poly;
    if (ax >= ay) {
        c = __fdiv_rn(ay, __fadd_rn(ax, eps));
    } else {
        c = __fdiv_rn(ax, __fadd_rn(ay, eps));
    }
    c2 = __fmul_rn(c, c);
    poly = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    a = (ax >= ay) ? poly : __fsub_rn(90.f, poly);
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

/* glibc 2.35 __sincosf_table (values read from libm.so.6 .rodata). Table 1 is table 0 with the
 * cosine coefficients negated and identical sine coefficients, and sign[n&3] = -1 for n&3 in
 * {1,2}; all constants are immediates (no memory loads on the hot path). */
#define SC_HPI_INV 0x1.45f306dc9c883p+23
#define SC_HPI 0x1.921fb54442d18p+0
#define SC_C0 1.0
#define SC_C1 -0x1.ffffffd0c621cp-2
#define SC_S1 -0x1.555545995a603p-3
#define SC_C2 0x1.55553e1068f19p-5
#define SC_S2 0x1.1107605230bc4p-7
#define SC_C3 -0x1.6c087e89a359dp-10
#define SC_S3 -0x1.994eb3774cf24p-13
#define SC_C4 0x1.99343027bf8c3p-16

__device__ __forceinline__ float sinf_poly(double xs, double x2) {
    double x3 = __dmul_rn(x2, xs);
    double a = __fma_rn(x2, SC_S3, SC_S2);
    double x5 = __dmul_rn(x3, x2);
    double s = __fma_rn(x3, SC_S1, xs);
    return __double2float_rn(__fma_rn(a, x5, s));
}
/* neg = 1 selects table 1 (cosine coefficients negated) */
__device__ __forceinline__ float cosf_poly(double x2, bool neg) {
    const double c0 = neg ? -SC_C0 : SC_C0, c1 = neg ? -SC_C1 : SC_C1, c2 = neg ? -SC_C2 : SC_C2;
    const double c3 = neg ? -SC_C3 : SC_C3, c4 = neg ? -SC_C4 : SC_C4;
    double x4 = __dmul_rn(x2, x2);
    double t1 = __fma_rn(x2, c1, c0);
    double t2 = __fma_rn(x2, c4, c3);
    double x6 = __dmul_rn(x2, x4);
    double c = __fma_rn(x4, c2, t1);
    return __double2float_rn(__fma_rn(t2, x6, c));
}
__device__ __forceinline__ unsigned top12(float y) { return (__float_as_uint(y) >> 20) & 0x7ff; }
/* valid for |y| < 120 (all ORB angles are in [0, 2*pi]) */
__device__ __forceinline__ void glibc_sincosf(float y, float* s_out, float* c_out) {
    double x = (double)y;
    if (top12(y) <= 0x3f3) {
        double x2 = __dmul_rn(x, x);
        if (top12(y) <= 0x397) {
            *s_out = y;
            *c_out = 1.0f;
            return;
        }
        *s_out = sinf_poly(x, x2);
        *c_out = cosf_poly(x2, false);
        return;
    }
    double r = __dmul_rn(x, SC_HPI_INV);
    int n = ((int)r + 0x800000) >> 24;
    double xr = __fma_rn(-(double)n, SC_HPI, x);
    const bool neg = (n & 2) != 0;
    double x2 = __dmul_rn(xr, xr);
    const int q = n & 3;
    double xs = (q == 1 || q == 2) ? -xr : xr;  // xr * sign[n&3], exact
    if (n & 1) {
        *s_out = cosf_poly(x2, neg);
        *c_out = sinf_poly(xs, x2);
    } else {
        *s_out = sinf_poly(xs, x2);
        *c_out = cosf_poly(x2, neg);
    }
}

/* glibc 2.35 logf (sysdeps/ieee754/flt-32/e_logf.c), the log of MapPoint::PredictScale (MapPoint.cc:385-417, `log`
 * of a float = logf): __logf_data's {invc, logc} table, ln2 and polynomial read from libm's .rodata; double
 * evaluation without contraction, one rounding. Equal to the host libm (FMA and plain ifunc variants) for every
 * positive normal float (tools/check_logf.c, which states the same sequence in C). */
static __constant__ double kLogfTab[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
    {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2},  {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
    {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
    {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4},
    {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3},
    {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2}};
#define LOGF_LN2 0x1.62e42fefa39efp-1
#define LOGF_A0 -0x1.00ea348b88334p-2
#define LOGF_A1 0x1.5575b0be00b6ap-2
#define LOGF_A2 -0x1.ffffef20a4123p-2

/* a positive normal float (0x00800000 <= bits < 0x7f800000); anything else is the caller's to exclude */
__device__ __forceinline__ bool logf_domain(float x) {
    return __float_as_uint(x) - 0x00800000u < 0x7f800000u - 0x00800000u;
}
__device__ __forceinline__ float glibc_logf(float x) {
    const uint32_t ix = __float_as_uint(x);
    if (ix == 0x3f800000u) return 0.0f;
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (tmp >> 19) & 15;
    const int k = (int32_t)tmp >> 23;
    const double z = (double)__uint_as_float(ix - (tmp & 0xff800000u));
    const double invc = kLogfTab[i][0], logc = kLogfTab[i][1];
    const double r = __dadd_rn(__dmul_rn(z, invc), -1.0);
    const double y0 = __dadd_rn(logc, __dmul_rn((double)k, LOGF_LN2));
    const double r2 = __dmul_rn(r, r);
    double y = __dadd_rn(__dmul_rn(LOGF_A1, r), LOGF_A2);
    y = __dadd_rn(__dmul_rn(LOGF_A0, r2), y);
    y = __dadd_rn(__dmul_rn(y, r2), __dadd_rn(y0, r));
    return __double2float_rn(y);
}

/* glibc 2.35 atanf (sysdeps/ieee754/flt-32/s_atanf.c, the fdlibm float form) for x >= 0: break points 0.4375, 0.6875,
 * 1.1875, 2.4375, the atanhi / atanlo tables and the 11-term aT polynomial split into odd and even parts, every
 * operation in float without contraction. x below 2^-29 returns x; x at or above 2^25 returns atanhi[3] + atanlo[3].
 * tools/check_atan2f.c states the same sequence in C and compares it with the host libm. */
__device__ __forceinline__ float glibc_atanf_pos(float x) {
    const uint32_t ix = __float_as_uint(x);
    const float hi3 = __uint_as_float(0x3fc90fdau), lo3 = __uint_as_float(0x33a22168u);
    if (ix >= 0x4c000000u) return __fadd_rn(hi3, lo3);
    int id = -1;
    if (ix < 0x3ee00000u) {
        if (ix < 0x31000000u) return x;
    } else if (ix < 0x3f980000u) {
        if (ix < 0x3f300000u) {
            id = 0;
            x = __fdiv_rn(__fsub_rn(__fmul_rn(2.0f, x), 1.0f), __fadd_rn(2.0f, x));
        } else {
            id = 1;
            x = __fdiv_rn(__fsub_rn(x, 1.0f), __fadd_rn(x, 1.0f));
        }
    } else if (ix < 0x401c0000u) {
        id = 2;
        x = __fdiv_rn(__fsub_rn(x, 1.5f), __fadd_rn(1.0f, __fmul_rn(1.5f, x)));
    } else {
        id = 3;
        x = __fdiv_rn(-1.0f, x);
    }
    const float aT0 = __uint_as_float(0x3eaaaaabu), aT1 = __uint_as_float(0xbe4ccccdu),
                aT2 = __uint_as_float(0x3e124925u), aT3 = __uint_as_float(0xbde38e38u),
                aT4 = __uint_as_float(0x3dba2e6eu), aT5 = __uint_as_float(0xbd9d8795u),
                aT6 = __uint_as_float(0x3d886b35u), aT7 = __uint_as_float(0xbd6ef16bu),
                aT8 = __uint_as_float(0x3d4bda59u), aT9 = __uint_as_float(0xbd15a221u),
                aT10 = __uint_as_float(0x3c8569d7u);
    const float z = __fmul_rn(x, x), w = __fmul_rn(z, z);
    float s1 = __fadd_rn(aT8, __fmul_rn(w, aT10));
    s1 = __fadd_rn(aT6, __fmul_rn(w, s1));
    s1 = __fadd_rn(aT4, __fmul_rn(w, s1));
    s1 = __fadd_rn(aT2, __fmul_rn(w, s1));
    s1 = __fmul_rn(z, __fadd_rn(aT0, __fmul_rn(w, s1)));
    float s2 = __fadd_rn(aT7, __fmul_rn(w, aT9));
    s2 = __fadd_rn(aT5, __fmul_rn(w, s2));
    s2 = __fadd_rn(aT3, __fmul_rn(w, s2));
    s2 = __fmul_rn(w, __fadd_rn(aT1, __fmul_rn(w, s2)));
    const float xs = __fmul_rn(x, __fadd_rn(s1, s2));
    if (id < 0) return __fsub_rn(x, xs);
    const float hi = id == 0 ? __uint_as_float(0x3eed6338u) : id == 1 ? __uint_as_float(0x3f490fdau)
                   : id == 2 ? __uint_as_float(0x3f7b985eu) : hi3;
    const float lo = id == 0 ? __uint_as_float(0x31ac3769u) : id == 1 ? __uint_as_float(0x33222168u)
                   : id == 2 ? __uint_as_float(0x33140fb4u) : lo3;
    return __fsub_rn(hi, __fsub_rn(__fsub_rn(xs, lo), x));
}

/* y > 0 and x > 0, both finite: the first quadrant, all that cos(2 * atan2(mb / 2, depth)) of CreateNewMapPoints
 * (LocalMapping.cc:312, :314) needs; anything else is the caller's to exclude */
__device__ __forceinline__ bool atan2f_domain(float y, float x) {
    return __float_as_uint(y) - 1u < 0x7f800000u - 1u && __float_as_uint(x) - 1u < 0x7f800000u - 1u;
}
/* glibc 2.35 atan2f (e_atan2f.c) in the first quadrant: atanf(y) for x == 1, pi/2 for an exponent gap above 60
 * (pi_o_2 + 0.5f * pi_lo rounds to pi_o_2), otherwise atanf(fabsf(y / x)) */
__device__ __forceinline__ float glibc_atan2f(float y, float x) {
    const int32_t hx = (int32_t)__float_as_uint(x), hy = (int32_t)__float_as_uint(y);
    if (hx == 0x3f800000) return glibc_atanf_pos(y);
    const int k = (hy - hx) >> 23;
    if (k > 60) return __fadd_rn(__uint_as_float(0x3fc90fdbu), __fmul_rn(0.5f, __uint_as_float(0xb3bbbd2eu)));
    return glibc_atanf_pos(fabsf(__fdiv_rn(y, x)));
}

}  // namespace orbamd

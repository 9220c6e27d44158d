/*
 * pose_math.h -- the double arithmetic of Optimizer::PoseOptimization (Optimizer.cc:239-451) with the parts of g2o it
 * runs (SE3Quat, the two OnlyPose edges, Huber, Levenberg, a dense 6x6 LDL^T), stated once for the host unit
 * (pose_optimize.c, plain C) and the device (frame_math.h includes it inside namespace orbamd; k_pose_optimize,
 * pose_kernels.hip). include/orbslam_amd.h ("Pose optimisation") states the sequence; tests/pose_py.py restates it in
 * Python, the yardstick.
 *
 * Every operation goes through one of five macros, so nothing can contract whatever the flags: on the device they are
 * the correctly rounded intrinsics (__dmul_rn, __dadd_rn, __dsub_rn, __ddiv_rn, __dsqrt_rn), on the host the plain
 * C operators of a unit built with -ffp-contract=off. The including file defines PM_FN (the function qualifier) and,
 * on the device, PM_DEVICE.
 *
 * so3_sincos is the project's own double sin / cos (glibc's rest on a table libm does not export): Cody-Waite
 * reduction by pi/2 to |r| <= pi/4, Taylor polynomials in Horner form, no libm call, no table, no FMA. The constants
 * are derived by tools/gen_so3_sincos.py; tools/check_so3_sincos.c measures the distance from libm.
 */
#ifndef ORBAMD_POSE_MATH_H
#define ORBAMD_POSE_MATH_H

#ifdef PM_DEVICE
#define pmM(a, b) __dmul_rn((a), (b))
#define pmA(a, b) __dadd_rn((a), (b))
#define pmS(a, b) __dsub_rn((a), (b))
#define pmD(a, b) __ddiv_rn((a), (b))
#define pmQ(a) __dsqrt_rn(a)
#define PM_UNROLL _Pragma("unroll")
#else
#define pmM(a, b) ((a) * (b))
#define pmA(a, b) ((a) + (b))
#define pmS(a, b) ((a) - (b))
#define pmD(a, b) ((a) / (b))
#define pmQ(a) sqrt(a)
#define PM_UNROLL
#endif

#define SO3_PIO2_1 0x1.921fb54400000p+0
#define SO3_PIO2_2 0x1.0b4611a600000p-34
#define SO3_PIO2_3 0x1.3198a2e037073p-69
#define SO3_INV_PIO2 0x1.45f306dc9c883p-1
#define SO3_S1 -0x1.5555555555555p-3
#define SO3_C1 -0x1.0000000000000p-1
#define SO3_S2 0x1.1111111111111p-7
#define SO3_C2 0x1.5555555555555p-5
#define SO3_S3 -0x1.a01a01a01a01ap-13
#define SO3_C3 -0x1.6c16c16c16c17p-10
#define SO3_S4 0x1.71de3a556c734p-19
#define SO3_C4 0x1.a01a01a01a01ap-16
#define SO3_S5 -0x1.ae64567f544e4p-26
#define SO3_C5 -0x1.27e4fb7789f5cp-22
#define SO3_S6 0x1.6124613a86d09p-33
#define SO3_C6 0x1.1eed8eff8d898p-29
#define SO3_S7 -0x1.ae7f3e733b81fp-41
#define SO3_C7 -0x1.93974a8c07c9dp-37
#define SO3_S8 0x1.952c77030ad4ap-49
#define SO3_C8 0x1.ae7f3e733b81fp-45

#define PM_DBL_MAX 0x1.fffffffffffffp+1023
#define PM_NTERMS 28 /* 21 upper-triangle H terms (row-major), 6 b terms, rho0 */

/* finite: the exponent field is not all ones */
PM_FN int pm_finite(double v) {
    union {
        double d;
        unsigned long long u;
    } c;
    c.d = v;
    return (c.u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

/* sin and cos of th >= 0. k = (int)(th * (2/pi) + 0.5); r = ((th - k * PIO2_1) - k * PIO2_2) - k * PIO2_3 (pi/2 in
 * three parts, the first two of 33 bits, so both products are exact); z = r * r;
 * sin r = r + r * (z * (S1 + z * (S2 + ... z * S8))); cos r = 1 + z * (C1 + z * (C2 + ... z * C8)); the quadrant
 * k & 3 picks (s, c), (c, -s), (-s, -c), (-c, s). Anything not below 2^20 (NaN included) gives (0, 1). */
PM_FN void so3_sincos(double th, double* s_out, double* c_out) {
    if (!(th < 1048576.0)) {
        *s_out = 0.0;
        *c_out = 1.0;
        return;
    }
    const int k = (int)pmA(pmM(th, SO3_INV_PIO2), 0.5);
    const double kd = (double)k;
    const double r = pmS(pmS(pmS(th, pmM(kd, SO3_PIO2_1)), pmM(kd, SO3_PIO2_2)), pmM(kd, SO3_PIO2_3));
    const double z = pmM(r, r);
    double ps = pmM(z, SO3_S8);
    ps = pmM(z, pmA(SO3_S7, ps));
    ps = pmM(z, pmA(SO3_S6, ps));
    ps = pmM(z, pmA(SO3_S5, ps));
    ps = pmM(z, pmA(SO3_S4, ps));
    ps = pmM(z, pmA(SO3_S3, ps));
    ps = pmM(z, pmA(SO3_S2, ps));
    ps = pmM(z, pmA(SO3_S1, ps));
    const double sn = pmA(r, pmM(r, ps));
    double pc = pmM(z, SO3_C8);
    pc = pmM(z, pmA(SO3_C7, pc));
    pc = pmM(z, pmA(SO3_C6, pc));
    pc = pmM(z, pmA(SO3_C5, pc));
    pc = pmM(z, pmA(SO3_C4, pc));
    pc = pmM(z, pmA(SO3_C3, pc));
    pc = pmM(z, pmA(SO3_C2, pc));
    pc = pmM(z, pmA(SO3_C1, pc));
    const double cs = pmA(1.0, pc);
    const int q = k & 3;
    *s_out = q == 0 ? sn : q == 1 ? cs : q == 2 ? -sn : -cs;
    *c_out = q == 0 ? cs : q == 1 ? -sn : q == 2 ? -cs : sn;
}

/* q /= sqrt(x^2 + y^2 + z^2 + w^2) (summed in that order); w < 0 negates all four (SE3Quat::normalizeRotation) */
PM_FN void pm_quat_normalize(double* q) {
    const double n =
        pmQ(pmA(pmA(pmA(pmM(q[0], q[0]), pmM(q[1], q[1])), pmM(q[2], q[2])), pmM(q[3], q[3])));
    q[0] = pmD(q[0], n);
    q[1] = pmD(q[1], n);
    q[2] = pmD(q[2], n);
    q[3] = pmD(q[3], n);
    if (q[3] < 0.0) {
        q[0] = -q[0];
        q[1] = -q[1];
        q[2] = -q[2];
        q[3] = -q[3];
    }
}

/* one trace <= 0 branch of Eigen's matrix -> quaternion: the largest diagonal entry is Rii, (i, j, k) cyclic */
PM_FN void pm_quat_branch(double Rii, double Rjj, double Rkk, double Rkj, double Rjk, double Rji, double Rij,
                          double Rki, double Rik, double* qi, double* qj, double* qk, double* w) {
    double s = pmQ(pmA(pmS(pmS(Rii, Rjj), Rkk), 1.0));
    *qi = pmM(0.5, s);
    s = pmD(0.5, s);
    *w = pmM(pmS(Rkj, Rjk), s);
    *qj = pmM(pmA(Rji, Rij), s);
    *qk = pmM(pmA(Rki, Rik), s);
}

/* Eigen's Quaterniond(Matrix3d), then normalizeRotation; R row-major, q = (x, y, z, w) */
PM_FN void pm_quat_from_R(const double* R, double* q) {
    const double tr = pmA(pmA(R[0], R[4]), R[8]);
    if (tr > 0.0) {
        double s = pmQ(pmA(tr, 1.0));
        q[3] = pmM(0.5, s);
        s = pmD(0.5, s);
        q[0] = pmM(pmS(R[7], R[5]), s);
        q[1] = pmM(pmS(R[2], R[6]), s);
        q[2] = pmM(pmS(R[3], R[1]), s);
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i == 1 ? R[4] : R[0])) i = 2;
        if (i == 0)
            pm_quat_branch(R[0], R[4], R[8], R[7], R[5], R[3], R[1], R[6], R[2], &q[0], &q[1], &q[2], &q[3]);
        else if (i == 1)
            pm_quat_branch(R[4], R[8], R[0], R[2], R[6], R[7], R[5], R[1], R[3], &q[1], &q[2], &q[0], &q[3]);
        else
            pm_quat_branch(R[8], R[0], R[4], R[3], R[1], R[2], R[6], R[5], R[7], &q[2], &q[0], &q[1], &q[3]);
    }
    pm_quat_normalize(q);
}

/* Converter::toSE3Quat: s = (qx, qy, qz, qw, tx, ty, tz) from the float mTcw (row-major 4x4) */
PM_FN void se3_from_Tcw(const float* T, double* s) {
    double R[9];
    PM_UNROLL
    for (int r = 0; r < 3; r++) {
        R[3 * r] = (double)T[4 * r];
        R[3 * r + 1] = (double)T[4 * r + 1];
        R[3 * r + 2] = (double)T[4 * r + 2];
        s[4 + r] = (double)T[4 * r + 3];
    }
    pm_quat_from_R(R, s);
}

/* q (x) X of Eigen: uv = qv x X; uv = uv + uv; X + w uv + qv x uv */
PM_FN void pm_quat_rot(const double* q, double X0, double X1, double X2, double* o) {
    double u0 = pmS(pmM(q[1], X2), pmM(q[2], X1));
    double u1 = pmS(pmM(q[2], X0), pmM(q[0], X2));
    double u2 = pmS(pmM(q[0], X1), pmM(q[1], X0));
    u0 = pmA(u0, u0);
    u1 = pmA(u1, u1);
    u2 = pmA(u2, u2);
    o[0] = pmA(pmA(X0, pmM(q[3], u0)), pmS(pmM(q[1], u2), pmM(q[2], u1)));
    o[1] = pmA(pmA(X1, pmM(q[3], u1)), pmS(pmM(q[2], u0), pmM(q[0], u2)));
    o[2] = pmA(pmA(X2, pmM(q[3], u2)), pmS(pmM(q[0], u1), pmM(q[1], u0)));
}

/* SE3Quat::map: q (x) X + t */
PM_FN void se3_map(const double* s, double X0, double X1, double X2, double* o) {
    pm_quat_rot(s, X0, X1, X2, o);
    o[0] = pmA(o[0], s[4]);
    o[1] = pmA(o[1], s[5]);
    o[2] = pmA(o[2], s[6]);
}

/* Converter::toCvMat(SE3Quat): Eigen's toRotationMatrix, cast to float */
PM_FN void se3_to_Tcw(const double* s, float* T) {
    const double x = s[0], y = s[1], z = s[2], w = s[3];
    const double tx = pmM(2.0, x), ty = pmM(2.0, y), tz = pmM(2.0, z);
    const double twx = pmM(tx, w), twy = pmM(ty, w), twz = pmM(tz, w);
    const double txx = pmM(tx, x), txy = pmM(ty, x), txz = pmM(tz, x);
    const double tyy = pmM(ty, y), tyz = pmM(tz, y), tzz = pmM(tz, z);
    T[0] = (float)pmS(1.0, pmA(tyy, tzz));
    T[1] = (float)pmS(txy, twz);
    T[2] = (float)pmA(txz, twy);
    T[3] = (float)s[4];
    T[4] = (float)pmA(txy, twz);
    T[5] = (float)pmS(1.0, pmA(txx, tzz));
    T[6] = (float)pmS(tyz, twx);
    T[7] = (float)s[5];
    T[8] = (float)pmS(txz, twy);
    T[9] = (float)pmA(tyz, twx);
    T[10] = (float)pmS(1.0, pmA(txx, tyy));
    T[11] = (float)s[6];
    T[12] = 0.0f;
    T[13] = 0.0f;
    T[14] = 0.0f;
    T[15] = 1.0f;
}

/* estimate := SE3Quat::exp(d) * estimate (VertexSE3Expmap::oplusImpl), d = (omega, upsilon); returns 1 when the
 * theta < 0.00001 branch of exp was taken */
PM_FN int se3_exp_mul(const double* d, double* s) {
    const double w0 = d[0], w1 = d[1], w2 = d[2];
    const double th = pmQ(pmA(pmA(pmM(w0, w0), pmM(w1, w1)), pmM(w2, w2)));
    double Om[9], O2[9], R[9], V[9];
    Om[0] = 0.0, Om[1] = -w2, Om[2] = w1;
    Om[3] = w2, Om[4] = 0.0, Om[5] = -w0;
    Om[6] = -w1, Om[7] = w0, Om[8] = 0.0;
    PM_UNROLL
    for (int r = 0; r < 3; r++) {
        PM_UNROLL
        for (int c = 0; c < 3; c++)
            O2[3 * r + c] = pmA(pmA(pmM(Om[3 * r], Om[c]), pmM(Om[3 * r + 1], Om[3 + c])), pmM(Om[3 * r + 2], Om[6 + c]));
    }
    int small = 0;
    if (th < 0.00001) {
        small = 1;
        PM_UNROLL
        for (int k = 0; k < 9; k++) {
            R[k] = pmA(pmA((k % 4) == 0 ? 1.0 : 0.0, Om[k]), O2[k]);
            V[k] = R[k];
        }
    } else {
        double sn, cs;
        so3_sincos(th, &sn, &cs);
        const double th2 = pmM(th, th);
        const double a = pmD(sn, th), b = pmD(pmS(1.0, cs), th2), c3 = pmD(pmS(th, sn), pmM(th2, th));
        PM_UNROLL
        for (int k = 0; k < 9; k++) {
            const double id = (k % 4) == 0 ? 1.0 : 0.0;
            R[k] = pmA(pmA(id, pmM(a, Om[k])), pmM(b, O2[k]));
            V[k] = pmA(pmA(id, pmM(b, Om[k])), pmM(c3, O2[k]));
        }
    }
    double qd[4], td[3], rt[3], qn[4];
    pm_quat_from_R(R, qd);
    PM_UNROLL
    for (int r = 0; r < 3; r++)
        td[r] = pmA(pmA(pmM(V[3 * r], d[3]), pmM(V[3 * r + 1], d[4])), pmM(V[3 * r + 2], d[5]));
    pm_quat_rot(qd, s[4], s[5], s[6], rt);
    /* Hamilton product qd (x) q, Eigen's order of terms */
    const double ax = qd[0], ay = qd[1], az = qd[2], aw = qd[3], bx = s[0], by = s[1], bz = s[2], bw = s[3];
    qn[3] = pmS(pmS(pmS(pmM(aw, bw), pmM(ax, bx)), pmM(ay, by)), pmM(az, bz));
    qn[0] = pmS(pmA(pmA(pmM(aw, bx), pmM(ax, bw)), pmM(ay, bz)), pmM(az, by));
    qn[1] = pmS(pmA(pmA(pmM(aw, by), pmM(ay, bw)), pmM(az, bx)), pmM(ax, bz));
    qn[2] = pmS(pmA(pmA(pmM(aw, bz), pmM(az, bw)), pmM(ax, by)), pmM(ay, bx));
    pm_quat_normalize(qn);
    s[0] = qn[0], s[1] = qn[1], s[2] = qn[2], s[3] = qn[3];
    s[4] = pmA(td[0], rt[0]);
    s[5] = pmA(td[1], rt[1]);
    s[6] = pmA(td[2], rt[2]);
    return small;
}

/* A x = b for a symmetric 6x6 A (row-major, the lower triangle is read) by LDL^T without pivoting:
 *   d_j = A_jj - sum_{k<j} (L_jk d_k) L_jk;  not (d_j > 0) fails;  L_ij = (A_ij - sum_{k<j} (L_ik d_k) L_jk) / d_j;
 *   y_i = b_i - sum_{k<i} L_ik y_k;  z_i = y_i / d_i;  x_i = z_i - sum_{k>i} L_ki x_k   (every sum with k ascending).
 * Returns 1, or 0 with x = 0 on a failure. */
PM_FN int ldlt6_solve(const double* A, const double* b, double* x) {
    double L[36], dg[6], y[6];
    int ok = 1;
    PM_UNROLL
    for (int j = 0; j < 6; j++) {
        double dj = A[6 * j + j];
        PM_UNROLL
        for (int k = 0; k < j; k++) dj = pmS(dj, pmM(pmM(L[6 * j + k], dg[k]), L[6 * j + k]));
        if (!(dj > 0.0)) ok = 0;
        dg[j] = dj;
        PM_UNROLL
        for (int i = j + 1; i < 6; i++) {
            double sv = A[6 * i + j];
            PM_UNROLL
            for (int k = 0; k < j; k++) sv = pmS(sv, pmM(pmM(L[6 * i + k], dg[k]), L[6 * j + k]));
            L[6 * i + j] = pmD(sv, dj);
        }
    }
    if (!ok) {
        PM_UNROLL
        for (int i = 0; i < 6; i++) x[i] = 0.0;
        return 0;
    }
    PM_UNROLL
    for (int i = 0; i < 6; i++) {
        double v = b[i];
        PM_UNROLL
        for (int k = 0; k < i; k++) v = pmS(v, pmM(L[6 * i + k], y[k]));
        y[i] = v;
    }
    PM_UNROLL
    for (int i = 5; i >= 0; i--) {
        double v = pmD(y[i], dg[i]);
        PM_UNROLL
        for (int k = i + 1; k < 6; k++) v = pmS(v, pmM(L[6 * k + i], x[k]));
        x[i] = v;
    }
    return 1;
}

/* the camera of the edges, widened once */
typedef struct pm_cam {
    double fx, fy, cx, cy, bf;
} pm_cam;

/* One edge (EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose) at the estimate s: returns chi2 =
 * e . (invSigma2 e). With out != NULL also Huber (delta > 0: the edge still has its kernel; delta = 0: none), and the
 * edge's terms of the quadratic form at out[k * stride]: k < 21 the upper triangle of J^T (rho1 invSigma2) J row by
 * row, 21..26 b = J^T ((-(invSigma2 e)) rho1), 27 rho0; full = 0 writes term 27 only. */
PM_FN double pose_edge_eval(const pm_cam* cam, const double* s, double Xw0, double Xw1, double Xw2, double ox,
                            double oy, double our, int stereo, double inv_sigma2, double delta, int full, double* out,
                            int stride) {
    double P[3];
    se3_map(s, Xw0, Xw1, Xw2, P);
    const double X = P[0], Y = P[1];
    const double invz = pmD(1.0, P[2]);
    const double u = pmA(pmM(pmM(X, invz), cam->fx), cam->cx);
    const double v = pmA(pmM(pmM(Y, invz), cam->fy), cam->cy);
    const double e0 = pmS(ox, u), e1 = pmS(oy, v);
    const double e2 = stereo ? pmS(our, pmS(u, pmM(cam->bf, invz))) : 0.0;
    const double we0 = pmM(inv_sigma2, e0), we1 = pmM(inv_sigma2, e1), we2 = pmM(inv_sigma2, e2);
    double chi2 = pmA(pmM(e0, we0), pmM(e1, we1));
    if (stereo) chi2 = pmA(chi2, pmM(e2, we2));
    if (!out) return chi2;
    double rho0 = chi2, rho1 = 1.0;
    if (delta > 0.0) {
        const double d2 = pmM(delta, delta);
        if (!(chi2 <= d2)) {
            const double sq = pmQ(chi2);
            rho0 = pmS(pmM(pmM(2.0, sq), delta), d2);
            rho1 = pmD(delta, sq);
        }
    }
    out[27 * stride] = rho0;
    if (!full) return chi2;
    const double iz2 = pmM(invz, invz);
    const double XY = pmM(X, Y);
    double J[18];
    J[0] = pmM(pmM(XY, iz2), cam->fx);
    J[1] = pmM(-pmA(1.0, pmM(pmM(X, X), iz2)), cam->fx);
    J[2] = pmM(pmM(Y, invz), cam->fx);
    J[3] = pmM(-invz, cam->fx);
    J[4] = 0.0;
    J[5] = pmM(pmM(X, iz2), cam->fx);
    J[6] = pmM(pmA(1.0, pmM(pmM(Y, Y), iz2)), cam->fy);
    J[7] = pmM(pmM(-XY, iz2), cam->fy);
    J[8] = pmM(pmM(-X, invz), cam->fy);
    J[9] = 0.0;
    J[10] = pmM(-invz, cam->fy);
    J[11] = pmM(pmM(Y, iz2), cam->fy);
    J[12] = pmS(J[0], pmM(pmM(cam->bf, Y), iz2));
    J[13] = pmA(J[1], pmM(pmM(cam->bf, X), iz2));
    J[14] = J[2];
    J[15] = J[3];
    J[16] = 0.0;
    J[17] = pmS(J[5], pmM(cam->bf, iz2));
    const double wgt = pmM(rho1, inv_sigma2);
    const double r0 = pmM(-we0, rho1), r1 = pmM(-we1, rho1), r2 = pmM(-we2, rho1);
    int t = 0;
    PM_UNROLL
    for (int a = 0; a < 6; a++) {
        PM_UNROLL
        for (int b = a; b < 6; b++) {
            double h = pmA(pmM(J[a], pmM(wgt, J[b])), pmM(J[6 + a], pmM(wgt, J[6 + b])));
            if (stereo) h = pmA(h, pmM(J[12 + a], pmM(wgt, J[12 + b])));
            out[t * stride] = h;
            t++;
        }
    }
    PM_UNROLL
    for (int a = 0; a < 6; a++) {
        double g = pmA(pmM(J[a], r0), pmM(J[6 + a], r1));
        if (stereo) g = pmA(g, pmM(J[12 + a], r2));
        out[(21 + a) * stride] = g;
    }
    return chi2;
}

/* Optimizer.cc:393-395 / :422-424: `const float chi2 = e->chi2(); if(chi2>chi2Mono[it])` -- the double chi2 cast to
 * float against the float constant, strictly: a chi2 whose float is the threshold itself is an inlier */
PM_FN int pose_edge_outlier(double chi2, int stereo) {
    const float th_mono = (float)5.991, th_stereo = (float)7.815;
    return (float)chi2 > (stereo ? th_stereo : th_mono);
}

/* Levenberg's bookkeeping of one optimize(10) (g2o's OptimizationAlgorithmLevenberg::solve), uniform per frame */
typedef struct pm_lm {
    double lambda, nu, cur, rho;
    int q, ok, rejected, fails, small;
} pm_lm;

/* after the full evaluation of iteration `iter` (sum = the 28 accumulated terms): cur, and at iter 0 lambda and nu */
PM_FN void pm_lm_iter_begin(pm_lm* lm, const double* sum, int iter) {
    lm->cur = sum[27];
    if (iter == 0) {
        double md = 0.0;
        const int dgi[6] = {0, 6, 11, 15, 18, 20};
        PM_UNROLL
        for (int a = 0; a < 6; a++) {
            const double v = fabs(sum[dgi[a]]);
            if (v > md) md = v;
        }
        lm->lambda = pmM(1e-5, md);
        lm->nu = 2.0;
    }
    lm->rho = 0.0;
    lm->q = 0;
}

/* one trial: solve (H + lambda I) x = b, save the estimate, apply exp(x) */
PM_FN void pm_lm_trial_step(pm_lm* lm, const double* sum, double* x, double* est, double* saved) {
    double A[36], b[6];
    int t = 0;
    PM_UNROLL
    for (int a = 0; a < 6; a++) {
        PM_UNROLL
        for (int c = a; c < 6; c++) {
            const double h = a == c ? pmA(sum[t], lm->lambda) : sum[t];
            A[6 * a + c] = h;
            A[6 * c + a] = h;
            t++;
        }
    }
    PM_UNROLL
    for (int a = 0; a < 6; a++) b[a] = sum[21 + a];
    lm->ok = ldlt6_solve(A, b, x);
    if (!lm->ok) lm->fails++;
    PM_UNROLL
    for (int k = 0; k < 7; k++) saved[k] = est[k];
    lm->small += se3_exp_mul(x, est);
}

/* after the error-only evaluation at the trial estimate (tmp = its robust chi2): accept or reject; returns 1 when
 * another trial follows (rho < 0 and fewer than 10 trials) */
PM_FN int pm_lm_trial_end(pm_lm* lm, const double* sum, double tmp, const double* x, double* est,
                          const double* saved) {
    if (!lm->ok) tmp = PM_DBL_MAX;
    double scale = 0.0;
    PM_UNROLL
    for (int a = 0; a < 6; a++) scale = pmA(scale, pmM(x[a], pmA(pmM(lm->lambda, x[a]), sum[21 + a])));
    scale = pmA(scale, 1e-3);
    lm->rho = pmD(pmS(lm->cur, tmp), scale);
    if (lm->rho > 0.0 && pm_finite(tmp)) {
        const double t = pmS(pmM(2.0, lm->rho), 1.0);
        double alpha = pmS(1.0, pmM(pmM(t, t), t));
        const double up = 2.0 / 3.0, lo = 1.0 / 3.0;
        if (up < alpha) alpha = up;
        lm->lambda = pmM(lm->lambda, lo < alpha ? alpha : lo);
        lm->nu = 2.0;
        lm->cur = tmp;
    } else {
        lm->lambda = pmM(lm->lambda, lm->nu);
        lm->nu = pmM(lm->nu, 2.0);
        PM_UNROLL
        for (int k = 0; k < 7; k++) est[k] = saved[k];
        lm->rejected++;
    }
    lm->q++;
    return lm->rho < 0.0 && lm->q < 10;
}

/* the iteration loop of optimize() ends after this iteration (g2o's Terminate) */
PM_FN int pm_lm_terminate(const pm_lm* lm) { return lm->q == 10 || lm->rho == 0.0; }

#endif /* ORBAMD_POSE_MATH_H */

/*
 * frustum.c -- Frame::isInFrustum (Frame.cc:274-330) with MapPoint::PredictScale (MapPoint.cc:385-417) on the host for
 * a table of MapPoints: the mbTrackInView / mTrackProj* / mnTrackScaleLevel / mTrackViewCos fields that
 * Tracking::SearchLocalPoints (Tracking.cc:1143-1193) fills before SearchByProjection(F, vpMapPoints, th). Plain C, no
 * device; built with -ffp-contract=off.
 *
 * The float sequence (include/orbslam_amd.h states it; the same is restated in Python, tests/frustum_py.py, the
 * yardstick, and on the device, frustum_device.h). cv::Mat arithmetic as pinned in DESIGN.md "Pinned semantics":
 *   Pc = mRcw * P + mtcw: the small-matrix gemm, a row's three float products summed in float, then
 *        (float)((double)t + (double)mtcw[i]);
 *   PcZ < 0.0f rejects; invz = 1.0f / PcZ, a float divide;
 *   u = fx * PcX * invz + cx, v = fy * PcY * invz + cy in float, left to right;
 *   u < mnMinX || u > mnMaxX rejects, v likewise;
 *   mOw = -mRcw.t() * mtcw: GEMM_1_T, double accumulation from 0, (float)(-1.0 * s);
 *   PO = P - mOw in float; dist = (float)sqrt(sum of (double)PO[k]^2);
 *   dist < 0.8f * mfMinDistance || dist > 1.2f * mfMaxDistance rejects;
 *   viewCos = (float)(sum of (double)PO[k] * (double)Pn[k] / (double)dist); viewCos < viewingCosLimit rejects;
 *   ratio = mfMaxDistance / dist; nScale = ceilf(logf(ratio) / mfLogScaleFactor), a float divide, clamped to
 *   [0, nlevels - 1]; mTrackProjXR = u - mbf * invz.
 * Where the reference's behaviour is undefined or its result meaningless the point is rejected (a contract, not a
 * measurement): a non-finite pose or point field, a non-finite Pc, u, v, dist or viewCos, PcZ == +-0, dist == 0, a
 * ratio that is not a positive normal float.
 */
#include <math.h>
#include <string.h>

#include "../../include/orbslam_amd.h"

static int finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

static int positive_normal(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u - 0x00800000u < 0x7f800000u - 0x00800000u;
}

int orbx_is_in_frustum(const orbm_track_geom* g, float log_scale_factor, const float Tcw[16], float viewing_cos_limit,
                       int n, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                       uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr, int32_t* level,
                       float* view_cos) {
    if (!g || g->nlevels < 1 || g->nlevels > 16 || !(log_scale_factor > 0) || !isfinite(log_scale_factor) || !Tcw ||
        !isfinite(viewing_cos_limit) || n < 0 ||
        (n && (!pos || !normal || !min_dist || !max_dist || !in_view || !proj_x || !proj_y || !proj_xr || !level ||
               !view_cos)))
        return ORBX_EARG;
    int pose_ok = 1;
    for (int k = 0; k < 12; k++) pose_ok &= isfinite(Tcw[k]) != 0;
    float Ow[3] = {0, 0, 0};
    if (pose_ok)
        for (int i = 0; i < 3; i++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)Tcw[4 * k + i] * (double)Tcw[4 * k + 3];
            Ow[i] = (float)(-1.0 * s);
        }
    for (int j = 0; j < n; j++) {
        in_view[j] = 0;
        proj_x[j] = proj_y[j] = proj_xr[j] = view_cos[j] = 0.0f;
        level[j] = 0;
        const float* P = pos + 3 * (size_t)j;
        const float* Pn = normal + 3 * (size_t)j;
        if (!pose_ok || !finite3(P) || !finite3(Pn) || !isfinite(min_dist[j]) || !isfinite(max_dist[j])) continue;
        float Pc[3];
        for (int i = 0; i < 3; i++) {
            const float t0 = Tcw[4 * i] * P[0] + Tcw[4 * i + 1] * P[1] + Tcw[4 * i + 2] * P[2];
            Pc[i] = (float)((double)t0 * 1.0 + (double)Tcw[4 * i + 3] * 1.0);
        }
        if (!finite3(Pc)) continue;
        if (Pc[2] < 0.0f) continue;
        if (Pc[2] == 0.0f) continue;
        const float invz = 1.0f / Pc[2];
        const float u = g->fx * Pc[0] * invz + g->cx;
        const float v = g->fy * Pc[1] * invz + g->cy;
        if (!isfinite(u) || !isfinite(v)) continue;
        if (u < g->min_x || u > g->max_x) continue;
        if (v < g->min_y || v > g->max_y) continue;
        const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)PO[k] * (double)PO[k];
        const float dist = (float)sqrt(s);
        if (!isfinite(dist) || dist == 0.0f) continue;
        const float maxDistance = 1.2f * max_dist[j];
        const float minDistance = 0.8f * min_dist[j];
        if (dist < minDistance || dist > maxDistance) continue;
        double d = 0;
        for (int k = 0; k < 3; k++) d += (double)PO[k] * (double)Pn[k];
        const float viewCos = (float)(d / (double)dist);
        if (!isfinite(viewCos)) continue;
        if (viewCos < viewing_cos_limit) continue;
        const float ratio = max_dist[j] / dist;
        if (!positive_normal(ratio)) continue;
        const float fl = ceilf(logf(ratio) / log_scale_factor);
        const int nScale = fl < 0.0f ? 0 : fl >= (float)g->nlevels ? g->nlevels - 1 : (int)fl;
        in_view[j] = 1;
        proj_x[j] = u;
        proj_y[j] = v;
        proj_xr[j] = u - g->bf * invz;
        level[j] = nScale;
        view_cos[j] = viewCos;
    }
    return 0;
}

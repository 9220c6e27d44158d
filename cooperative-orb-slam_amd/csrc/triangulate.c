/*
 * triangulate.c -- the per-match body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:284-450) with the per-pair
 * baseline test (:244-261) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:330-371) of the new point's two
 * observations, on the host for one pair of keyframes: the match row of SearchForTriangulation in, a status and a
 * position per feature and a compact table of new MapPoints out. Plain C, no device; built with -ffp-contract=off.
 *
 * The float sequence is stated in include/orbslam_amd.h (orbx_triangulate_matches); the same is restated in Python,
 * tests/triangulate_py.py, the yardstick, and on the device, frame_math.h (triangulate_match). The stereo
 * un-projection is orbx_unproject_stereo's (unproject.c), called, not restated.
 */
#include <float.h>
#include <math.h>
#include <string.h>

#include "../../include/orbslam_amd.h"

static double dot_d(const float* a, const float* b, int n) {
    double s = 0;
    for (int k = 0; k < n; k++) s += (double)a[k] * (double)b[k];
    return s;
}

/* vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV), 4x4 float: OpenCV 3.x's JacobiSVDImpl_ (a build
 * without LAPACK) on At = A.t(), with sqrt(p*p + beta*beta) where OpenCV calls hypot */
static void svd4_null(const float A[4][4], float x[4]) {
    float At[4][4], Vt[4][4];
    double W[4];
    for (int i = 0; i < 4; i++) {
        for (int k = 0; k < 4; k++) {
            At[i][k] = A[k][i];
            Vt[i][k] = i == k ? 1.0f : 0.0f;
        }
        W[i] = dot_d(At[i], At[i], 4);
    }
    const float eps = FLT_EPSILON * 2;
    for (int iter = 0; iter < 30; iter++) {
        int changed = 0;
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; j < 4; j++) {
                float *Ai = At[i], *Aj = At[j], *Vi = Vt[i], *Vj = Vt[j];
                double a = W[i], b = W[j], p = dot_d(Ai, Aj, 4);
                if (fabs(p) <= (double)eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * (double)s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * (double)c * 2));
                }
                a = b = 0;
                for (int k = 0; k < 4; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += (double)t0 * (double)t0;
                    b += (double)t1 * (double)t1;
                }
                W[i] = a;
                W[j] = b;
                changed = 1;
                for (int k = 0; k < 4; k++) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0;
                    Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    int row[4] = {0, 1, 2, 3};
    for (int i = 0; i < 4; i++) W[i] = sqrt(dot_d(At[i], At[i], 4));
    for (int i = 0; i < 3; i++) { /* selection sort, descending, strict <: the rows move with W */
        int j = i;
        for (int k = i + 1; k < 4; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double w = W[i];
            W[i] = W[j];
            W[j] = w;
            const int r = row[i];
            row[i] = row[j];
            row[j] = r;
        }
    }
    for (int k = 0; k < 4; k++) x[k] = Vt[row[3]][k];
}

static int finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

static void camera_center(const float* T, float Ow[3]) {
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)T[4 * k + i] * (double)T[4 * k + 3];
        Ow[i] = (float)(-1.0 * s);
    }
}

typedef struct {
    float x3D[3], normal[3], min_dist, max_dist;
} tri_point;

/* one match of a pair with finite poses that passed the baseline test */
static int triangulate_match(const orbm_tri_geom* g, const float* T1, const float* Ow1, const float* T2,
                             const float* Ow2, const orbx_kp* kp1, float ur1, float d1, const orbx_kp* kp2, float ur2,
                             float d2, tri_point* out) {
    const float u1 = kp1->x, v1 = kp1->y, u2 = kp2->x, v2 = kp2->y;
    const int o1 = kp1->octave, o2 = kp2->octave;
    if (o1 < 0 || o1 >= g->nlevels || o2 < 0 || o2 >= g->nlevels || !isfinite(u1) || !isfinite(v1) || !isfinite(u2) ||
        !isfinite(v2) || !isfinite(ur1) || !isfinite(ur2))
        return ORBM_TRI_EXCLUDED;
    const int st1 = ur1 >= 0, st2 = ur2 >= 0;
    if ((st1 || st2) && !(isfinite(g->b) && g->b > 0)) return ORBM_TRI_EXCLUDED;
    if ((st1 && !(isfinite(d1) && d1 > 0)) || (st2 && !(isfinite(d2) && d2 > 0))) return ORBM_TRI_EXCLUDED;
    const float invfx = 1.0f / g->fx, invfy = 1.0f / g->fy;
    const float xn1[3] = {(u1 - g->cx) * invfx, (v1 - g->cy) * invfy, 1.0f};
    const float xn2[3] = {(u2 - g->cx) * invfx, (v2 - g->cy) * invfy, 1.0f};
    float ray1[3], ray2[3];
    for (int i = 0; i < 3; i++) { /* row i of Rwc = column i of Rcw */
        ray1[i] = T1[i] * xn1[0] + T1[4 + i] * xn1[1] + T1[8 + i] * xn1[2];
        ray2[i] = T2[i] * xn2[0] + T2[4 + i] * xn2[1] + T2[8 + i] * xn2[2];
    }
    const float cosRays =
        (float)(dot_d(ray1, ray2, 3) / (sqrt(dot_d(ray1, ray1, 3)) * sqrt(dot_d(ray2, ray2, 3))));
    if (!isfinite(cosRays)) return ORBM_TRI_EXCLUDED;
    float cs1 = cosRays + 1.0f, cs2 = cs1;
    if (st1)
        cs1 = cosf(2.0f * atan2f(g->b * 0.5f, d1));
    else if (st2)
        cs2 = cosf(2.0f * atan2f(g->b * 0.5f, d2));
    const float cs = cs2 < cs1 ? cs2 : cs1;
    int made;
    float* x3D = out->x3D;
    if (cosRays < cs && cosRays > 0.0f && (st1 || st2 || (double)cosRays < 0.9998)) {
        float A[4][4], x4[4];
        for (int k = 0; k < 4; k++) {
            A[0][k] = xn1[0] * T1[8 + k] - T1[k];
            A[1][k] = xn1[1] * T1[8 + k] - T1[4 + k];
            A[2][k] = xn2[0] * T2[8 + k] - T2[k];
            A[3][k] = xn2[1] * T2[8 + k] - T2[4 + k];
        }
        svd4_null(A, x4);
        if (!finite3(x4) || !isfinite(x4[3])) return ORBM_TRI_EXCLUDED;
        if (x4[3] == 0.0f) return ORBM_TRI_W_ZERO;
        const float sc = (float)(1.0 / (double)x4[3]);
        for (int k = 0; k < 3; k++) x3D[k] = x4[k] * sc;
        made = ORBM_TRI_TRIANGULATED;
    } else if ((st1 && cs1 < cs2) || (st2 && cs2 < cs1)) {
        const int first = st1 && cs1 < cs2;
        orbx_camera cam;
        memset(&cam, 0, sizeof(cam));
        cam.fx = g->fx, cam.fy = g->fy, cam.cx = g->cx, cam.cy = g->cy;
        orbx_unproject_stereo(&cam, first ? T1 : T2, 1, first ? kp1 : kp2, first ? &d1 : &d2, x3D, NULL);
        made = first ? ORBM_TRI_STEREO1 : ORBM_TRI_STEREO2;
    } else {
        return ORBM_TRI_LOW_PARALLAX;
    }
    if (!finite3(x3D)) return ORBM_TRI_EXCLUDED;
    float c1[3], c2[3];
    for (int r = 0; r < 3; r++) {
        c1[r] = (float)(dot_d(T1 + 4 * r, x3D, 3) + (double)T1[4 * r + 3]);
        c2[r] = (float)(dot_d(T2 + 4 * r, x3D, 3) + (double)T2[4 * r + 3]);
    }
    if (!finite3(c1) || !finite3(c2)) return ORBM_TRI_EXCLUDED;
    if (c1[2] <= 0) return ORBM_TRI_Z1;
    if (c2[2] <= 0) return ORBM_TRI_Z2;
    for (int w = 0; w < 2; w++) {
        const float* c = w ? c2 : c1;
        const float u = w ? u2 : u1, v = w ? v2 : v1, ur = w ? ur2 : ur1;
        const float sigma2 = g->level_sigma2[w ? o2 : o1];
        const float invz = (float)(1.0 / (double)c[2]);
        const float pu = g->fx * c[0] * invz + g->cx;
        const float pv = g->fy * c[1] * invz + g->cy;
        const float ex = pu - u, ey = pv - v;
        float e2 = ex * ex + ey * ey;
        double th = 5.991;
        if (w ? st2 : st1) {
            const float pur = pu - g->bf * invz; /* KF1's mbf for both (:380, :406) */
            const float er = pur - ur;
            e2 = e2 + er * er;
            th = 7.8;
        }
        if (!isfinite(e2)) return ORBM_TRI_EXCLUDED;
        if ((double)e2 > th * (double)sigma2) return w ? ORBM_TRI_REPROJ2 : ORBM_TRI_REPROJ1;
    }
    const float n1[3] = {x3D[0] - Ow1[0], x3D[1] - Ow1[1], x3D[2] - Ow1[2]};
    const float n2[3] = {x3D[0] - Ow2[0], x3D[1] - Ow2[1], x3D[2] - Ow2[2]};
    const double nd1 = sqrt(dot_d(n1, n1, 3)), nd2 = sqrt(dot_d(n2, n2, 3));
    const float dist1 = (float)nd1, dist2 = (float)nd2;
    if (!isfinite(dist1) || !isfinite(dist2)) return ORBM_TRI_EXCLUDED;
    if (dist1 == 0 || dist2 == 0) return ORBM_TRI_DIST_ZERO;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = g->scale_factors[o1] / g->scale_factors[o2];
    const float ratioFactor = 1.5f * g->scale_factors[1];
    if (!isfinite(ratioDist)) return ORBM_TRI_EXCLUDED;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return ORBM_TRI_SCALE_RATIO;
    const float s1 = (float)(1.0 / nd1), s2 = (float)(1.0 / nd2);
    for (int k = 0; k < 3; k++) out->normal[k] = ((0.0f + n1[k] * s1) + n2[k] * s2) * 0.5f;
    out->max_dist = dist1 * g->scale_factors[o1];
    out->min_dist = out->max_dist / g->scale_factors[g->nlevels - 1];
    return made;
}

int orbx_triangulate_matches(const orbm_tri_geom* g, int monocular, float median_depth2, const float Tcw1[16],
                             const float Tcw2[16], int n1, const orbx_kp* kps1, const float* uright1,
                             const float* depth1, const uint8_t* desc1, int n2, const orbx_kp* kps2,
                             const float* uright2, const float* depth2, const int32_t* match12, int8_t* status,
                             float* pos3, float* tab_pos, float* tab_normal, float* tab_min_dist, float* tab_max_dist,
                             uint8_t* tab_desc, uint8_t* tab_flags, int32_t* tab_feat1, int32_t* tab_feat2,
                             int32_t* nnew) {
    if (!g || g->nlevels < 1 || g->nlevels > 16 || g->fx == 0 || g->fy == 0 || !Tcw1 || !Tcw2 || n1 < 0 || n2 < 0 ||
        !nnew || (n2 && !kps2) ||
        (n1 && (!kps1 || !desc1 || !match12 || !status || !pos3 || !tab_pos || !tab_normal || !tab_min_dist ||
                !tab_max_dist || !tab_desc || !tab_flags || !tab_feat1 || !tab_feat2)))
        return ORBX_EARG;
    int pose_ok = 1;
    for (int k = 0; k < 12; k++) pose_ok &= isfinite(Tcw1[k]) && isfinite(Tcw2[k]);
    float Ow1[3], Ow2[3];
    camera_center(Tcw1, Ow1);
    camera_center(Tcw2, Ow2);
    int skip = 0;
    if (pose_ok) { /* :244-261 */
        const float vb[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
        const float baseline = (float)sqrt(dot_d(vb, vb, 3));
        if (!monocular)
            skip = baseline < g->b;
        else
            skip = (double)(baseline / median_depth2) < 0.01;
    }
    int nn = 0;
    for (int i = 0; i < n1; i++) {
        status[i] = ORBM_TRI_NO_MATCH;
        pos3[3 * i] = pos3[3 * i + 1] = pos3[3 * i + 2] = 0.0f;
        const int idx2 = match12[i];
        if (idx2 < 0) continue;
        if (!pose_ok || idx2 >= n2) {
            status[i] = ORBM_TRI_EXCLUDED;
            continue;
        }
        if (skip) {
            status[i] = ORBM_TRI_BASELINE;
            continue;
        }
        tri_point pt;
        memset(&pt, 0, sizeof(pt));
        const int st = triangulate_match(g, Tcw1, Ow1, Tcw2, Ow2, kps1 + i, uright1 ? uright1[i] : -1.0f,
                                         depth1 ? depth1[i] : -1.0f, kps2 + idx2, uright2 ? uright2[idx2] : -1.0f,
                                         depth2 ? depth2[idx2] : -1.0f, &pt);
        status[i] = (int8_t)st;
        if (st < ORBM_TRI_TRIANGULATED || st > ORBM_TRI_STEREO2) continue;
        for (int k = 0; k < 3; k++) {
            pos3[3 * i + k] = pt.x3D[k];
            tab_pos[3 * nn + k] = pt.x3D[k];
            tab_normal[3 * nn + k] = pt.normal[k];
        }
        tab_min_dist[nn] = pt.min_dist;
        tab_max_dist[nn] = pt.max_dist;
        memcpy(tab_desc + 32 * (size_t)nn, desc1 + 32 * (size_t)i, 32);
        tab_flags[nn] = 9;
        tab_feat1[nn] = i;
        tab_feat2[nn] = idx2;
        nn++;
    }
    *nnew = nn;
    return 0;
}

/*
 * pose_optimize.c -- Optimizer::PoseOptimization(Frame*) (Optimizer.cc:239-451) on the host for one frame: the match
 * row of a tracking search in (each feature's MapPoint as a row of a position table), the optimised mTcw, mvbOutlier
 * and the return value out. Plain C, no device; built with -ffp-contract=off.
 *
 * The arithmetic is pose_math.h's (one statement for this unit and for k_pose_optimize); the sequence is stated in
 * include/orbslam_amd.h (orbx_pose_optimization) and restated in Python, tests/pose_py.py, the yardstick.
 */
#include <math.h>
#include <string.h>

#include "orbslam_amd_testing.h"

#define PM_FN static inline
#include "pose_math.h"

typedef struct {
    const pm_cam* cam;
    int n;
    const orbx_kp* kps;
    const float* uright;
    const int32_t* mp_index;
    const float* pos;
    const float* inv_sigma2;
    const uint32_t* lvl; /* bit i = feature i's edge is at level 1 (an outlier of the last classification) */
    double delta_mono, delta_stereo;
} pose_job;

static int is_stereo(const pose_job* j, int i) { return j->uright && !(j->uright[i] < 0); }

static double edge_at(const pose_job* j, int i, const double* est, double* out, int full, int robust) {
    const float* X = j->pos + 3 * (size_t)j->mp_index[i];
    const int st = is_stereo(j, i);
    const double delta = robust ? (st ? j->delta_stereo : j->delta_mono) : 0.0;
    return pose_edge_eval(j->cam, est, (double)X[0], (double)X[1], (double)X[2], (double)j->kps[i].x,
                          (double)j->kps[i].y, st ? (double)j->uright[i] : 0.0, st,
                          (double)j->inv_sigma2[j->kps[i].octave], delta, full, out, 1);
}

/* the active edges in ascending feature order: sum[k] = 0; sum[k] += term_k(edge) */
static void evaluate(const pose_job* j, const double* est, int full, int robust, double* sum) {
    double term[PM_NTERMS];
    for (int k = 0; k < PM_NTERMS; k++) sum[k] = 0.0;
    for (int i = 0; i < j->n; i++) {
        if (j->mp_index[i] < 0 || ((j->lvl[i >> 5] >> (i & 31)) & 1u)) continue;
        edge_at(j, i, est, term, full, robust);
        for (int k = full ? 0 : 27; k < PM_NTERMS; k++) sum[k] = sum[k] + term[k];
    }
}

int orbx_pose_optimization(const orbm_track_geom* g, const float* inv_level_sigma2, int nlevels, float Tcw[16], int n,
                           const orbx_kp* kps_un, const float* uright, const int32_t* mp_index, const float* pos,
                           uint8_t* outlier, int32_t* ninliers, int32_t* status, int32_t* diag) {
    if (!g || !inv_level_sigma2 || nlevels < 1 || nlevels > 16 || !Tcw || n < 0 || n > 65536 || !ninliers || !status ||
        (n && (!kps_un || !mp_index || !pos || !outlier)))
        return ORBX_EARG;
    int32_t dg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const pm_cam cam = {(double)g->fx, (double)g->fy, (double)g->cx, (double)g->cy, (double)g->bf};
    uint32_t lvl[65536 / 32]; /* n <= 65536, the kp_stride limit of the device entries */
    memset(lvl, 0, sizeof(uint32_t) * (size_t)((n + 31) / 32));
#define LVL(i) ((lvl[(i) >> 5] >> ((i) & 31)) & 1u)
    pose_job j = {&cam, n, kps_un, uright, mp_index, pos, inv_level_sigma2, lvl, 0, 0};
    j.delta_mono = (double)(float)sqrt(5.991);
    j.delta_stereo = (double)(float)sqrt(7.815);
    int st = ORBM_POSE_OK, ninit = 0, nbad = 0;
    for (int k = 0; k < 12; k++)
        if (!isfinite(Tcw[k])) st = ORBM_POSE_EXCLUDED;
    for (int i = 0; i < n; i++) {
        if (mp_index[i] < 0) continue;
        ninit++;
        const float* X = pos + 3 * (size_t)mp_index[i];
        if (kps_un[i].octave < 0 || kps_un[i].octave >= nlevels || !isfinite(kps_un[i].x) || !isfinite(kps_un[i].y) ||
            (uright && !isfinite(uright[i])) || !isfinite(X[0]) || !isfinite(X[1]) || !isfinite(X[2]))
            st = ORBM_POSE_EXCLUDED;
    }
    double est[7], saved[7], errst[7], x[6], sum[PM_NTERMS];
    pm_lm lm;
    memset(&lm, 0, sizeof(lm));
    if (st == ORBM_POSE_OK && ninit < 3) st = ORBM_POSE_TOO_FEW;
    int robust = 1;
    for (int it = 0; it < 4 && st == ORBM_POSE_OK; it++) {
        se3_from_Tcw(Tcw, est);
        memcpy(errst, est, sizeof(est));
        int nact = 0;
        for (int i = 0; i < n; i++) nact += mp_index[i] >= 0 && !LVL(i);
        for (int iter = 0; iter < 10 && nact > 0; iter++) {
            evaluate(&j, est, 1, robust, sum);
            memcpy(errst, est, sizeof(est));
            if (iter == 0 && !pm_finite(sum[27])) {
                st = ORBM_POSE_EXCLUDED;
                break;
            }
            pm_lm_iter_begin(&lm, sum, iter);
            int more;
            do {
                pm_lm_trial_step(&lm, sum, x, est, saved);
                double tmp[PM_NTERMS];
                evaluate(&j, est, 0, robust, tmp);
                memcpy(errst, est, sizeof(est));
                more = pm_lm_trial_end(&lm, sum, tmp[27], x, est, saved);
            } while (more);
            dg[1 + it]++;
            if (pm_lm_terminate(&lm)) break;
        }
        if (st != ORBM_POSE_OK) break;
        dg[0]++;
        /* :381-438: an inlier's chi2 is the error of the last evaluation (stale after a rejected last trial), an
         * outlier's is recomputed at the estimate */
        nbad = 0;
        for (int i = 0; i < n; i++) {
            if (mp_index[i] < 0) continue;
            const int o = pose_edge_outlier(edge_at(&j, i, LVL(i) ? est : errst, NULL, 0, 0), is_stereo(&j, i));
            if (o)
                lvl[i >> 5] |= 1u << (i & 31);
            else
                lvl[i >> 5] &= ~(1u << (i & 31));
            nbad += o;
        }
        if (it == 2) robust = 0;
        if (ninit < 10) break;
    }
    if (st == ORBM_POSE_OK) {
        se3_to_Tcw(est, Tcw);
        *ninliers = ninit - nbad;
    } else {
        *ninliers = 0;
    }
    if (st != ORBM_POSE_EXCLUDED)
        for (int i = 0; i < n; i++)
            if (mp_index[i] >= 0) outlier[i] = st == ORBM_POSE_OK ? (uint8_t)LVL(i) : 0;
    *status = st;
    dg[5] = lm.rejected;
    dg[6] = lm.fails;
    dg[7] = lm.small;
    if (diag) memcpy(diag, dg, sizeof(dg));
#undef LVL
    return 0;
}

/* ---- test hooks (orbslam_amd_testing.h) ---- */
int orbx_test_so3_sincos(const double* th, double* s, double* c, int n) {
    if (!th || !s || !c || n < 0) return ORBX_EARG;
    for (int i = 0; i < n; i++) so3_sincos(th[i], s + i, c + i);
    return 0;
}

int orbx_test_ldlt6_solve(const double A[36], const double b[6], double x[6]) {
    if (!A || !b || !x) return ORBX_EARG;
    return ldlt6_solve(A, b, x);
}

int orbx_test_se3(int op, const float Tcw_in[16], const double delta[6], double state[7], float Tcw_out[16]) {
    if (!Tcw_in || !state || !Tcw_out || (op == 1 && !delta)) return ORBX_EARG;
    int small = 0;
    se3_from_Tcw(Tcw_in, state);
    if (op == 1) small = se3_exp_mul(delta, state);
    se3_to_Tcw(state, Tcw_out);
    return small;
}

/* projection.cpp -- the matchers that project MapPoints into a frame's feature grid: SearchByProjection x4, Fuse x2,
 * SearchForInitialization, SearchBySim3 (host prologues: per-MapPoint geometry with the reference's float semantics;
 * the device grid / windowed search / claim resolution: frame_kernels.hip), and the distinctive descriptors. */
#include "matcher_host.h"

using namespace orbamd;

namespace {

/* cv::Mat float arithmetic as pinned in DESIGN.md (identical to the oracle's restatement):
 * A*x + c (3x3 by 3x1, flags 0) = OpenCV's small-matrix gemm path: float products and sums,
 * then (float)(t*alpha + c*beta) in double; A.t()*x (GEMM_1_T) = generic path, double
 * accumulation; norm/dot accumulate in double. */
void gemm33_fast(const float* A, int astep, const float* x, const float* c, float* d) {
    for (int i = 0; i < 3; i++) {
        const float* a = A + i * astep;
        const float t0 = a[0] * x[0] + a[1] * x[1] + a[2] * x[2];
        d[i] = (float)((double)t0 * 1.0 + (double)c[i] * 1.0);
    }
}
void gemm33t_neg(const float* A, int astep, const float* x, float* d) {
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)A[k * astep + i] * (double)x[k];
        d[i] = (float)(-1.0 * s);
    }
}
float norm3(const float* v) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
    return (float)std::sqrt(s);
}
double dot3(const float* a, const float* b) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)a[k] * (double)b[k];
    return s;
}
/* MapPoint::PredictScale (MapPoint.cc:385-417); log of a float = logf (pinned) */
int predict_scale(float max_dist, float currentDist, const orbm_frame_view* F) {
    const float ratio = max_dist / currentDist;
    int nScale = (int)std::ceil(logf(ratio) / F->log_scale_factor);
    if (nScale < 0)
        nScale = 0;
    else if (nScale >= F->nlevels)
        nScale = F->nlevels - 1;
    return nScale;
}
inline bool flag(const uint8_t* a, int i) { return a && a[i]; }

struct ProjBatch {
    std::vector<ProjQuery> q;
    std::vector<uint8_t> qdesc;
    void add(const ProjQuery& pq, const uint8_t* d) {
        q.push_back(pq);
        qdesc.insert(qdesc.end(), d, d + 32);
    }
};

bool frame_view_ok(const orbm_frame_view* F) {
    return F && F->n >= 0 && F->n < 65536 && F->nlevels >= 1 && F->nlevels <= 16 && F->scale_factors &&
           (F->n == 0 || (F->desc && F->x && F->y && F->octave));
}

/* uploads the Frame side + queries, runs k_grid / k_proj_scan / k_proj_resolve, downloads */
constexpr bool kProjDirect = true;  // Fuse: results written by the scan kernel (no k_proj_resolve wave)
/* init_n >= 0: SearchForInitialization (k_init_resolve) with F = F2 and match[] = vnMatches12 of F1's init_n
 * keypoints; otherwise match[] has F->n entries */
/* ce: the frame's cached device arrays and grid (orbm_kf_cache): only the queries travel, no k_grid */
int run_projection(orbm_ctx* ctx, const orbm_frame_view* F, const ProjBatch& pb, int accept_th, int ratio,
                   float nnratio, int check_ori, int32_t* match, int* nmatches, const float* inv_sigma2 = nullptr,
                   int32_t* qres = nullptr, int init_n = -1, const KfEntry* ce = nullptr) {
    if (const int rc_ = ctx->ready()) return rc_;
    const size_t n = (size_t)F->n, nq = pb.q.size();
    const size_t nout = init_n >= 0 ? (size_t)init_n : n;
    const size_t nF = ce ? 0 : n;  // per-feature arrays uploaded with the call
    // inputs first (staged in pinned memory, one H2D copy), then outputs (one D2H copy), then scratch
    Carve cv;
    const size_t o_call = cv.take(sizeof(ProjCall)), o_x = cv.take(4 * nF), o_y = cv.take(4 * nF),
                 o_ang = cv.take(4 * nF), o_ur = cv.take(4 * nF), o_oct = cv.take(4 * nF), o_occ = cv.take(n),
                 o_desc = cv.take(32 * nF), o_q = cv.take(sizeof(ProjQuery) * nq), o_qd = cv.take(32 * nq);
    const size_t in_bytes = cv.off;
    const size_t o_nm = cv.take(4 * nout + 4);  // nmatches, then match[nout]
    const size_t o_gs = cv.take(ce ? 0 : 4 * (kGridCols * kGridRows + 1)), o_gi = cv.take(2 * nF),
                 o_scan = cv.take(8 * (size_t)proj_topk() * nq), o_scnt = cv.take(4 * nq), o_res = cv.take(8 * nq);
    if (ctx->scratch.ensure(cv.off)) return ORBX_EDEVICE;
    // results: written by the kernels straight into the pinned buffer after the inputs (ProjCall::host_out)
    const size_t n_host = std::max(nout + 1, nq);
    uint8_t* hp = ctx->ensure_pinned(in_bytes + 8 * n_host);
    if (!hp) return ORBX_EDEVICE;
    uint8_t* base = ctx->scratch.as<uint8_t>();
    hipStream_t st = ctx->s();
    ProjCall c;
    memset(&c, 0, sizeof(c));
    c.x = (const float*)(base + o_x);
    c.y = (const float*)(base + o_y);
    c.angle = (const float*)(base + o_ang);
    c.uright = F->uright ? (const float*)(base + o_ur) : nullptr;
    c.octave = (const int32_t*)(base + o_oct);
    c.occ0 = F->occupied ? base + o_occ : nullptr;
    c.desc = base + o_desc;
    c.n = F->n;
    c.min_x = F->min_x;
    c.min_y = F->min_y;
    c.gw_inv = F->grid_w_inv;
    c.gh_inv = F->grid_h_inv;
    c.q = (const ProjQuery*)(base + o_q);
    c.qdesc = base + o_qd;
    c.nq = (int)nq;
    c.accept_th = accept_th;
    c.ratio = ratio;
    c.nnratio = nnratio;
    c.check_ori = check_ori && F->angle;
    // per-query results with nothing to arbitrate (Fuse): the scan writes them, no resolve wave
    bool claims = false;
    for (const ProjQuery& q : pb.q) claims |= (q.flags & kProjClaims) != 0;
    c.direct = kProjDirect && qres && !ratio && !c.check_ori && !claims;
    c.n_out = (int)nout;
    c.grid_start = (int*)(base + o_gs);
    c.grid_idx = (uint16_t*)(base + o_gi);
    if (ce) {
        c.x = (const float*)ce->at(ce->o_x);
        c.y = (const float*)ce->at(ce->o_y);
        c.angle = (const float*)ce->at(ce->o_ang);
        c.uright = F->uright && ce->has_ur ? (const float*)ce->at(ce->o_ur) : nullptr;
        c.octave = (const int32_t*)ce->at(ce->o_oct);
        c.desc = ce->at(ce->o_desc);
        c.grid_start = (int*)ce->at(ce->o_gs);
        c.grid_idx = (uint16_t*)ce->at(ce->o_gi);
    }
    c.scan = (unsigned long long*)(base + o_scan);
    c.scan_cnt = (int*)(base + o_scnt);
    c.res = (int*)(base + o_res);
    c.nmatches = (int32_t*)(base + o_nm);
    c.match = (int32_t*)(base + o_nm + 4);
    c.host_out = (unsigned long long*)ctx->pinned_on_device(in_bytes);
    c.seq = (int)ctx->next_seq();
    if (inv_sigma2)
        for (int l = 0; l < F->nlevels; l++) c.inv_sigma2[l] = inv_sigma2[l];
    memcpy(hp + o_call, &c, sizeof(c));
    if (n && F->occupied) memcpy(hp + o_occ, F->occupied, n);
    if (nF) {
        memcpy(hp + o_x, F->x, 4 * n);
        memcpy(hp + o_y, F->y, 4 * n);
        if (F->angle) memcpy(hp + o_ang, F->angle, 4 * n);
        if (F->uright) memcpy(hp + o_ur, F->uright, 4 * n);
        memcpy(hp + o_oct, F->octave, 4 * n);
        memcpy(hp + o_desc, F->desc, 32 * n);
    }
    if (nq) {
        memcpy(hp + o_q, pb.q.data(), sizeof(ProjQuery) * nq);
        memcpy(hp + o_qd, pb.qdesc.data(), 32 * nq);
    }
    const size_t nwait = c.direct ? nq : nout + 1;
    // the polled words start at 0, which no call carries (seq >= 1; see bow_small)
    memset(hp + in_bytes, 0, 8 * nwait);
    HIPR(hipMemcpyAsync(base, hp, in_bytes, hipMemcpyHostToDevice, st));
    HIPR(launch_projection((const ProjCall*)(base + o_call), 1, (int)nq, st, !c.direct, init_n >= 0, !ce));
    // poll the results (each carries this call's seq) instead of a D2H copy + stream synchronisation
    const unsigned long long* ho = (const unsigned long long*)(hp + in_bytes);
    const uint32_t seq = (uint32_t)c.seq;
    size_t next = 0;
    if (const int rc = wait_until(st, [&] {
            while (next < nwait && (uint32_t)(__atomic_load_n(ho + next, __ATOMIC_ACQUIRE) >> 32) == seq) next++;
            return next == nwait;
        }))
        return rc;
    if (qres) {
        // per-query results (Fuse): the accepted feature or -1, reported at the query's src
        if (c.direct)
            for (size_t qi = 0; qi < nq; qi++) qres[pb.q[qi].src] = (int32_t)(uint32_t)ho[qi];
        else {  // a resolve launch: per-query results stay on the device (res[2 qi])
            HIPR(hipMemcpyAsync(hp, base + o_res, 8 * nq, hipMemcpyDeviceToHost, st));
            HIPR(hipStreamSynchronize(st));
            for (size_t qi = 0; qi < nq; qi++) qres[pb.q[qi].src] = ((const int32_t*)hp)[2 * qi];
        }
        return 0;
    }
    for (size_t i = 0; i < nout; i++) match[i] = (int32_t)(uint32_t)ho[i];
    if (nmatches) *nmatches = (int)(uint32_t)ho[nout];
    return 0;
}

ProjQuery make_query(float u, float v, float radius, int minl, int maxl, float ur, float er_th, float angle, int flags,
                     int src) {
    ProjQuery q;
    q.u = u;
    q.v = v;
    q.radius = radius;
    q.min_level = minl;
    q.max_level = maxl;
    q.ur = ur;
    q.er_th = er_th;
    q.angle = angle;
    q.flags = flags | kProjValid;
    q.src = src;
    return q;
}

}  // namespace

extern "C" {

int orbm_search_by_projection_local(orbm_ctx* ctx, const orbm_frame_view* F, const orbm_mappoints* mp, float th,
                                    float nnratio, int32_t* match, int* nmatches) {
    if (!ctx || !frame_view_ok(F) || !mp || mp->n < 0 || (mp->n && (!mp->desc || !mp->track_in_view ||
        !mp->track_proj_x || !mp->track_proj_y || !mp->track_proj_xr || !mp->track_level || !mp->track_view_cos)) ||
        (F->n && !match))
        return ORBX_EARG;
    ProjBatch pb;
    const bool bFactor = th != 1.0;  // ORBmatcher.cc:49
    for (int iMP = 0; iMP < mp->n; iMP++) {
        if (!mp->track_in_view[iMP] || flag(mp->bad, iMP)) continue;
        const int lvl = mp->track_level[iMP];
        if (lvl < 0 || lvl >= F->nlevels) return ORBX_EARG;
        float r = mp->track_view_cos[iMP] > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos (:131-137)
        if (bFactor) r *= th;
        const float radius = r * F->scale_factors[lvl];
        pb.add(make_query(mp->track_proj_x[iMP], mp->track_proj_y[iMP], radius, lvl - 1, lvl, mp->track_proj_xr[iMP],
                          radius, 0.f, kProjStereo | (flag(mp->has_obs, iMP) ? kProjClaims : 0), iMP),
               mp->desc + 32 * (size_t)iMP);
    }
    return run_projection(ctx, F, pb, 100 /*TH_HIGH*/, 1, nnratio, 0, match, nmatches);
}

int orbm_search_by_projection_last_frame(orbm_ctx* ctx, const orbm_frame_view* F, const float Tcw_c[16],
                                         const orbm_mappoints* mp, const float Tcw_l[16], float th, int bMono,
                                         int check_ori, int32_t* match, int* nmatches) {
    if (!ctx || !frame_view_ok(F) || !Tcw_c || !Tcw_l || !mp || mp->n < 0 ||
        (mp->n && (!mp->desc || !mp->pos || !mp->octave || (check_ori && !mp->angle))) || (F->n && !match) ||
        (check_ori && !F->angle))
        return ORBX_EARG;
    const float* Rcw = Tcw_c;  // ORBmatcher.cc:1339-1351
    const float tcw[3] = {Tcw_c[3], Tcw_c[7], Tcw_c[11]};
    float twc[3], tlc[3];
    gemm33t_neg(Rcw, 4, tcw, twc);
    const float tlw[3] = {Tcw_l[3], Tcw_l[7], Tcw_l[11]};
    gemm33_fast(Tcw_l, 4, twc, tlw, tlc);
    const bool bForward = tlc[2] > F->b && !bMono;
    const bool bBackward = -tlc[2] > F->b && !bMono;
    ProjBatch pb;
    for (int i = 0; i < mp->n; i++) {  // :1353-1405
        if (flag(mp->skip, i)) continue;
        float x3Dc[3];
        gemm33_fast(Rcw, 4, mp->pos + 3 * (size_t)i, tcw, x3Dc);
        const float xc = x3Dc[0], yc = x3Dc[1];
        const float invzc = 1.0 / x3Dc[2];
        if (invzc < 0) continue;
        const float u = F->fx * xc * invzc + F->cx;
        const float v = F->fy * yc * invzc + F->cy;
        if (u < F->min_x || u > F->max_x) continue;
        if (v < F->min_y || v > F->max_y) continue;
        const int nLastOctave = mp->octave[i];
        if (nLastOctave < 0 || nLastOctave >= F->nlevels) return ORBX_EARG;
        const float radius = th * F->scale_factors[nLastOctave];
        int minl, maxl;
        if (bForward) {
            minl = nLastOctave;
            maxl = -1;
        } else if (bBackward) {
            minl = 0;
            maxl = nLastOctave;
        } else {
            minl = nLastOctave - 1;
            maxl = nLastOctave + 1;
        }
        const float ur = u - F->bf * invzc;
        pb.add(make_query(u, v, radius, minl, maxl, ur, radius, mp->angle ? mp->angle[i] : 0.f,
                          kProjStereo | (flag(mp->has_obs, i) ? kProjClaims : 0), i),
               mp->desc + 32 * (size_t)i);
    }
    return run_projection(ctx, F, pb, 100 /*TH_HIGH*/, 0, 0.f, check_ori, match, nmatches);
}

int orbm_search_by_projection_keyframe(orbm_ctx* ctx, const orbm_frame_view* F, const float Tcw_c[16],
                                       const orbm_mappoints* mp, float th, int orb_dist, int check_ori,
                                       int32_t* match, int* nmatches) {
    if (!ctx || !frame_view_ok(F) || !Tcw_c || !mp || mp->n < 0 ||
        (mp->n && (!mp->desc || !mp->pos || !mp->min_dist || !mp->max_dist || (check_ori && !mp->angle))) ||
        (F->n && !match) || (check_ori && !F->angle))
        return ORBX_EARG;
    const float* Rcw = Tcw_c;  // ORBmatcher.cc:1476-1478
    const float tcw[3] = {Tcw_c[3], Tcw_c[7], Tcw_c[11]};
    float Ow[3];
    gemm33t_neg(Rcw, 4, tcw, Ow);
    ProjBatch pb;
    for (int i = 0; i < mp->n; i++) {  // :1488-1537
        if (flag(mp->skip, i) || flag(mp->bad, i)) continue;
        const float* x3Dw = mp->pos + 3 * (size_t)i;
        float x3Dc[3];
        gemm33_fast(Rcw, 4, x3Dw, tcw, x3Dc);
        const float xc = x3Dc[0], yc = x3Dc[1];
        const float invzc = 1.0 / x3Dc[2];
        const float u = F->fx * xc * invzc + F->cx;
        const float v = F->fy * yc * invzc + F->cy;
        if (u < F->min_x || u > F->max_x) continue;
        if (v < F->min_y || v > F->max_y) continue;
        const float PO[3] = {x3Dw[0] - Ow[0], x3Dw[1] - Ow[1], x3Dw[2] - Ow[2]};
        const float dist3D = norm3(PO);
        const float maxDistance = 1.2f * mp->max_dist[i];
        const float minDistance = 0.8f * mp->min_dist[i];
        if (dist3D < minDistance || dist3D > maxDistance) continue;
        const int nPredictedLevel = predict_scale(mp->max_dist[i], dist3D, F);
        const float radius = th * F->scale_factors[nPredictedLevel];
        pb.add(make_query(u, v, radius, nPredictedLevel - 1, nPredictedLevel + 1, 0.f, -1.f,
                          mp->angle ? mp->angle[i] : 0.f, kProjClaims, i),
               mp->desc + 32 * (size_t)i);
    }
    return run_projection(ctx, F, pb, orb_dist, 0, 0.f, check_ori, match, nmatches);
}

int orbm_search_by_projection_sim3(orbm_ctx* ctx, const orbm_frame_view* KF, const float Scw[16],
                                   const orbm_mappoints* mp, int th, int32_t* match, int* nmatches) {
    if (!ctx || !frame_view_ok(KF) || !Scw || !mp || mp->n < 0 ||
        (mp->n && (!mp->desc || !mp->pos || !mp->normal || !mp->min_dist || !mp->max_dist)) || (KF->n && !match))
        return ORBX_EARG;
    // decompose Scw (ORBmatcher.cc:298-304): sRcw/scw and t/scw are convertTo with scale (float)(1./scw)
    const float scw = (float)std::sqrt(dot3(Scw, Scw));
    const float inv = (float)(1. / (double)scw);
    float Rcw[9], tcw[3], Ow[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rcw[3 * r + c] = Scw[4 * r + c] * inv;
        tcw[r] = Scw[4 * r + 3] * inv;
    }
    gemm33t_neg(Rcw, 3, tcw, Ow);
    ProjBatch pb;
    for (int iMP = 0; iMP < mp->n; iMP++) {  // :313-367
        if (flag(mp->bad, iMP) || flag(mp->skip, iMP)) continue;
        const float* p3Dw = mp->pos + 3 * (size_t)iMP;
        float p3Dc[3];
        gemm33_fast(Rcw, 3, p3Dw, tcw, p3Dc);
        if (p3Dc[2] < 0.0) continue;
        const float invz = 1 / p3Dc[2];
        const float x = p3Dc[0] * invz;
        const float y = p3Dc[1] * invz;
        const float u = KF->fx * x + KF->cx;
        const float v = KF->fy * y + KF->cy;
        if (!(u >= KF->min_x && u < KF->max_x && v >= KF->min_y && v < KF->max_y)) continue;  // IsInImage
        const float maxDistance = 1.2f * mp->max_dist[iMP];
        const float minDistance = 0.8f * mp->min_dist[iMP];
        const float PO[3] = {p3Dw[0] - Ow[0], p3Dw[1] - Ow[1], p3Dw[2] - Ow[2]};
        const float dist = norm3(PO);
        if (dist < minDistance || dist > maxDistance) continue;
        if (dot3(PO, mp->normal + 3 * (size_t)iMP) < 0.5 * dist) continue;
        const int nPredictedLevel = predict_scale(mp->max_dist[iMP], dist, KF);
        const float radius = th * KF->scale_factors[nPredictedLevel];
        // KeyFrame::GetFeaturesInArea has no level test; the caller's kpLevel window (:385-388)
        pb.add(make_query(u, v, radius, nPredictedLevel - 1, nPredictedLevel, 0.f, -1.f, 0.f, kProjClaims, iMP),
               mp->desc + 32 * (size_t)iMP);
    }
    return run_projection(ctx, KF, pb, 50 /*TH_LOW*/, 0, 0.f, 0, match, nmatches);
}

}  // extern "C"

/* ===================================================================================== */
/* ORBmatcher::Fuse x2: the per-MapPoint projection + windowed search on the device (the    */
/* k_grid / k_proj_scan / k_proj_resolve pipeline without claims); the map updates that     */
/* follow each match stay with the caller, in the reference's loop order                    */
/* ===================================================================================== */
static int fuse_common(orbm_ctx* ctx, const orbm_frame_view* KF, const float Tcw[16], const float Ow[3],
                       const orbm_mappoints* mp, float th, const float* inv_level_sigma2, int32_t* best_idx,
                       int* nfused, const KfEntry* ce = nullptr) {
    const float* Rcw = Tcw;  // ORBmatcher.cc:827-837
    const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]};
    ProjBatch pb;
    for (int i = 0; i < mp->n; i++) {  // :843-892
        best_idx[i] = -1;
        if (flag(mp->skip, i) || flag(mp->bad, i)) continue;
        const float* p3Dw = mp->pos + 3 * (size_t)i;
        float p3Dc[3];
        gemm33_fast(Rcw, 4, p3Dw, tcw, p3Dc);
        if (p3Dc[2] < 0.0f) continue;
        const float invz = 1 / p3Dc[2];
        const float x = p3Dc[0] * invz;
        const float y = p3Dc[1] * invz;
        const float u = KF->fx * x + KF->cx;
        const float v = KF->fy * y + KF->cy;
        if (!(u >= KF->min_x && u < KF->max_x && v >= KF->min_y && v < KF->max_y)) continue;  // IsInImage
        const float ur = u - KF->bf * invz;
        const float maxDistance = 1.2f * mp->max_dist[i];
        const float minDistance = 0.8f * mp->min_dist[i];
        const float PO[3] = {p3Dw[0] - Ow[0], p3Dw[1] - Ow[1], p3Dw[2] - Ow[2]};
        const float dist3D = norm3(PO);
        if (dist3D < minDistance || dist3D > maxDistance) continue;
        if (dot3(PO, mp->normal + 3 * (size_t)i) < 0.5 * dist3D) continue;
        const int nPredictedLevel = predict_scale(mp->max_dist[i], dist3D, KF);
        const float radius = th * KF->scale_factors[nPredictedLevel];
        // KeyFrame::GetFeaturesInArea has no level test; the caller's kpLevel window (:901-902)
        pb.add(make_query(u, v, radius, nPredictedLevel - 1, nPredictedLevel, ur, -1.f, 0.f, kProjChi2, i),
               mp->desc + 32 * (size_t)i);
    }
    orbm_frame_view K = *KF;
    K.occupied = nullptr;  // Fuse searches every feature
    const int rc = run_projection(ctx, &K, pb, 50 /*TH_LOW*/, 0, 0.f, 0, nullptr, nullptr, inv_level_sigma2, best_idx,
                                  -1, ce);
    if (rc) return rc;
    if (nfused) {
        int nf = 0;
        for (int i = 0; i < mp->n; i++) nf += best_idx[i] >= 0;
        *nfused = nf;
    }
    return 0;
}

static bool fuse_args_ok(orbm_ctx* ctx, const orbm_frame_view* KF, const float Tcw[16], const float Ow[3],
                         const orbm_mappoints* mp, const float* inv_level_sigma2, const int32_t* best_idx) {
    return ctx && frame_view_ok(KF) && Tcw && Ow && inv_level_sigma2 && mp && mp->n >= 0 &&
           !(mp->n && (!mp->desc || !mp->pos || !mp->normal || !mp->min_dist || !mp->max_dist || !best_idx));
}

extern "C" int orbm_fuse(orbm_ctx* ctx, const orbm_frame_view* KF, const float Tcw[16], const float Ow[3],
                         const orbm_mappoints* mp, float th, const float* inv_level_sigma2, int32_t* best_idx,
                         int* nfused) {
    if (!fuse_args_ok(ctx, KF, Tcw, Ow, mp, inv_level_sigma2, best_idx)) return ORBX_EARG;
    return fuse_common(ctx, KF, Tcw, Ow, mp, th, inv_level_sigma2, best_idx, nfused);
}

extern "C" {

int orbm_fuse_cached(orbm_ctx* ctx, orbm_kf_cache* cache, uint64_t key, const orbm_frame_view* KF, const float Tcw[16],
                     const float Ow[3], const orbm_mappoints* mp, float th, const float* inv_level_sigma2,
                     int32_t* best_idx, int* nfused) {
    if (!cache || !fuse_args_ok(ctx, KF, Tcw, Ow, mp, inv_level_sigma2, best_idx) || cache->device != ctx->device)
        return ORBX_EARG;
    if (const int rc_ = ctx->ready()) return rc_;
    const std::shared_ptr<KfEntry> ck = cache_get(cache, 1, key, nullptr, KF, ctx->s());
    if (!ck) return ORBX_EDEVICE;
    return fuse_common(ctx, KF, Tcw, Ow, mp, th, inv_level_sigma2, best_idx, nfused, ck.get());
}

int orbm_fuse_sim3(orbm_ctx* ctx, const orbm_frame_view* KF, const float Scw[16], const orbm_mappoints* mp, float th,
                   int32_t* best_idx, int* nfused) {
    if (!ctx || !frame_view_ok(KF) || !Scw || !mp || mp->n < 0 ||
        (mp->n && (!mp->desc || !mp->pos || !mp->normal || !mp->min_dist || !mp->max_dist || !best_idx)))
        return ORBX_EARG;
    // decompose Scw (ORBmatcher.cc:985-990) as in orbm_search_by_projection_sim3
    const float scw = (float)std::sqrt(dot3(Scw, Scw));
    const float inv = (float)(1. / (double)scw);
    float Rcw[9], tcw[3], Ow[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rcw[3 * r + c] = Scw[4 * r + c] * inv;
        tcw[r] = Scw[4 * r + 3] * inv;
    }
    gemm33t_neg(Rcw, 3, tcw, Ow);
    ProjBatch pb;
    for (int iMP = 0; iMP < mp->n; iMP++) {  // :1000-1052
        best_idx[iMP] = -1;
        if (flag(mp->bad, iMP) || flag(mp->skip, iMP)) continue;
        const float* p3Dw = mp->pos + 3 * (size_t)iMP;
        float p3Dc[3];
        gemm33_fast(Rcw, 3, p3Dw, tcw, p3Dc);
        if (p3Dc[2] < 0.0f) continue;
        const float invz = (float)(1.0 / (double)p3Dc[2]);  // 1.0/ here (:1019)
        const float x = p3Dc[0] * invz;
        const float y = p3Dc[1] * invz;
        const float u = KF->fx * x + KF->cx;
        const float v = KF->fy * y + KF->cy;
        if (!(u >= KF->min_x && u < KF->max_x && v >= KF->min_y && v < KF->max_y)) continue;  // IsInImage
        const float maxDistance = 1.2f * mp->max_dist[iMP];
        const float minDistance = 0.8f * mp->min_dist[iMP];
        const float PO[3] = {p3Dw[0] - Ow[0], p3Dw[1] - Ow[1], p3Dw[2] - Ow[2]};
        const float dist3D = norm3(PO);
        if (dist3D < minDistance || dist3D > maxDistance) continue;
        if (dot3(PO, mp->normal + 3 * (size_t)iMP) < 0.5 * dist3D) continue;
        const int nPredictedLevel = predict_scale(mp->max_dist[iMP], dist3D, KF);
        const float radius = th * KF->scale_factors[nPredictedLevel];
        pb.add(make_query(u, v, radius, nPredictedLevel - 1, nPredictedLevel, 0.f, -1.f, 0.f, 0, iMP),
               mp->desc + 32 * (size_t)iMP);
    }
    orbm_frame_view K = *KF;
    K.occupied = nullptr;
    const int rc = run_projection(ctx, &K, pb, 50 /*TH_LOW*/, 0, 0.f, 0, nullptr, nullptr, nullptr, best_idx);
    if (rc) return rc;
    if (nfused) {
        int nf = 0;
        for (int i = 0; i < mp->n; i++) nf += best_idx[i] >= 0;
        *nfused = nf;
    }
    return 0;
}

/* ORBmatcher::SearchForInitialization (ORBmatcher.cc:405-520): one query per F1 keypoint of octave <= 0
 * (level1 > 0 skips, :421-423) over F2's grid, window prev_xy[i1] +- windowSize at level level1 (:425);
 * the in-order resolution on the device (k_init_resolve). prev_xy is updated for the matched i1 (:514-517). */
int orbm_search_for_initialization(orbm_ctx* ctx, const orbm_frame_view* F1, const orbm_frame_view* F2, float* prev_xy,
                                   int window_size, float nnratio, int check_ori, int32_t* match12, int* nmatches) {
    if (!ctx || !frame_view_ok(F1) || !frame_view_ok(F2) || (F1->n && (!prev_xy || !match12)) ||
        (check_ori && ((F1->n && !F1->angle) || (F2->n && !F2->angle))))
        return ORBX_EARG;
    if (F1->n > init_max_features() || F2->n > init_max_features()) return ORBX_ECAPACITY;
    ProjBatch pb;
    for (int i1 = 0; i1 < F1->n; i1++) {
        const int level1 = F1->octave[i1];
        if (level1 > 0) continue;
        pb.add(make_query(prev_xy[2 * i1], prev_xy[2 * i1 + 1], (float)window_size, level1, level1, 0.f, 0.f,
                          check_ori ? F1->angle[i1] : 0.f, 0, i1),
               F1->desc + 32 * (size_t)i1);
    }
    int nm = 0;
    int rc = run_projection(ctx, F2, pb, 50 /*TH_LOW*/, 1, nnratio, check_ori, match12, &nm, nullptr, nullptr, F1->n);
    if (rc) return rc;
    for (int i1 = 0; i1 < F1->n; i1++)  // :514-517
        if (match12[i1] >= 0) {
            prev_xy[2 * i1] = F2->x[match12[i1]];
            prev_xy[2 * i1 + 1] = F2->y[match12[i1]];
        }
    if (nmatches) *nmatches = nm;
    return 0;
}

/* one direction of SearchBySim3 (ORBmatcher.cc:1148-1225, 1228-1305): the prologue of each MapPoint of the
 * source keyframe on the host (reference float semantics), the windowed first-strict-minimum search with
 * the octave band [nPredictedLevel-1, nPredictedLevel] on the device (per-query results, no claims) */
static int sim3_direction(orbm_ctx* ctx, const orbm_frame_view* KF, const float* Tsw, const orbm_mappoints* mp,
                          const float* sR, const float* t, float fx, float fy, float cx, float cy, float th,
                          int32_t* vnMatch) {
    const float Rsw[9] = {Tsw[0], Tsw[1], Tsw[2], Tsw[4], Tsw[5], Tsw[6], Tsw[8], Tsw[9], Tsw[10]};
    const float tsw[3] = {Tsw[3], Tsw[7], Tsw[11]};
    ProjBatch pb;
    for (int i = 0; i < mp->n; i++) {
        vnMatch[i] = -1;
        if (flag(mp->skip, i) || flag(mp->bad, i)) continue;  // :1152-1156
        const float* p3Dw = mp->pos + 3 * (size_t)i;
        float p3Dcs[3], p3Dct[3];
        gemm33_fast(Rsw, 3, p3Dw, tsw, p3Dcs);
        gemm33_fast(sR, 3, p3Dcs, t, p3Dct);
        if (p3Dct[2] < 0.0) continue;
        const float invz = 1.0 / p3Dct[2];
        const float x = p3Dct[0] * invz;
        const float y = p3Dct[1] * invz;
        const float u = fx * x + cx;
        const float v = fy * y + cy;
        if (!(u >= KF->min_x && u < KF->max_x && v >= KF->min_y && v < KF->max_y)) continue;  // IsInImage
        const float maxDistance = 1.2f * mp->max_dist[i];
        const float minDistance = 0.8f * mp->min_dist[i];
        const float dist3D = norm3(p3Dct);
        if (dist3D < minDistance || dist3D > maxDistance) continue;
        const int nPredictedLevel = predict_scale(mp->max_dist[i], dist3D, KF);
        const float radius = th * KF->scale_factors[nPredictedLevel];
        pb.add(make_query(u, v, radius, nPredictedLevel - 1, nPredictedLevel, 0.f, 0.f, 0.f, 0, i),
               mp->desc + 32 * (size_t)i);
    }
    if (pb.q.empty()) return 0;
    return run_projection(ctx, KF, pb, 100 /*TH_HIGH*/, 0, 0.f, 0, nullptr, nullptr, nullptr, vnMatch);
}

/* ORBmatcher::SearchBySim3 (ORBmatcher.cc:1102-1326) */
int orbm_search_by_sim3(orbm_ctx* ctx, const orbm_frame_view* KF1, const float T1w[16], const orbm_mappoints* mp1,
                        const orbm_frame_view* KF2, const float T2w[16], const orbm_mappoints* mp2, float s12,
                        const float R12[9], const float t12[3], float th, int32_t* match12, int* nfound) {
    auto mp_ok = [](const orbm_mappoints* m) {
        return m && m->n >= 0 && (m->n == 0 || (m->desc && m->pos && m->min_dist && m->max_dist));
    };
    if (!ctx || !frame_view_ok(KF1) || !frame_view_ok(KF2) || !T1w || !T2w || !mp_ok(mp1) || !mp_ok(mp2) || !R12 ||
        !t12 || (mp1->n && !match12) || !(s12 != 0.f))
        return ORBX_EARG;
    // sR12 = s12*R12, sR21 = (1.0/s12)*R12.t() (convertTo with a float scale), t21 = -sR21*t12 (small-matrix
    // gemm, alpha = -1) (:1119-1121)
    float sR12[9], sR21[9], t21[3];
    const float inv_s = (float)(1.0 / (double)s12);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            sR12[3 * r + c] = R12[3 * r + c] * s12;
            sR21[3 * r + c] = R12[3 * c + r] * inv_s;
        }
    for (int r = 0; r < 3; r++) {
        const float t0 = sR21[3 * r] * t12[0] + sR21[3 * r + 1] * t12[1] + sR21[3 * r + 2] * t12[2];
        t21[r] = (float)((double)t0 * -1.0);
    }
    std::vector<int32_t> m1((size_t)mp1->n + 1), m2((size_t)mp2->n + 1);
    // both directions project with pKF1's camera (:1105-1108, 1250-1251)
    int rc = sim3_direction(ctx, KF2, T1w, mp1, sR21, t21, KF1->fx, KF1->fy, KF1->cx, KF1->cy, th, m1.data());
    if (!rc) rc = sim3_direction(ctx, KF1, T2w, mp2, sR12, t12, KF1->fx, KF1->fy, KF1->cx, KF1->cy, th, m2.data());
    if (rc) return rc;
    int nFound = 0;
    for (int i1 = 0; i1 < mp1->n; i1++) {  // :1310-1323
        const int idx2 = m1[i1];
        match12[i1] = -1;
        if (idx2 >= 0 && idx2 < mp2->n && m2[idx2] == i1) {
            match12[i1] = idx2;
            nFound++;
        }
    }
    if (nfound) *nfound = nFound;
    return 0;
}

/* ===================================================================================== */
/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307), batched                 */
/* ===================================================================================== */
int orbm_compute_distinctive_descriptors_device(orbm_ctx* ctx, int npoints, const int32_t* d_offsets,
                                                const uint8_t* d_desc, int32_t* d_best_idx, uint8_t* d_out_desc,
                                                void* stream) {
    if (!ctx || npoints < 0 || (npoints && (!d_offsets || !d_desc || !d_best_idx))) return ORBX_EARG;
    if (npoints == 0) return 0;
    HIPR(hipSetDevice(ctx->device));
    HIPR(launch_distinctive(npoints, d_offsets, d_desc, d_best_idx, d_out_desc, (hipStream_t)stream));
    return 0;
}

int orbm_compute_distinctive_descriptors(orbm_ctx* ctx, int npoints, const int32_t* offsets, const uint8_t* desc,
                                         int32_t* best_idx, uint8_t* out_desc) {
    if (!ctx || npoints < 0 || (npoints && (!offsets || !best_idx))) return ORBX_EARG;
    if (npoints == 0) return 0;
    if (offsets[0] != 0) return ORBX_EARG;
    for (int p = 0; p < npoints; p++)
        if (offsets[p + 1] < offsets[p]) return ORBX_EARG;
    const size_t nrows = (size_t)offsets[npoints];
    if (nrows && !desc) return ORBX_EARG;
    if (const int rc_ = ctx->ready()) return rc_;
    Carve cv;
    const size_t o_off = cv.take(4 * ((size_t)npoints + 1)), o_desc = cv.take(32 * nrows), o_best = cv.take(4 * (size_t)npoints),
                 o_out = cv.take(32 * (size_t)npoints);
    if (ctx->scratch.ensure(cv.off)) return ORBX_EDEVICE;
    uint8_t* base = ctx->scratch.as<uint8_t>();
    hipStream_t st = ctx->s();
    HIPR(hipMemcpyAsync(base + o_off, offsets, 4 * ((size_t)npoints + 1), hipMemcpyHostToDevice, st));
    if (nrows) HIPR(hipMemcpyAsync(base + o_desc, desc, 32 * nrows, hipMemcpyHostToDevice, st));
    HIPR(launch_distinctive(npoints, (const int32_t*)(base + o_off), base + o_desc, (int32_t*)(base + o_best),
                            out_desc ? base + o_out : nullptr, st));
    HIPR(hipMemcpyAsync(best_idx, base + o_best, 4 * (size_t)npoints, hipMemcpyDeviceToHost, st));
    if (out_desc) HIPR(hipMemcpyAsync(out_desc, base + o_out, 32 * (size_t)npoints, hipMemcpyDeviceToHost, st));
    HIPR(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"

/*
 * orbslam_amd.h -- C ABI of the MI355X-native ORB front-end + Hamming matcher.
 *
 * This is the drop-in boundary underneath the reference's two C++ class surfaces
 * (ORB_SLAM2/include/ORBextractor.h:45-111, ORB_SLAM2/include/ORBmatcher.h:37-102; the
 * files are byte-identical in ORB_SLAM2/ and ORB_SLAM2.1/). Every entry point below
 * names the reference member it replaces. Plain pointers and sizes only; no torch,
 * OpenCV or HIP types cross it (streams are passed as `void*` = hipStream_t).
 *
 * Conventions:
 *   return 0 = OK, negative = error (ORBX_E*). Nothing throws across the ABI.
 *   Host entry points take host memory; *_device entry points take device memory and a
 *   stream and do not synchronise.
 *   A handle (orbx_handle / orbm_ctx) must not be used by two threads at once; create one
 *   per thread (the reference creates one ORBextractor per Tracking instance and stack
 *   ORBmatcher objects per thread: Tracking.cc:119-125, LocalMapping.cc:215).
 */
#ifndef ORBSLAM_AMD_H
#define ORBSLAM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_OK 0
#define ORBX_EARG (-1)     /* bad argument (null pointer, size out of range)          */
#define ORBX_EDEVICE (-2)  /* HIP runtime / kernel failure, or no usable device        */
#define ORBX_ECAPACITY (-3) /* caller buffer too small for the result                  */

/* ------------------------------------------------------------------------------------
 * Extractor -- replaces ORB_SLAM2::ORBextractor (ORBextractor.h:45-111, .cc:410-1132)
 * ---------------------------------------------------------------------------------- */

/* ctor arguments of ORBextractor::ORBextractor (ORBextractor.cc:410-411); the values the
 * reference runs with are my.yaml:31-43 = {1000, 1.2f, 8, 20, 7}. */
typedef struct orbx_params {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} orbx_params;

/* One output keypoint = cv::KeyPoint of ORBextractor::operator() (ORBextractor.cc:1043-1105)
 * minus class_id (always -1 in the reference). 24 bytes. Coordinates are level-0 pixels
 * (pt *= mvScaleFactor[level], ORBextractor.cc:1095-1101). */
typedef struct orbx_kp {
    float x, y;
    float size;      /* (int)(PATCH_SIZE * mvScaleFactor[level])  ORBextractor.cc:837,846 */
    float angle;     /* IC_Angle, degrees in [0,360]               ORBextractor.cc:77-104  */
    float response;  /* FAST score                                 ORBextractor.cc:809-816 */
    int32_t octave;  /* pyramid level                              ORBextractor.cc:845     */
} orbx_kp;

typedef struct orbx_handle orbx_handle;

/* ORBextractor::ORBextractor (ORBextractor.cc:410-470). Device buffers are sized for frames
 * up to max_width x max_height and batches up to max_batch frames. device = HIP ordinal. */
int orbx_create(const orbx_params* params, int device, int max_width, int max_height,
                int max_batch, orbx_handle** out);
void orbx_destroy(orbx_handle* h);

/* Upper bound on keypoints one frame can produce: sum over levels of
 * max(N_l + 3, 4*nIni_l) (DistributeOctTree overshoot, ORBextractor.cc:669-735). */
int orbx_max_keypoints(const orbx_handle* h, int width, int height);

/* ORBextractor::operator()(image, mask(ignored), keypoints, descriptors)
 * (ORBextractor.cc:1043-1105). Host image (8UC1, row pitch in bytes); outputs written to
 * host arrays kps[cap], desc[cap*32] in the reference's order (levels 0..L-1, each in
 * DistributeOctTree order). *n = keypoint count. Empty image (w or h == 0) -> *n = 0,
 * outputs untouched (ORBextractor.cc:1046-1047). */
int orbx_extract(orbx_handle* h, const uint8_t* img, int width, int height, size_t pitch,
                 orbx_kp* kps, uint8_t* desc, int cap, int* n);

/* Batched, device-resident form of operator(): nframes frames at d_frames + f*frame_stride
 * (each width x height, row pitch `pitch`). Per frame f: kps at d_kps + f*kp_stride,
 * descriptors at d_desc + f*kp_stride*32, count at d_counts[f]. kp_stride must be
 * >= orbx_max_keypoints(). Enqueued on `stream` (hipStream_t); no host sync. */
int orbx_extract_batch_device(orbx_handle* h, int nframes, const uint8_t* d_frames,
                              size_t frame_stride, int width, int height, size_t pitch,
                              orbx_kp* d_kps, uint8_t* d_desc, int32_t* d_counts,
                              int kp_stride, void* stream);

/* Waits for `stream` and reports a device-side consistency failure (octree capacity or
 * root-index overflow) of any batched extraction since the previous check: 0 = OK,
 * ORBX_EDEVICE otherwise (the flag is then cleared). */
int orbx_check_error(orbx_handle* h, void* stream);

/* public ORBextractor::mvImagePyramid (ORBextractor.h:85), materialised lazily: copies
 * level `level` of frame `frame` of the most recent extraction to host dst (pitch bytes).
 * Pass dst = NULL to query the size only. */
int orbx_pyramid_level(orbx_handle* h, int frame, int level, uint8_t* dst, size_t pitch,
                       int* width, int* height);

/* public ORBextractor::mvImagePyramid (ORBextractor.h:85, filled by ComputePyramid in every
 * operator() call, ORBextractor.cc:1107-1132) delivered eagerly for the host path without a
 * copy after the call: with on != 0 every subsequent orbx_extract on `h` also writes the frame's
 * levels 1..L-1 into pinned host memory from extra workgroups of its octree launch (they copy
 * while the octree runs, so the call's latency does not grow), and orbx_host_pyramid_level then
 * points at level `level` of the last orbx_extract (level 0: the call's pinned copy of the
 * input image). The memory belongs to the handle: valid until the next orbx_extract,
 * orbx_set_host_pyramid or orbx_destroy on it. ORBX_EARG when the last call delivered none
 * (host pyramid off, or a stage-profiled call). */
int orbx_set_host_pyramid(orbx_handle* h, int on);
int orbx_host_pyramid_level(orbx_handle* h, int level, const uint8_t** data, size_t* pitch,
                            int* width, int* height);

/* Caller-owned destination of that eager pyramid. The reference assigns every level a freshly
 * allocated Mat in each call (ORBextractor.cc:1114-1115), so a level a caller keeps is never
 * overwritten by a later call; the drop-in ORBextractor keeps that by handing each call storage no
 * caller holds (host/ORBextractor.cc). orbx_host_pyramid_bytes: bytes of one target for a
 * width x height frame (level 0 contiguous at offset 0, rounded up to 256, then levels 1..L-1 in
 * the device layout). orbx_host_register / orbx_host_unregister: make caller memory writable by
 * the device (mapped) and release it again. orbx_set_host_pyramid_target: subsequent
 * orbx_extract calls on `h` write their levels into `host` (registered, >= bytes of the frame;
 * ORBX_EARG from orbx_extract otherwise), and orbx_host_pyramid_level then points into the target
 * the last call filled; host = NULL returns to the handle's own pinned memory. The target stays
 * the caller's: the library never frees or unregisters it. */
int orbx_host_pyramid_bytes(orbx_handle* h, int width, int height, size_t* bytes);
int orbx_host_register(void* p, size_t bytes);
int orbx_host_unregister(void* p);
int orbx_set_host_pyramid_target(orbx_handle* h, uint8_t* host, size_t bytes);

/* ORBextractor getters (ORBextractor.h:63-81): GetLevels, GetScaleFactor,
 * GetScaleFactors, GetInverseScaleFactors, GetScaleSigmaSquares,
 * GetInverseScaleSigmaSquares. Arrays have nlevels entries. */
int orbx_get_levels(const orbx_handle* h);
float orbx_get_scale_factor(const orbx_handle* h);
int orbx_get_scale_tables(const orbx_handle* h, float* scale, float* inv_scale, float* sigma2,
                          float* inv_sigma2);
/* The same four tables from the ctor arguments alone, host-only (no device, no handle): the
 * drop-in ORBextractor answers its getters from these even when no device is usable. */
int orbx_compute_scale_tables(const orbx_params* params, float* scale, float* inv_scale, float* sigma2,
                              float* inv_sigma2);
/* mnFeaturesPerLevel (ORBextractor.cc:435-446) and umax (ORBextractor.cc:454-469, 16
 * entries) -- exposed for tests. */
int orbx_get_feature_split(const orbx_handle* h, int32_t* per_level, int32_t* umax16);

/* ------------------------------------------------------------------------------------
 * Matcher -- replaces ORB_SLAM2::ORBmatcher (ORBmatcher.h:37-102, ORBmatcher.cc)
 * ---------------------------------------------------------------------------------- */

/* One KeyFrame/Frame as the matcher sees it, gathered by the caller under its own
 * locks (KeyFrame::GetMapPoint/GetMapPointMatches, ORBmatcher.cc:526,699,722).
 * All arrays have n entries unless noted; host or device memory depending on the call. */
typedef struct orbm_kf_view {
    int32_t n;                 /* KeyFrame::N                                              */
    const uint8_t* desc;       /* mDescriptors, n x 32 contiguous rows                     */
    const float* x;            /* mvKeysUn[i].pt.x                                         */
    const float* y;            /* mvKeysUn[i].pt.y                                         */
    const float* angle;        /* mvKeysUn[i].angle (== mvKeys[i].angle)                   */
    const int32_t* octave;     /* mvKeysUn[i].octave                                       */
    const float* uright;       /* mvuRight; NULL = monocular (all -1)                      */
    const uint8_t* has_mp;     /* GetMapPoint(i) != NULL; NULL = none                      */
    const uint8_t* mp_bad;     /* that MapPoint's isBad(); NULL = none bad                 */
    int32_t n_nodes;           /* DBoW2::FeatureVector as CSR, node ids ascending          */
    const uint32_t* node_id;   /* [n_nodes]                                                */
    const int32_t* node_off;   /* [n_nodes+1] offsets into node_feat                       */
    const int32_t* node_feat;  /* feature indices, ascending within a node                 */
    int32_t nlevels;
    const float* scale_factors; /* mvScaleFactors[nlevels]                                 */
    const float* level_sigma2;  /* mvLevelSigma2[nlevels]                                  */
} orbm_kf_view;

typedef struct orbm_ctx orbm_ctx;

/* ORBmatcher::ORBmatcher(nnratio, checkOri) state lives in the call arguments; the ctx
 * only owns a device, a stream and scratch (one per thread). */
int orbm_create(int device, orbm_ctx** out);
void orbm_destroy(orbm_ctx* ctx);

/* ORBmatcher::DescriptorDistance (ORBmatcher.cc:1647-1663): host, 32-byte rows. */
int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* ORBmatcher::SearchForTriangulation (ORBmatcher.cc:657-823). F12 = 3x3 row-major float
 * (F12.at<float>(r,c)); (ex,ey) = epipole of KF1's centre in KF2 (ORBmatcher.cc:664-670,
 * see orbm_epipole). match12[kf1.n] receives idx2 or -1; *nmatches = pair count. */
int orbm_search_for_triangulation(orbm_ctx* ctx, const orbm_kf_view* kf1, const orbm_kf_view* kf2,
                                  const float F12[9], float ex, float ey, int only_stereo,
                                  int check_ori, int32_t* match12, int* nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (ORBmatcher.cc:159-288).
 * match_f[f.n] receives the KF feature index whose MapPoint was assigned to that Frame
 * feature (vpMapPointMatches[i] = pKF->GetMapPointMatches()[match_f[i]]) or -1. */
int orbm_search_by_bow_kf_f(orbm_ctx* ctx, const orbm_kf_view* kf, const orbm_kf_view* f,
                            float nnratio, int check_ori, int32_t* match_f, int* nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (ORBmatcher.cc:522-655).
 * match12[kf1.n] receives idx2 (vpMatches12[idx1] = vpMapPoints2[idx2]) or -1. */
int orbm_search_by_bow_kf_kf(orbm_ctx* ctx, const orbm_kf_view* kf1, const orbm_kf_view* kf2,
                             float nnratio, int check_ori, int32_t* match12, int* nmatches);

/* Device batch of SearchForTriangulation with one FeatureVector node holding every
 * feature of both keyframes (the BASELINE "BF" configuration): pair p
 * matches frame q1[p] (KF1) against frame q2[p] (KF2) of an orbx_extract_batch_device
 * output (kps/desc/counts/kp_stride as produced there). All keypoints monocular, no
 * MapPoints, one F12/(ex,ey) and one scale table for all pairs. match12[p*kp_stride+i]; only
 * rows i < counts[q1[p]] are written. kp_stride <= 65536 (ORBX_EARG above it, here and in the
 * stereo form: the kernel's selection key holds the candidate index in 16 bits).
 * This call and the stereo form keep per-launch scratch in the context (the pairs' queries and
 * candidates ordered along the epipolar lines, for kp_stride <= 4096; grown before anything is
 * enqueued, when a launch is larger than any before it): calls that share a context must be
 * ordered on one stream. A context of its own per stream lifts that. */
int orbm_triangulation_bf_batch_device(orbm_ctx* ctx, int npairs, const int32_t* d_q1,
                                       const int32_t* d_q2, const orbx_kp* d_kps,
                                       const uint8_t* d_desc, const int32_t* d_counts,
                                       int kp_stride, const float F12[9], float ex, float ey,
                                       int nlevels, const float* scale_factors,
                                       const float* level_sigma2, int check_ori,
                                       int32_t* d_match12, int32_t* d_nmatches, void* stream);
/* The stereo form of the same batch (ORBmatcher.cc:657-823 with mvuRight, as LocalMapping::CreateNewMapPoints
 * calls it between stereo keyframes): d_uright[f*kp_stride + i] = mvuRight of keypoint i of frame f (-1 =
 * monocular), e.g. the output of orbx_stereo_matches_batch_device for the left frames. The epipole-radius test
 * applies to monocular-monocular pairs only (:743-749); only_stereo = bOnlyStereo (:705-707, :729-731). No
 * MapPoints, one F12/(ex,ey) and scale table for all pairs, match12 / nmatches as above. */
int orbm_triangulation_bf_stereo_batch_device(orbm_ctx* ctx, int npairs, const int32_t* d_q1,
                                              const int32_t* d_q2, const orbx_kp* d_kps,
                                              const uint8_t* d_desc, const int32_t* d_counts,
                                              const float* d_uright, int kp_stride, const float F12[9],
                                              float ex, float ey, int nlevels,
                                              const float* scale_factors, const float* level_sigma2,
                                              int only_stereo, int check_ori, int32_t* d_match12,
                                              int32_t* d_nmatches, void* stream);
/* The same batch over common BoW nodes (SearchForTriangulation's own merge walk,
 * ORBmatcher.cc:691-789, as LocalMapping::CreateNewMapPoints calls it with a real vocabulary):
 * the FeatureVectors are orbv_transform_batch_device's device output for the same frames
 * (fv_node / fv_feat at f*kp_stride, fv_off at f*(kp_stride+1), nfv[f]); max_nodes bounds nfv
 * (e.g. min(kp_stride, k^(L-levelsup))). Mono, no MapPoints, as above. */
int orbm_triangulation_nodes_batch_device(orbm_ctx* ctx, int npairs, const int32_t* d_q1,
                                          const int32_t* d_q2, const orbx_kp* d_kps,
                                          const uint8_t* d_desc, const int32_t* d_counts,
                                          int kp_stride, const uint32_t* d_fv_node,
                                          const int32_t* d_fv_off, const int32_t* d_fv_feat,
                                          const int32_t* d_nfv, int max_nodes, const float F12[9],
                                          float ex, float ey, int nlevels,
                                          const float* scale_factors, const float* level_sigma2,
                                          int check_ori, int32_t* d_match12, int32_t* d_nmatches,
                                          void* stream);
/* SearchByBoW for a batch of frame pairs over the same device FeatureVectors: mode 1 =
 * SearchByBoW(KF1, KF2, vpMatches12) (ORBmatcher.cc:522-655; out[p*kp_stride + idx1] = idx2),
 * mode 0 = SearchByBoW(KF, F, vpMapPointMatches) (:159-288; qf = KF, cf = F,
 * out[p*kp_stride + idxF] = idxKF). mp_flags[f*kp_stride + idx]: bit 0 = the feature has a
 * MapPoint, bit 1 = that MapPoint is bad (the KF side, and in mode 1 both sides, need bit 0
 * without bit 1). Rotation histogram with check_ori. nmatches[p] = entries >= 0. */
int orbm_search_by_bow_batch_device(orbm_ctx* ctx, int npairs, int mode, const int32_t* d_qf,
                                    const int32_t* d_cf, const orbx_kp* d_kps,
                                    const uint8_t* d_desc, const int32_t* d_counts, int kp_stride,
                                    const uint8_t* d_mp_flags, const uint32_t* d_fv_node,
                                    const int32_t* d_fv_off, const int32_t* d_fv_feat,
                                    const int32_t* d_nfv, int max_nodes, float nnratio,
                                    int check_ori, int32_t* d_out, int32_t* d_nmatches,
                                    void* stream);

/* The four batches above read d_kps as the keyframes' mvKeysUn (the epipolar test is written on
 * it, ORBmatcher.cc:743-760): with a distorted camera d_kps is the d_kps_un output of
 * orbx_undistort_batch_device, not the extractor's own array. */

/* Waits for `stream` and reports (then clears) the ctx's device error flag, raised by the
 * *_device calls that validate device-resident input (orbm_search_for_triangulation_slots_device:
 * a malformed or foreign slot, a query count above its capacity): 0 = OK, ORBX_EDEVICE. */
int orbm_check_error(orbm_ctx* ctx, void* stream);

/* Epipole helper (ORBmatcher.cc:664-670): C2 = R2w*Cw + t2w with OpenCV's small-matrix gemm
 * semantics (float products/sums, + t in double, one rounding; DESIGN.md "Pinned semantics"),
 * ex = fx*C2.x*invz + cx, ey likewise. */
void orbm_epipole(const float R2w[9], const float t2w[3], const float Cw[3], float fx, float fy,
                  float cx, float cy, float* ex, float* ey);

/* ------------------------------------------------------------------------------------
 * SearchByProjection x4 (ORBmatcher.cc:45-129, 1328-1470, 1472-1599, 290-403) with
 * Frame/KeyFrame::GetFeaturesInArea over the 64x48 feature grid (Frame.cc:235-250,
 * 332-389; KeyFrame.cc:569-613). The per-MapPoint geometry prologue of each variant
 * (projection, frustum/scale tests, PredictScale) runs on the host with the reference's
 * float semantics (DESIGN.md "Pinned semantics"); the grid build, windowed Hamming search
 * (best / second best), the in-order claim resolution and the rotation histogram run on the
 * device.
 * ---------------------------------------------------------------------------------- */

/* The Frame (or KeyFrame) side. */
typedef struct orbm_frame_view {
    int32_t n;                    /* N                                                    */
    const uint8_t* desc;          /* mDescriptors, n x 32                                 */
    const float* x;               /* mvKeysUn[i].pt.x                                     */
    const float* y;               /* mvKeysUn[i].pt.y                                     */
    const int32_t* octave;        /* mvKeysUn[i].octave                                   */
    const float* angle;           /* mvKeysUn[i].angle (rotation histogram)               */
    const float* uright;          /* mvuRight; NULL = monocular (all -1)                  */
    const uint8_t* occupied;      /* the variant's "already matched" test on the state
                                     before the call (see each entry point); NULL = none  */
    float min_x, min_y, max_x, max_y;  /* mnMinX, mnMinY, mnMaxX, mnMaxY                  */
    float grid_w_inv, grid_h_inv;      /* mfGridElementWidthInv, mfGridElementHeightInv   */
    float fx, fy, cx, cy;              /* camera                                          */
    float bf, b;                       /* mbf, mb                                         */
    int32_t nlevels;                   /* mnScaleLevels                                   */
    const float* scale_factors;        /* mvScaleFactors[nlevels]                         */
    float log_scale_factor;            /* mfLogScaleFactor                                */
} orbm_frame_view;

/* The MapPoint side (one entry per candidate MapPoint, in the reference's loop order).
 * Each entry point documents which arrays it reads; the rest may be NULL. */
typedef struct orbm_mappoints {
    int32_t n;
    const uint8_t* desc;          /* GetDescriptor(), n x 32                              */
    const float* pos;             /* GetWorldPos(), n x 3                                 */
    const float* normal;          /* GetNormal(), n x 3                                   */
    const float* min_dist;        /* mfMinDistance (GetMinDistanceInvariance = 0.8f*it)   */
    const float* max_dist;        /* mfMaxDistance (GetMaxDistanceInvariance = 1.2f*it)   */
    const uint8_t* bad;           /* isBad()                                              */
    const uint8_t* has_obs;       /* Observations() > 0                                   */
    const uint8_t* skip;          /* entry excluded before any test (see entry points)    */
    const int32_t* octave;        /* source keypoint octave (SearchByProjection(F, LastF)) */
    const float* angle;           /* source keypoint angle (rotation histogram)           */
    /* Tracking fields set by Frame::isInFrustum (Frame.cc:274-330) */
    const uint8_t* track_in_view; /* mbTrackInView                                        */
    const float* track_proj_x;    /* mTrackProjX                                          */
    const float* track_proj_y;    /* mTrackProjY                                          */
    const float* track_proj_xr;   /* mTrackProjXR                                         */
    const int32_t* track_level;   /* mnTrackScaleLevel                                    */
    const float* track_view_cos;  /* mTrackViewCos                                        */
} orbm_mappoints;

/* Results of every variant: match[view.n] = index (into the orbm_mappoints) of the MapPoint
 * the call assigned to that feature (the last assignment wins, as in the reference), -1 if
 * the call left the feature untouched, -2 if the rotation-consistency filter reset it to
 * NULL; *nmatches = the reference's return value. */

/* ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-129).
 * F.occupied[i] = F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0. Reads mp: desc,
 * bad, has_obs, track_*. nnratio = mfNNratio. */
int orbm_search_by_projection_local(orbm_ctx* ctx, const orbm_frame_view* F, const orbm_mappoints* mp,
                                    float th, float nnratio, int32_t* match, int* nmatches);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
 * (ORBmatcher.cc:1328-1470). mp = LastFrame's N entries: skip[i] = !LastFrame.mvpMapPoints[i]
 * || LastFrame.mvbOutlier[i]; pos, desc, has_obs of that MapPoint; octave = LastFrame.mvKeys[i]
 * .octave; angle = LastFrame.mvKeysUn[i].angle. F.occupied as in _local. Tcw_cur / Tcw_last =
 * the frames' mTcw (4x4 row-major float). */
int orbm_search_by_projection_last_frame(orbm_ctx* ctx, const orbm_frame_view* F, const float Tcw_cur[16],
                                         const orbm_mappoints* mp, const float Tcw_last[16], float th, int mono,
                                         int check_ori, int32_t* match, int* nmatches);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>&
 * sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1472-1599). mp = pKF->GetMapPointMatches():
 * skip[i] = NULL entry or in sAlreadyFound; pos, desc, bad, min_dist, max_dist; angle =
 * pKF->mvKeysUn[i].angle. F.occupied[i] = CurrentFrame.mvpMapPoints[i] != NULL. */
int orbm_search_by_projection_keyframe(orbm_ctx* ctx, const orbm_frame_view* F, const float Tcw_cur[16],
                                       const orbm_mappoints* mp, float th, int orb_dist, int check_ori,
                                       int32_t* match, int* nmatches);

/* ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
 * vector<MapPoint*>& vpMatched, th) (ORBmatcher.cc:290-403). KF.occupied[i] = vpMatched[i] !=
 * NULL; mp = vpPoints: skip[i] = in spAlreadyFound (the non-NULL entries of vpMatched); pos,
 * normal, desc, bad, min_dist, max_dist. Scw = 4x4 row-major float Sim3. */
int orbm_search_by_projection_sim3(orbm_ctx* ctx, const orbm_frame_view* KF, const float Scw[16],
                                   const orbm_mappoints* mp, int th, int32_t* match, int* nmatches);

/* ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th) (ORBmatcher.cc:825-975,
 * called by LocalMapping::SearchInNeighbors, LocalMapping.cc:489,514): the per-MapPoint projection,
 * frustum / scale / viewing-angle tests, windowed search with the reprojection-error (chi2) test on
 * the device; best_idx[i] = the keypoint of pKF that MapPoint i fuses with (bestDist <= TH_LOW),
 * -1 otherwise, *nfused = the reference's return value. The caller then applies, for i in order,
 * the reference's update (:947-971: Replace by Observations() or AddObservation + AddMapPoint),
 * re-checking isBad() / IsInKeyFrame(pKF) at that point exactly as the reference loop does (an
 * entry that turns true there was changed by an earlier update and is skipped). mp: skip = NULL
 * entry or IsInKeyFrame(pKF), bad, pos, normal, desc, min_dist, max_dist. KF.occupied is ignored.
 * Tcw = pKF->GetPose() (4x4 row-major), Ow = pKF->GetCameraCenter(), inv_level_sigma2 =
 * pKF->mvInvLevelSigma2[nlevels]. */
int orbm_fuse(orbm_ctx* ctx, const orbm_frame_view* KF, const float Tcw[16], const float Ow[3],
              const orbm_mappoints* mp, float th, const float* inv_level_sigma2, int32_t* best_idx, int* nfused);

/* ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, th, vpReplacePoint)
 * (ORBmatcher.cc:977-1100, LoopClosing::SearchAndFuse): best_idx as in orbm_fuse (no reprojection
 * test); the caller sets vpReplacePoint[i] = pKF->GetMapPoint(best) when that is a good MapPoint,
 * else adds the observation (:1084-1096), in order. mp: skip = in pKF->GetMapPoints() at the call,
 * bad, pos, normal, desc, min_dist, max_dist. Scw = 4x4 row-major float Sim3. */
int orbm_fuse_sim3(orbm_ctx* ctx, const orbm_frame_view* KF, const float Scw[16], const orbm_mappoints* mp,
                   float th, int32_t* best_idx, int* nfused);

/* ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched,
 * vector<int>& vnMatches12, windowSize) (ORBmatcher.cc:405-520; Tracking::MonocularInitialization,
 * Tracking.cc:600, with ORBmatcher(0.9, true) and windowSize 100). F1: mvKeysUn octave / angle and
 * mDescriptors (n entries; x / y unused); F2: the grid side (F2.GetFeaturesInArea: x, y, octave, grid
 * bounds, angle, desc). prev_xy[2*F1.n] = vbPrevMatched (x, y), updated in place for every matched
 * keypoint; match12[F1.n] = vnMatches12; *nmatches = the reference's return value. Frames of at most
 * 8192 keypoints (ORBX_ECAPACITY above). */
int orbm_search_for_initialization(orbm_ctx* ctx, const orbm_frame_view* F1, const orbm_frame_view* F2,
                                   float* prev_xy, int window_size, float nnratio, int check_ori,
                                   int32_t* match12, int* nmatches);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1102-1326;
 * LoopClosing::ComputeSim3). KF1 / KF2: the keyframes' grid views (mvKeysUn, descriptors, bounds, grid,
 * camera: both directions project with KF1's fx, fy, cx, cy as the reference does); T1w / T2w = their
 * poses (4x4 row-major). mp1 / mp2 = pKF1 / pKF2->GetMapPointMatches(): skip = NULL entry or
 * vbAlreadyMatched1 / 2 (:1129-1142: vpMatches12[i] != NULL, and that MapPoint's index in pKF2), bad, pos,
 * desc, min_dist, max_dist (mfMinDistance / mfMaxDistance). R12 row-major 3x3, t12[3].
 * match12[mp1.n] = idx2 where both directions agree (vpMatches12[i1] = vpMapPoints2[idx2]; other entries
 * of vpMatches12 are left as they were), else -1; *nfound = the reference's return value. */
int orbm_search_by_sim3(orbm_ctx* ctx, const orbm_frame_view* KF1, const float T1w[16], const orbm_mappoints* mp1,
                        const orbm_frame_view* KF2, const float T2w[16], const orbm_mappoints* mp2, float s12,
                        const float R12[9], const float t12[3], float th, int32_t* match12, int* nfound);

/* ------------------------------------------------------------------------------------
 * Keyframe cache: a KeyFrame's descriptors, mvKeysUn (x, y, angle, octave), mvuRight and
 * FeatureVector never change after KeyFrame::ComputeBoW, but the reference's matchers read them
 * again on every call (LocalMapping::CreateNewMapPoints matches one keyframe against up to 20
 * neighbours, LocalMapping.cc:207-268; SearchInNeighbors fuses into each of them, :454-520). The
 * cache keeps them in HBM across calls and threads (thread-safe, shared by every orbm_ctx of its
 * device), keyed by a caller-chosen 64-bit key (the drop-ins use the KeyFrame's address and mnId).
 * The *_cached matchers equal their uncached forms (same arguments, same results); the views must
 * still be complete: an absent or stale entry (different N, FeatureVector size or grid geometry)
 * is uploaded from them, and the per-call MapPoint flags (has_mp, mp_bad, occupied) are always
 * taken from the view. Least-recently-used entries are evicted above capacity_bytes (0 = 1 GiB).
 * ---------------------------------------------------------------------------------- */
typedef struct orbm_kf_cache orbm_kf_cache;
int orbm_kf_cache_create(int device, size_t capacity_bytes, orbm_kf_cache** out);
void orbm_kf_cache_destroy(orbm_kf_cache* cache);
/* drop a keyframe's entries (e.g. from KeyFrame::SetBadFlag); unknown keys are ignored */
int orbm_kf_cache_erase(orbm_kf_cache* cache, uint64_t key);
int orbm_kf_cache_stats(orbm_kf_cache* cache, int* entries, size_t* bytes, long long* hits, long long* misses);
int orbm_search_for_triangulation_cached(orbm_ctx* ctx, orbm_kf_cache* cache, uint64_t key1, const orbm_kf_view* kf1,
                                         uint64_t key2, const orbm_kf_view* kf2, const float F12[9], float ex,
                                         float ey, int only_stereo, int check_ori, int32_t* match12, int* nmatches);
int orbm_search_by_bow_kf_kf_cached(orbm_ctx* ctx, orbm_kf_cache* cache, uint64_t key1, const orbm_kf_view* kf1,
                                    uint64_t key2, const orbm_kf_view* kf2, float nnratio, int check_ori,
                                    int32_t* match12, int* nmatches);
/* the Frame side is not cached (a Frame is matched once) */
int orbm_search_by_bow_kf_f_cached(orbm_ctx* ctx, orbm_kf_cache* cache, uint64_t key, const orbm_kf_view* kf,
                                   const orbm_kf_view* f, float nnratio, int check_ori, int32_t* match_f,
                                   int* nmatches);
/* the keyframe's arrays and its feature grid (AssignFeaturesToGrid) are cached */
int orbm_fuse_cached(orbm_ctx* ctx, orbm_kf_cache* cache, uint64_t key, const orbm_frame_view* KF, const float Tcw[16],
                     const float Ow[3], const orbm_mappoints* mp, float th, const float* inv_level_sigma2,
                     int32_t* best_idx, int* nfused);

/* ------------------------------------------------------------------------------------
 * MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307) for a batch of MapPoints.
 * MapPoint p's observed descriptors (the rows pKF->mDescriptors.row(idx) of its non-bad
 * observing KeyFrames, in mObservations order) are desc[offsets[p] .. offsets[p+1]) (32 B
 * each). best_idx[p] = index within that list of the descriptor with the least median
 * Hamming distance to the others (first on ties), -1 if the list is empty (mDescriptor left
 * unchanged); out_desc[p] (optional) = that descriptor.
 * ---------------------------------------------------------------------------------- */
int orbm_compute_distinctive_descriptors(orbm_ctx* ctx, int npoints, const int32_t* offsets,
                                         const uint8_t* desc, int32_t* best_idx, uint8_t* out_desc);
int orbm_compute_distinctive_descriptors_device(orbm_ctx* ctx, int npoints, const int32_t* d_offsets,
                                                const uint8_t* d_desc, int32_t* d_best_idx,
                                                uint8_t* d_out_desc, void* stream);

/* ------------------------------------------------------------------------------------
 * DBoW2 vocabulary transform -- replaces ORBVocabulary::transform(features, BowVector&,
 * FeatureVector&, levelsup) as called by Frame::ComputeBoW (Frame.cc:400-407) and
 * KeyFrame::ComputeBoW (levelsup 4), with the vocabulary loaded by loadFromTextFile
 * (System.cc:64-65). DBoW2 is not vendored in the reference: the ORB-SLAM2 fork's published
 * algorithm is restated (parity unpinned).
 * ---------------------------------------------------------------------------------- */
typedef struct orbv_handle orbv_handle;

/* ORBvoc.txt text format: "k L scoring weighting", then "parent isLeaf d0..d31 weight" per node
 * (node ids = line order, root = 0). */
int orbv_load_text(const char* path, int device, orbv_handle** out);
/* the same from arrays of the node lines (nlines nodes after the root, in file order) */
int orbv_create(int k, int L, int scoring, int weighting, int nlines, const int32_t* parent,
                const uint8_t* is_leaf, const uint8_t* desc, const double* weight, int device,
                orbv_handle** out);
void orbv_destroy(orbv_handle* h);
int orbv_info(const orbv_handle* h, int* k, int* L, int* nnodes, int* nwords);

/* n descriptors (32 B rows, n <= 4096) -> BowVector (bow_word ascending, bow_value; *nbow
 * entries) and FeatureVector as CSR (fv_node ascending, fv_off[*nfv+1], fv_feat ascending within
 * a node). Capacities: n entries each, fv_off n+1. */
int orbv_transform(orbv_handle* h, const uint8_t* desc, int n, int levelsup, uint32_t* bow_word,
                   double* bow_value, int* nbow, uint32_t* fv_node, int32_t* fv_off,
                   int32_t* fv_feat, int* nfv);
/* device batch over the frames of an orbx_extract_batch_device output (descriptors at f*kp_stride,
 * d_counts[f]; kp_stride <= 4096): per-feature word id / weight / node id at L-levelsup and per
 * frame the BowVector / FeatureVector (frame f's arrays at f*kp_stride, fv_off at
 * f*(kp_stride+1), counts d_nbow[f], d_nfv[f]). A frame's count is read as
 * min(max(d_counts[f], 0), kp_stride): a negative count is an empty frame, a count above kp_stride
 * transforms the frame's first kp_stride descriptors, and nothing is read or written outside the
 * frame's own rows. */
int orbv_transform_batch_device(orbv_handle* h, int nframes, const uint8_t* d_desc,
                                const int32_t* d_counts, int kp_stride, int levelsup,
                                int32_t* d_word, double* d_weight, uint32_t* d_nid,
                                uint32_t* d_bow_word, double* d_bow_value, int32_t* d_nbow,
                                uint32_t* d_fv_node, int32_t* d_fv_off, int32_t* d_fv_feat,
                                int32_t* d_nfv, void* stream);

/* ------------------------------------------------------------------------------------
 * Keyframe database -- the scoring half of KeyFrameDatabase (KeyFrameDatabase.cc:33-309): the
 * BowVectors of every keyframe stay resident in HBM, and one query scores a BowVector against
 * all of them, replacing the inverted-file walk (KeyFrameDatabase.cc:86-104, 207-222) and the
 * per-keyframe mpVoc->score calls (:133, :249) of DetectLoopCandidates (called by
 * LoopClosing::DetectLoop, LoopClosing.cc:143) and DetectRelocalizationCandidates (called by
 * Tracking::Relocalization, Tracking.cc:1348). Only DBoW2's L1 scoring (ORBvoc.txt's) is
 * implemented; DBoW2 is not vendored in the reference: L1Scoring::score is restated (parity
 * unpinned, as for the transform):
 *     s += (fabs(vi - wi) - fabs(vi)) - fabs(wi)   per common word, ascending word id, double
 *     score = (float)(-s / 2.0)                    (-0.0f when no word is common)
 * Entries are identified by a caller-chosen 64-bit key. Every call takes the HIP stream it is
 * ordered on (0 = the default stream); calls on one database must be ordered by the caller
 * (one stream, or events between streams). The handle's bookkeeping (key -> entry, free list,
 * insertion sequence numbers) is thread-safe.
 * ---------------------------------------------------------------------------------- */
typedef struct orbdb_handle orbdb_handle;
#define ORBDB_SCORING_L1 0 /* DBoW2::L1_NORM */
#define ORBDB_MODE_LOOP 0
#define ORBDB_MODE_RELOC 1
#define ORBDB_MAX_WORDS 4096

/* KeyFrameDatabase::KeyFrameDatabase (KeyFrameDatabase.cc:33-37): room for `capacity` keyframes
 * of at most word_stride (<= 4096) BowVector entries each. scoring other than ORBDB_SCORING_L1:
 * ORBX_EARG. The device storage is allocated by the first call that needs it (ORBX_EDEVICE there
 * when the device is unusable). */
int orbdb_create(int device, int capacity, int word_stride, int scoring, orbdb_handle** out);
void orbdb_destroy(orbdb_handle* db);
/* KeyFrameDatabase::add (KeyFrameDatabase.cc:40-46) from host arrays (word ids strictly
 * ascending, n <= word_stride, else ORBX_EARG; a key already present: ORBX_EARG; no free entry:
 * ORBX_ECAPACITY). The entry gets the next insertion sequence number. Synchronises `stream`
 * (the arrays may be released on return). */
int orbdb_add(orbdb_handle* db, uint64_t key, const uint32_t* words, const double* values, int n,
              void* stream);
/* the same from device memory (a slot's BOWWORD / BOWVALUE sections and header nbow in the
 * all-gather receive buffer, or orbv_transform_batch_device's output), no host copy. The count
 * and the word order are checked on the device: a bad input leaves an empty entry and raises the
 * error flag of orbdb_check_error; nothing is read past word_stride entries (which both arrays
 * must hold when the count is not trusted). */
int orbdb_add_device(orbdb_handle* db, uint64_t key, const uint32_t* d_words, const double* d_values,
                     const int32_t* d_count, void* stream);
/* KeyFrameDatabase::erase (KeyFrameDatabase.cc:48-67; unknown keys are ignored) and clear
 * (:69-73), ordered on `stream` against the queries queued before them */
int orbdb_erase(orbdb_handle* db, uint64_t key, void* stream);
int orbdb_clear(orbdb_handle* db, void* stream);
/* the live entries in insertion order: keys[i], entry index slots[i] (either may be NULL);
 * *n = their number (ORBX_ECAPACITY if cap is smaller) */
int orbdb_entries(orbdb_handle* db, int cap, uint64_t* keys, int32_t* slots, int* n);
/* nq queries against every entry, enqueued on `stream`. Query q's word ids are at d_words +
 * q * word_stride_bytes (uint32, ascending), its values at d_values + q * value_stride_bytes
 * (double), its count at d_counts + q * count_stride_bytes (int32; more than 4096: error flag,
 * scored as empty) -- so the slots of a receive buffer or the rows of a transform batch are
 * queried in place. Outputs at [q * capacity + entry index]: d_ncommon (mnLoopWords /
 * mnRelocWords, KeyFrameDatabase.cc:102, :220; -1 for an entry that is not live), d_score
 * (mpVoc->score, :133, :249) and d_first_word (the smallest common word id, which orders
 * lKFsSharingWords, :99, :218; 0xFFFFFFFF if none). */
int orbdb_query_device(orbdb_handle* db, int nq, const void* d_words, size_t word_stride_bytes,
                       const void* d_values, size_t value_stride_bytes, const void* d_counts,
                       size_t count_stride_bytes, int32_t* d_ncommon, float* d_score,
                       uint32_t* d_first_word, void* stream);
/* one host query (n <= 4096): uploads it, queries, synchronises `stream` and returns the live
 * entries in insertion order (*nout of them; ORBX_ECAPACITY if cap is smaller) */
int orbdb_query(orbdb_handle* db, const uint32_t* words, const double* values, int n, int cap,
                uint64_t* keys, int32_t* ncommon, float* score, uint32_t* first_word, int* nout,
                void* stream);
/* reads and clears the device error flag (synchronises `stream`): ORBX_EDEVICE if a device add
 * or query since the last call rejected its input */
int orbdb_check_error(orbdb_handle* db, void* stream);
/* The candidate selection of DetectLoopCandidates (KeyFrameDatabase.cc:107-196, mode
 * ORBDB_MODE_LOOP) and DetectRelocalizationCandidates (:224-308, ORBDB_MODE_RELOC) over the n
 * entries of a query, in insertion order. Host only, no device. connected[i] != 0 (loop mode;
 * NULL = none): entry i is in pKF->GetConnectedKeyFrames(). Entry i's
 * GetBestCovisibilityKeyFrames(10) are neigh[neigh_off[i] .. neigh_off[i+1]) as entry indices in
 * best-covisibility order, -1 for a keyframe that is not in the database. last_score[i] is the
 * persistent mLoopScore / mRelocScore: written only for the entries the reference scores
 * (ncommon > minCommonWords), read for the neighbours (in reloc mode also for neighbours that
 * were not scored by this call, as the reference does). out_idx (n entries) receives the
 * candidates' entry indices in the reference's order, *nout their number. */
int orbdb_select_candidates(int mode, int n, const int32_t* ncommon, const float* score,
                            const uint32_t* first_word, const uint8_t* connected,
                            const int32_t* neigh_off, const int32_t* neigh, float min_score,
                            float* last_score, int32_t* out_idx, int* nout);

/* ------------------------------------------------------------------------------------
 * Cross-agent keyframe slot -- replaces the LCM message lcmKeyFrame::lcmKeyFrameInfo
 * (ORB_SLAM2.1/include/lcmKeyFrame/lcmKeyFrameInfo.hpp:24-150), published by the sending
 * agent (ORB_SLAM2.1/Examples/ROS/ORB_SLAM2/src/ros_mono.cc:1907-2410) and decoded into
 * receiveKeyframeInfo by the receiving one (ORB_SLAM2/Examples/ROS/ORB_SLAM2/src/
 * ros_mono.cc:88-166, 230-544) for Tracking::CreateNewKeyFrame (:2108-2192). One slot is a
 * fixed-size, self-describing byte block (so an RCCL all-gather of equal-sized slots is the
 * whole transport):
 *   [0, 128)      orbx_slot_header (magic, version, counts, section offsets)
 *   [128, 832)    orbx_kf_meta     (every scalar / matrix field of lcmKeyFrameInfo)
 *   [1024, ...)   sections, each 256-byte aligned, sized by the capacity `cap`:
 *     KPS      cap x orbx_kp        mvKeys (float coordinates; LCM truncated them to int16,
 *                                   lcmKeyPoint.hpp:19-24)
 *     KUN      cap x float[2]       mvKeysUn[i].pt (size/angle/octave equal mvKeys')
 *     URIGHT   cap x float          mvuRight (-1 = monocular)
 *     DEPTH    cap x float          mvDepth
 *     DESC     cap x 32 B           mDescriptors (bytes; LCM sent them as float rows)
 *     MPFLAGS  cap x u8             bit 0: mvpMapPoints[i] != NULL  (lcmKeyFrameMapPoints
 *                                   .ifMapPoints), bit 1: that MapPoint isBad()
 *     MPPOS    cap x float[3]       its world position (poseX/Y/Z)
 *     BOWWORD  cap x u32, BOWVALUE cap x f64   mBowVec (ascending word id), nbow entries
 *     FVNODE   cap x u32, FVOFF (cap+1) x i32, FVFEAT cap x i32   mFeatVec as CSR, nfv nodes
 * Entries past n (nbow, nfv) are zero. All-little-endian, no pointers.
 * ---------------------------------------------------------------------------------- */
#define ORBX_SLOT_MAGIC 0x4B42524Fu /* "ORBK" */
#define ORBX_SLOT_VERSION 2
enum {
    ORBX_SLOT_KPS = 0, ORBX_SLOT_KUN, ORBX_SLOT_URIGHT, ORBX_SLOT_DEPTH, ORBX_SLOT_DESC,
    ORBX_SLOT_MPFLAGS, ORBX_SLOT_MPPOS, ORBX_SLOT_BOWWORD, ORBX_SLOT_BOWVALUE, ORBX_SLOT_FVNODE,
    ORBX_SLOT_FVOFF, ORBX_SLOT_FVFEAT, ORBX_SLOT_NSECTIONS
};
/* header.flags: which optional fields the sender filled (the rest hold their defaults) */
#define ORBX_SLOT_F_KUN 1u     /* mvKeysUn differs from mvKeys (else KUN = mvKeys' pt)   */
#define ORBX_SLOT_F_STEREO 2u  /* mvuRight / mvDepth present (else -1)                   */
#define ORBX_SLOT_F_MP 4u      /* MapPoint records present (else none)                   */
#define ORBX_SLOT_F_BOW 8u     /* BowVector present                                      */
#define ORBX_SLOT_F_FV 16u     /* FeatureVector present                                  */

typedef struct orbx_slot_header {
    uint32_t magic, version;
    int32_t n;        /* N (keypoints)                                                    */
    int32_t cap;      /* capacity the section sizes were computed for                     */
    int32_t nbow;     /* BowVector entries                                                */
    int32_t nfv;      /* FeatureVector nodes                                              */
    uint32_t flags;   /* ORBX_SLOT_F_*                                                    */
    uint32_t bytes;   /* orbx_slot_bytes(cap)                                             */
    uint32_t off[ORBX_SLOT_NSECTIONS]; /* byte offset of each section                    */
    uint32_t reserved[12];
} orbx_slot_header; /* 128 bytes */

/* The scalar and matrix fields of lcmKeyFrameInfo (lcmKeyFrameInfo.hpp:24-100), grouped by
 * type; 4x4 / 3x3 matrices row-major (cv::Mat::at<float>(r,c)). 704 bytes. */
typedef struct orbx_kf_meta {
    int64_t nNextId, mnId, mnFrameId, mnGridCols, mnGridRows, mnTrackReferenceForFrame,
        mnFuseTargetForKF, mnBALocalForKF, mnBAFixedForKF, mnLoopQuery, mnLoopWords, mnRelocQuery,
        mnRelocWords, mnBAGlobalForKF, mnMinX, mnMinY, mnMaxX, mnMaxY;
    double mTimeStamp;
    int32_t agent;          /* sending agent (rank); not in the LCM message              */
    int32_t mnScaleLevels;
    float mfGridElementWidthInv, mfGridElementHeightInv, mLoopScore, mRelocScore;
    float fx, fy, cx, cy, invfx, invfy, mbf, mb, mThDepth;
    float mfScaleFactor, mfLogScaleFactor;
    float mvScaleFactors[16], mvLevelSigma2[16], mvInvLevelSigma2[16];
    float mK[9];
    float mTcw[16], mTcwGBA[16], mTcwBefGBA[16], mTcp[16];
} orbx_kf_meta;

/* One keyframe's per-feature arrays (device memory for the *_device calls, host memory for
 * orbx_pack_keyframe_host). count -> N. Optional arrays may be NULL (see ORBX_SLOT_F_*):
 * kun (n x 2 floats), uright + depth, mp_flags (+ mp_pos n x 3), bow_word + bow_value + nbow,
 * fv_node + fv_off + fv_feat + nfv. */
typedef struct orbx_kf_source {
    const orbx_kp* kps;
    const uint8_t* desc;
    const int32_t* count;
    const float* kun;
    const float* uright;
    const float* depth;
    const uint8_t* mp_flags;
    const float* mp_pos;
    const uint32_t* bow_word;
    const double* bow_value;
    const int32_t* nbow;
    const uint32_t* fv_node;
    const int32_t* fv_off;
    const int32_t* fv_feat;
    const int32_t* nfv;
} orbx_kf_source;

/* Fixed slot size for capacity cap (and the header with the section offsets, hdr optional). */
size_t orbx_slot_bytes(int cap);
int orbx_slot_layout(int cap, orbx_slot_header* hdr);

/* Pack one keyframe (device arrays, e.g. an orbx_extract_batch_device frame + its
 * orbv_transform_batch_device BoW) into d_slot (orbx_slot_bytes(cap) bytes), enqueued on
 * `stream`. Counts above cap are clamped to cap and raise bit 0 of *d_err (optional device int). */
int orbx_pack_keyframe_device(const orbx_kf_source* src, const orbx_kf_meta* meta, int cap,
                              uint8_t* d_slot, int32_t* d_err, void* stream);
/* The same from host arrays into a host slot (byte-identical to the device pack). ORBX_ECAPACITY
 * if a count exceeds cap. */
int orbx_pack_keyframe_host(const orbx_kf_source* src, const orbx_kf_meta* meta, int cap,
                            uint8_t* slot, size_t slot_bytes);

/* A validated view of a received slot in host memory: magic/version, cap vs slot_bytes, every
 * section offset, n/nbow/nfv <= cap, the FeatureVector CSR (offsets monotone, node ids and word
 * ids strictly ascending, feature indices < n and ascending within a node). ORBX_EARG if any
 * check fails. Pointers alias `slot`. */
typedef struct orbx_slot_view {
    const orbx_slot_header* hdr;
    const orbx_kf_meta* meta;
    const orbx_kp* kps;
    const float* kun;
    const float* uright;
    const float* depth;
    const uint8_t* desc;
    const uint8_t* mp_flags;
    const float* mp_pos;
    const uint32_t* bow_word;
    const double* bow_value;
    const uint32_t* fv_node;
    const int32_t* fv_off;
    const int32_t* fv_feat;
} orbx_slot_view;
int orbx_slot_parse(const uint8_t* slot, size_t slot_bytes, orbx_slot_view* out);

/* Geometry of one (query keyframe, slot keyframe) pair: F12 (LocalMapping::ComputeF12,
 * LocalMapping.cc:536-553) and the epipole (ex, ey) of the query's centre in the slot's
 * keyframe (ORBmatcher.cc:664-670). */
typedef struct orbm_slot_geom {
    float F12[9];
    float ex, ey;
} orbm_slot_geom;

/* Cross-agent ORBmatcher::SearchForTriangulation(query KF, slot KF, F12, vMatchedPairs,
 * bOnlyStereo = false) (ORBmatcher.cc:657-823) of this agent's keyframe (`query`, device
 * arrays: kps/desc/count, optional kun, uright, mp_flags and, with use_bow, its FeatureVector)
 * against nref received slots at d_slots + r*slot_bytes (e.g. the all-gather receive buffer),
 * straight from device memory. Per slot: geom[r] (host array), the slot keyframe's
 * mvScaleFactors / mvLevelSigma2 from its meta, its mvKeysUn / mvuRight / MapPoint flags.
 * use_bow = 0: one node holding every feature (brute force, the BASELINE configuration);
 * use_bow = 1: the common nodes of the two FeatureVectors (query nodes <= max_nodes).
 * Outputs d_match[r*cap1 + idx1] (idx2 or -1), d_nmatches[r]. A slot that fails validation
 * (magic, version, size, counts, CSR bounds) contributes no matches and raises the ctx's
 * device error flag (orbm_check_error). */
int orbm_search_for_triangulation_slots_device(orbm_ctx* ctx, const orbx_kf_source* query, int cap1,
                                               int nref, const uint8_t* d_slots, size_t slot_bytes,
                                               const orbm_slot_geom* geom, int use_bow, int max_nodes,
                                               int32_t* d_match, int32_t* d_nmatches, void* stream);

/* Cross-agent ORBmatcher::SearchByBoW(query KF, slot KF, vpMatches12) (ORBmatcher.cc:522-655):
 * the loop-candidate match the receiving agent runs on a received keyframe (it goes to
 * LoopClosing::InsertKeyFrame, ORB_SLAM2/Examples/ROS/ORB_SLAM2/src/ros_mono.cc:3530, and
 * LoopClosing::ComputeSim3 calls SearchByBoW(mpCurrentKF, pKF) with ORBmatcher(0.75, true),
 * LoopClosing.cc:239, 265), of this agent's keyframe (`query`, device arrays: kps/desc/count,
 * mp_flags (bit 0 a MapPoint, bit 1 bad; NULL = none) and its FeatureVector) against nref
 * received slots at d_slots + r*slot_bytes, straight from device memory, over the common nodes
 * of the two FeatureVectors (query nodes <= max_nodes). Outputs d_match[r*cap1 + idx1] = the
 * slot keyframe's feature idx2 whose MapPoint vpMatches12[idx1] is (or -1), after the
 * rotation filter when check_ori, and d_nmatches[r]. A slot that fails validation contributes
 * no matches and raises the ctx's device error flag (orbm_check_error). Slots may carry a
 * larger capacity than the query (agents with other feature counts): a common node is matched
 * whole up to 4551 candidates (one CU's LDS); a node past that raises the error flag. */
int orbm_search_by_bow_slots_device(orbm_ctx* ctx, const orbx_kf_source* query, int cap1, int nref,
                                    const uint8_t* d_slots, size_t slot_bytes, float nnratio, int check_ori,
                                    int max_nodes, int32_t* d_match, int32_t* d_nmatches, void* stream);

/* ------------------------------------------------------------------------------------
 * Cross-agent collective -- replaces the LCM keyframe publish / subscribe between the agents
 * (ORB_SLAM2.1/Examples/ROS/ORB_SLAM2/src/ros_mono.cc:2399, ORB_SLAM2/Examples/ROS/ORB_SLAM2/
 * src/ros_mono.cc:602): one RCCL all-gather over xGMI of every agent's keyframe slot
 * (orbx_pack_keyframe_device), enqueued on the caller's stream (no collective-owned stream), one
 * process = one agent = one GPU. RCCL is bound at run time (the process's librccl.so.1 if one
 * is loaded, else ROCm's); ORBX_EDEVICE without it.
 * ---------------------------------------------------------------------------------- */
#define ORBX_COMM_ID_BYTES 128
typedef struct orbx_comm orbx_comm;
/* rank 0 creates the id (ncclGetUniqueId); the caller hands it to every rank (any transport) */
int orbx_comm_unique_id(uint8_t* id);
/* collective over the world: every rank calls it with the same id, its rank and its device */
int orbx_comm_create(const uint8_t* id, int world, int rank, int device, orbx_comm** out);
/* d_recv[r*bytes .. (r+1)*bytes) = rank r's d_send[0 .. bytes), on `stream` (ncclAllGather, uint8) */
int orbx_comm_allgather(orbx_comm* c, const void* d_send, void* d_recv, size_t bytes, void* stream);
void orbx_comm_destroy(orbx_comm* c);

/* ------------------------------------------------------------------------------------
 * Stereo -- replaces Frame::ComputeStereoMatches (ORB_SLAM2.1/src/Frame.cc:470-641, the
 * stereo Frame constructor's step after ExtractORB(0/1), Frame.cc:80-98), reading the two
 * extractors' pyramids (mpORBextractorLeft/Right->mvImagePyramid) where they already live.
 * mvScaleFactors / mvInvScaleFactors come from `left`; both handles must have the same
 * frame size and ORB parameters. bf = mbf, b = mb (Frame.cc:501-503).
 * ---------------------------------------------------------------------------------- */

/* Host form: kpsL/descL (mvKeys, mDescriptors) and kpsR/descR (mvKeysRight,
 * mDescriptorsRight) are the outputs of the latest orbx_extract on `left` and `right`
 * (two distinct handles, like the two ORBextractor instances). Writes mvuRight and
 * mvDepth (nL floats, -1 = no stereo match) and the number of stereo matches kept.
 * ORBX_EARG where the reference would throw (an 11x11 correlation window outside the level:
 * cv::Mat::rowRange/colRange assert). */
int orbx_compute_stereo_matches(orbx_handle* left, orbx_handle* right, const orbx_kp* kpsL,
                                const uint8_t* descL, int nL, const orbx_kp* kpsR,
                                const uint8_t* descR, int nR, float bf, float b, float* uright,
                                float* depth, int* nstereo);

/* Device batch form: pair p = frame d_fl[p] of the latest orbx_extract_batch_device on
 * `left` with frame d_fr[p] of the latest one on `right` (left == right allowed, e.g. a
 * batch holding left and right images). Keypoints/descriptors/counts as produced by those
 * extractions (frame f at f*kp_stride). Outputs: d_uright/d_depth[p*kp_stride + i],
 * d_nstereo[p]. A window outside the level sets the device error flag (orbx_check_error on
 * `left`). Enqueued on `stream` after both extractions (the caller orders the streams). */
int orbx_stereo_matches_batch_device(orbx_handle* left, orbx_handle* right, int npairs,
                                     const int32_t* d_fl, const int32_t* d_fr,
                                     const orbx_kp* d_kpsL, const uint8_t* d_descL,
                                     const int32_t* d_cntL, const orbx_kp* d_kpsR,
                                     const uint8_t* d_descR, const int32_t* d_cntR, int kp_stride,
                                     float bf, float b, float* d_uright, float* d_depth,
                                     int32_t* d_nstereo, void* stream);

/* ------------------------------------------------------------------------------------
 * Undistorted keypoints -- replaces Frame::UndistortKeyPoints (ORB_SLAM2/src/Frame.cc:405-435)
 * and Frame::ComputeImageBounds (Frame.cc:437-465) with the grid cell sizes derived from the
 * bounds (Frame.cc:213-214). cv::undistortPoints(src, dst, K, D, noArray(), K) of OpenCV 3.x is
 * restated from its published algorithm (parity unpinned; DESIGN.md "Pinned semantics"): five
 * fixed-point iterations in double, no convergence test, then the projection with P = mK, one
 * rounding to float. The reference's quirk stays: mDistCoef.at<float>(0) == 0.0 (k1 alone)
 * means mvKeysUn = mvKeys and bounds (0, cols, 0, rows), whatever k2, p1, p2, k3 are.
 * ---------------------------------------------------------------------------------- */

/* The float members of mK (fx, fy, cx, cy) and mDistCoef (k1, k2, p1, p2[, k3]) as Tracking reads
 * them from the settings file (Tracking.cc:54-77); k3 = 0 for a 4-entry mDistCoef. */
typedef struct orbx_camera {
    float fx, fy, cx, cy, k1, k2, p1, p2, k3;
} orbx_camera;

/* The cv::undistortPoints call of Frame::UndistortKeyPoints (Frame.cc:423) over n points
 * (xy_in / xy_out: n x 2 floats; in place allowed), with the k1 == 0 copy of Frame.cc:407-411.
 * Host only, no device. ORBX_EARG on NULL arguments, n < 0 or fx == 0 || fy == 0 (here and in the
 * two calls below). */
int orbx_undistort_points(const orbx_camera* cam, int n, const float* xy_in, float* xy_out);
/* Frame::UndistortKeyPoints (Frame.cc:405-435): out[i] = in[i] with only (x, y) replaced
 * (Frame.cc:430-433); in place allowed. Host only. */
int orbx_undistort_keypoints(const orbx_camera* cam, int n, const orbx_kp* in, orbx_kp* out);
/* Frame::ComputeImageBounds (Frame.cc:437-465) of a cols x rows image: bounds = {mnMinX, mnMaxX,
 * mnMinY, mnMaxY}; grid_w_inv / grid_h_inv (either may be NULL) = mfGridElementWidthInv /
 * mfGridElementHeightInv = 64.0f / (mnMaxX - mnMinX), 48.0f / (mnMaxY - mnMinY) in float
 * (Frame.cc:213-214). Host only. */
int orbx_image_bounds(const orbx_camera* cam, int cols, int rows, float bounds[4], float* grid_w_inv,
                      float* grid_h_inv);
/* Frame::UndistortKeyPoints (Frame.cc:405-435) for every frame of an orbx_extract_batch_device
 * output (d_kps / d_counts / kp_stride as produced there), on the device: d_kps_un (a full
 * orbx_kp array of the same layout; may equal d_kps) receives mvKeysUn and, when d_kun is not
 * NULL, d_kun[(f*kp_stride + i)*2 .. +2) its (x, y) alone (orbx_kf_source::kun of frame f at
 * d_kun + f*kp_stride*2). Only rows i < min(d_counts[f], kp_stride) are read or written. The
 * arrays must be 8-byte aligned (ORBX_EARG otherwise). Enqueued on `stream`; no host sync. */
int orbx_undistort_batch_device(orbx_handle* h, const orbx_camera* cam, int nframes, const orbx_kp* d_kps,
                                const int32_t* d_counts, int kp_stride, orbx_kp* d_kps_un, float* d_kun,
                                void* stream);

/* The one-frame path: with a camera set (cam = NULL: off, the default) every subsequent orbx_extract on
 * `h` also delivers Frame::UndistortKeyPoints (Frame.cc:405-435) of its keypoints, from one more
 * kernel node of its captured graph into the handle's pinned memory, and orbx_last_keypoints_un copies
 * them out after the call (kps_un[cap]; *n = their number, the call's keypoint count). ORBX_EARG when
 * the last orbx_extract had no camera, was stage-profiled (orbx_profile_enable) or delivered nothing
 * (empty image, error); ORBX_ECAPACITY if cap is smaller. Without a camera orbx_extract is unchanged. */
int orbx_set_camera(orbx_handle* h, const orbx_camera* cam);
int orbx_last_keypoints_un(orbx_handle* h, orbx_kp* kps_un, int cap, int* n);

/* ------------------------------------------------------------------------------------
 * Frame-to-frame tracking on a device batch: Frame::UnprojectStereo (ORB_SLAM2/src/Frame.cc:
 * 667-681) and ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
 * (ORBmatcher.cc:1328-1470) as Tracking::TrackWithMotionModel calls it (Tracking.cc:869-900),
 * over frames that already sit in HBM.
 * ---------------------------------------------------------------------------------- */

/* Frame::UnprojectStereo (Frame.cc:667-681) of keypoints 0..n-1 of one frame on the host:
 * pos[3 i .. +3) = mRwc * x3Dc + mOw with x3Dc = ((u - cx) z invfx, (v - cy) z invfy, z), (u, v) =
 * kps_un[i] (mvKeysUn), z = depth[i] (mvDepth), invfx = 1.0f / fx (Frame.cc:104-105), mRwc = mRcw.t()
 * and mOw = -mRcw.t() * mtcw of Tcw (mTcw, 4x4 row-major; Frame.cc:261-267), in cv::Mat's float
 * arithmetic (DESIGN.md "Pinned semantics"). z <= 0 (the reference returns cv::Mat()): three zeros,
 * valid[i] = 0; otherwise valid[i] = 1 (valid may be NULL). Only fx, fy, cx, cy of cam are read.
 * Host only, no device. ORBX_EARG on NULL arguments, n < 0 or fx == 0 || fy == 0, before anything
 * is written. */
int orbx_unproject_stereo(const orbx_camera* cam, const float Tcw[16], int n, const orbx_kp* kps_un,
                          const float* depth, float* pos, uint8_t* valid);

/* The same for every frame of a device batch: frame f's keypoints, depths and outputs at
 * f*kp_stride (d_kps_un: orbx_undistort_batch_device's output or, without distortion, the
 * extractor's; d_depth: orbx_stereo_matches_batch_device's), its count d_counts[f] (clamped to
 * kp_stride) and its pose d_Tcw[16 f .. +16); mOw is derived per frame on the device, so a captured
 * graph can be replayed with new poses. Rows i >= d_counts[f] are not written. With d_mp_flags (not
 * NULL) row i also gets valid_flags for z > 0 and 0 otherwise: the flags
 * orbm_search_by_projection_last_frame_batch_device reads. Bit-identical to the host form. d_kps_un
 * must be 8-byte aligned, nframes <= 65535. Enqueued on `stream`; no host sync. */
int orbx_unproject_stereo_batch_device(orbx_handle* h, const orbx_camera* cam, int nframes,
                                       const orbx_kp* d_kps_un, const float* d_depth,
                                       const int32_t* d_counts, int kp_stride, const float* d_Tcw,
                                       float* d_pos, uint8_t* d_mp_flags, int valid_flags,
                                       void* stream);

/* The Frame fields SearchByProjection(CurrentFrame, LastFrame, ...) reads, one set per launch. */
typedef struct orbm_track_geom {
    float fx, fy, cx, cy, bf, b;                                /* camera, mbf, mb                */
    float min_x, min_y, max_x, max_y, grid_w_inv, grid_h_inv;   /* orbx_image_bounds              */
    int32_t nlevels;                                            /* mnScaleLevels, 1..16           */
    float scale_factors[16];                                    /* mvScaleFactors                 */
} orbm_track_geom;

/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1328-1470) for
 * npairs frame pairs of one device batch: pair p is the reference call with CurrentFrame = frame
 * d_cur[p] and LastFrame = frame d_last[p]. Per frame f (everything at f*kp_stride, count
 * d_counts[f]): d_kps_un = mvKeysUn, d_desc = mDescriptors, d_uright = mvuRight (NULL = monocular,
 * all -1), d_occupied[i] != 0 = CurrentFrame.mvpMapPoints[i] with Observations() > 0 before the call
 * (NULL = none, as after Tracking.cc:879), d_pos = the world position of feature i's MapPoint
 * (n x 3), d_Tcw[16 f .. +16) = mTcw (row-major), and d_mp_flags of feature i:
 *   bit 0  the feature has a MapPoint (as in orbm_search_by_bow_batch_device);
 *   bit 1  that MapPoint is bad: the reference does not test it here, ignored;
 *   bit 2  LastFrame.mvbOutlier[i];
 *   bit 3  Observations() > 0: a match occupies the feature for the queries after it.
 * Feature i of the last frame is a query iff bit 0 is set and bit 2 is clear (ORBmatcher.cc:1355-
 * 1359); its octave and angle are d_kps_un's, its descriptor its d_desc row. A device prologue does
 * the per-MapPoint geometry of ORBmatcher.cc:1339-1405 with the per-call entry's float semantics
 * and fills one search call per pair in the ctx's scratch; the grid, scan and in-order resolve
 * kernels of the per-call entry then run once each over all pairs.
 * Output as for every variant: d_match[p*kp_stride + i], i < d_counts[d_cur[p]], = the last-frame
 * feature index, -1 or -2; d_nmatches[p] = the reference's return value.
 * Validation on the device: a current frame's count is clamped to kp_stride; a pair with a frame
 * index outside [0, nframes), a last-frame count above kp_stride or an accepted feature whose
 * octave is outside [0, nlevels) raises the ctx's error flag (orbm_check_error), gets nmatches = 0
 * and -1 in its whole d_match row, and reads nothing out of range; the other pairs are unaffected.
 * ORBX_EARG for NULL arguments, npairs < 0, nframes < 1, kp_stride outside [1, 65536], nlevels
 * outside [1, 16] or d_kps_un / d_desc not 8- / 16-byte aligned; npairs == 0 (with a valid ctx, geom
 * and sizes; the arrays may then be NULL) is a no-op that returns 0.
 * The call only enqueues on `stream` (no upload, no host wait); the ctx's scratch grows at the first
 * call of a larger npairs x kp_stride (an allocation: not inside a stream capture). One ctx serves
 * one stream at a time. */
int orbm_search_by_projection_last_frame_batch_device(
    orbm_ctx* ctx, int npairs, const int32_t* d_cur, const int32_t* d_last, int nframes,
    const orbx_kp* d_kps_un, const uint8_t* d_desc, const int32_t* d_counts, int kp_stride,
    const float* d_uright, const uint8_t* d_occupied, const float* d_pos, const uint8_t* d_mp_flags,
    const float* d_Tcw, const orbm_track_geom* geom, float th, int mono, int check_ori,
    int32_t* d_match, int32_t* d_nmatches, void* stream);

/* ------------------------------------------------------------------------------------
 * Local-map tracking on a device batch: Frame::isInFrustum (Frame.cc:274-330, with
 * MapPoint::PredictScale, MapPoint.cc:385-417) and Tracking::SearchLocalPoints
 * (Tracking.cc:1143-1193) with its ORBmatcher::SearchByProjection(F, vpMapPoints, th)
 * (ORBmatcher.cc:45-129), as Tracking::TrackLocalMap runs them on every frame.
 * ---------------------------------------------------------------------------------- */

/* Frame::isInFrustum(pMP, viewingCosLimit) of n MapPoints on the host, under the pose Tcw (mTcw, 4x4
 * row-major). Of geom: fx, fy, cx, cy, bf, the bounds and nlevels are read; log_scale_factor =
 * mfLogScaleFactor. Per point: pos (GetWorldPos, n x 3), normal (GetNormal, n x 3), min_dist / max_dist =
 * the raw mfMinDistance / mfMaxDistance (the 0.8f / 1.2f of Get*DistanceInvariance are applied here).
 * Outputs, the six tracking arrays of orbm_mappoints: in_view = mbTrackInView, proj_x / proj_y /
 * proj_xr = mTrackProjX / Y / XR, level = mnTrackScaleLevel, view_cos = mTrackViewCos; a rejected point
 * gets in_view = 0 and zeros. The float sequence, in cv::Mat's arithmetic (DESIGN.md "Pinned semantics"):
 *   Pc = mRcw * P + mtcw (small-matrix gemm); PcZ < 0.0f rejects; invz = 1.0f / PcZ (a float divide);
 *   u = fx * PcX * invz + cx, v = fy * PcY * invz + cy (float, left to right);
 *   u < min_x || u > max_x || v < min_y || v > max_y rejects;
 *   mOw = -mRcw.t() * mtcw (GEMM_1_T, double accumulation); PO = P - mOw (float);
 *   dist = (float)sqrt(sum (double)PO^2); dist < 0.8f * min_dist || dist > 1.2f * max_dist rejects;
 *   viewCos = (float)(dot_double(PO, Pn) / (double)dist); viewCos < viewing_cos_limit rejects;
 *   ratio = max_dist / dist; level = ceilf(logf(ratio) / log_scale_factor) (a float divide, glibc's
 *   logf) clamped to [0, nlevels - 1]; proj_xr = u - bf * invz.
 * Contract: where the reference's behaviour is undefined or meaningless the point is rejected -- a
 * non-finite pose entry or point field, a non-finite Pc, u, v, dist or viewCos, PcZ == +-0, dist == 0,
 * a ratio that is not a positive normal float.
 * Host only, no device. ORBX_EARG on NULL arguments, n < 0, nlevels outside [1, 16], a
 * log_scale_factor that is not finite and > 0 or a non-finite limit, before anything is written. */
int orbx_is_in_frustum(const orbm_track_geom* geom, float log_scale_factor, const float Tcw[16],
                       float viewing_cos_limit, int n, const float* pos, const float* normal,
                       const float* min_dist, const float* max_dist, uint8_t* in_view, float* proj_x,
                       float* proj_y, float* proj_xr, int32_t* level, float* view_cos);

/* The same for a device table of M points under nframes poses d_Tcw[16 f .. +16) (the layout
 * orbx_unproject_stereo_batch_device reads): every output at f*M + m. Bit-identical to the host form. A
 * point the contract excludes also raises the ctx's device error flag (orbm_check_error). M == 0 or
 * nframes == 0 is a no-op; nframes <= 65535. Enqueued on `stream`; no host sync, no scratch. */
int orbx_is_in_frustum_batch_device(orbm_ctx* ctx, const orbm_track_geom* geom, float log_scale_factor,
                                    float viewing_cos_limit, int M, const float* d_pos,
                                    const float* d_normal, const float* d_min_dist,
                                    const float* d_max_dist, int nframes, const float* d_Tcw,
                                    uint8_t* d_in_view, float* d_proj_x, float* d_proj_y,
                                    float* d_proj_xr, int32_t* d_level, float* d_view_cos, void* stream);

/* Tracking::SearchLocalPoints (Tracking.cc:1143-1193) for every frame of a device batch. The frame
 * arrays are those of orbm_search_by_projection_last_frame_batch_device (d_kps_un, d_desc, d_counts,
 * kp_stride, d_uright or NULL, d_Tcw, geom); log_scale_factor = mfLogScaleFactor. The local map is a
 * table of M MapPoints: d_pos, d_normal (M x 3), d_min_dist, d_max_dist (raw, as above), d_mp_desc
 * (M x 32, 16-byte aligned) and d_mp_flags with the bits' usual meaning (bit 1 isBad(), bit 3
 * Observations() > 0, the others ignored). Frame f's mvpLocalMapPoints is the slice
 * [d_range[2f], d_range[2f+1]) of the table (d_range NULL: the whole table), so the maps of several
 * agents or windows can share one table. d_frame_mp[f*kp_stride + i] = the table index of feature i's
 * MapPoint (mCurrentFrame.mvpMapPoints, e.g. from the last-frame search's match row) or negative.
 * Per frame, on the device:
 *   - the first loop (:1146-1162): a feature whose MapPoint is bad counts as having none; any other
 *     MapPoint is marked seen for this frame (mnLastFrameSeen) and occupies its feature iff bit 3 is set
 *     (ORBmatcher.cc:87-89);
 *   - the second loop (:1167-1180): every point of the slice that is neither seen nor bad goes through
 *     isInFrustum(pMP, viewing_cos_limit) exactly as orbx_is_in_frustum states it; d_ntomatch[f] =
 *     nToMatch; d_in_view[f*M + m] (optional) = 1 where it returned true, 0 elsewhere (the host's
 *     IncreaseVisible);
 *   - SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:45-129): radius = RadiusByViewingCos
 *     (> 0.998: 2.5f, else 4.0f), times th when th != 1.0, times mvScaleFactors[level]; levels
 *     [level - 1, level]; the mvuRight test; TH_HIGH = 100; the ratio test with nnratio; a match
 *     occupies its feature iff the point's bit 3 is set. Rejected points stay in place as queries with
 *     an empty window, so the in-order claim resolution sees the points in table order.
 * Output as for every variant: d_match[f*kp_stride + i], i < d_counts[f], = the table index or -1
 * (rows past the count are not written); d_nmatches[f] = the reference's return value. A frame with
 * nToMatch == 0 gets nmatches = 0 and an all -1 row.
 * Validation on the device: a count above kp_stride is clamped; a d_frame_mp index >= M raises the
 * ctx's error flag (orbm_check_error) and is treated as none; a d_range pair outside [0, M] or with
 * begin > end raises the flag, and that frame alone gets nmatches = ntomatch = 0 and -1 in its whole
 * d_match row; a point or pose the isInFrustum contract excludes raises the flag and is rejected.
 * ORBX_EARG for NULL arguments (the table's arrays may be NULL when M == 0), nframes < 0, M < 0,
 * kp_stride outside [1, 65536], nlevels outside [1, 16], a log_scale_factor that is not finite and > 0,
 * a non-finite limit, or d_kps_un / d_desc / d_mp_desc not 8- / 16- / 16-byte aligned; nframes == 0 is a
 * no-op that returns 0. The call only enqueues on `stream` (no upload, no host wait); the ctx's scratch
 * grows at the first call of a larger nframes x (kp_stride, M) (an allocation: not inside a stream
 * capture). One ctx serves one stream at a time. */
int orbm_search_local_points_batch_device(
    orbm_ctx* ctx, int nframes, const orbx_kp* d_kps_un, const uint8_t* d_desc, const int32_t* d_counts,
    int kp_stride, const float* d_uright, const float* d_Tcw, const orbm_track_geom* geom,
    float log_scale_factor, int M, const float* d_pos, const float* d_normal, const float* d_min_dist,
    const float* d_max_dist, const uint8_t* d_mp_desc, const uint8_t* d_mp_flags, const int32_t* d_range,
    const int32_t* d_frame_mp, float th, float nnratio, float viewing_cos_limit, int32_t* d_match,
    int32_t* d_nmatches, int32_t* d_ntomatch, uint8_t* d_in_view, void* stream);

/* ------------------------------------------------------------------------------------
 * New MapPoints from triangulation matches: the per-match body of
 * LocalMapping::CreateNewMapPoints (LocalMapping.cc:284-450) with its per-pair baseline test
 * (:244-261) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:330-371) of the new point's two
 * observations. Input: the match row of a SearchForTriangulation variant; output: a table of
 * MapPoints in the row format orbm_search_local_points_batch_device reads.
 * ---------------------------------------------------------------------------------- */

/* What the loop reads of the two keyframes, one set per call. BOTH keyframes use it: the reference
 * reads each keyframe's own copy (equal within an agent) and even KF1's mbf for KF2 (:406). */
typedef struct orbm_tri_geom {
    float fx, fy, cx, cy, bf, b;    /* camera, mbf, mb                                            */
    int32_t nlevels;                /* mnScaleLevels, 1..16                                       */
    float scale_factors[16];        /* mvScaleFactors; [1] = mfScaleFactor is read whatever nlevels */
    float level_sigma2[16];         /* mvLevelSigma2                                              */
} orbm_tri_geom;

/* One code per outcome of a feature of the current keyframe (status arrays, int8). */
enum {
    ORBM_TRI_NO_MATCH = 0,      /* match12[i] < 0                                                   */
    ORBM_TRI_TRIANGULATED = 1,  /* created by the linear triangulation (:321-338)                   */
    ORBM_TRI_STEREO1 = 2,       /* created from KF1's stereo (:340-343)                             */
    ORBM_TRI_STEREO2 = 3,       /* created from KF2's stereo (:344-347)                             */
    ORBM_TRI_BASELINE = 4,      /* the pair was skipped by the baseline test (:251, :259)           */
    ORBM_TRI_LOW_PARALLAX = 5,  /* :349                                                             */
    ORBM_TRI_W_ZERO = 6,        /* :333                                                             */
    ORBM_TRI_Z1 = 7,            /* :355                                                             */
    ORBM_TRI_Z2 = 8,            /* :359                                                             */
    ORBM_TRI_REPROJ1 = 9,       /* :374 / :385                                                      */
    ORBM_TRI_REPROJ2 = 10,      /* :400 / :411                                                      */
    ORBM_TRI_DIST_ZERO = 11,    /* :422                                                             */
    ORBM_TRI_SCALE_RATIO = 12,  /* :430                                                             */
    ORBM_TRI_EXCLUDED = 13      /* excluded by the contract below                                   */
};

/* One pair on the host: current keyframe 1 (n1 features: kps1 = mvKeysUn, uright1 / depth1 = mvuRight /
 * mvDepth or NULL = monocular, all -1; desc1 = mDescriptors), neighbour 2 likewise (no descriptors),
 * Tcw1 / Tcw2 = their poses (4x4 row-major), match12[i] = idx2 or negative. Pair test: baseline =
 * (float)sqrt(sum (double)(Ow2 - Ow1)^2), Ow2 - Ow1 in float, Ow = -Rcw.t() * tcw (GEMM_1_T); !monocular:
 * skipped when baseline < geom->b; monocular: when (double)(baseline / median_depth2) < 0.01, a float
 * divide (ComputeSceneMedianDepth(2) stays with the caller). Every matched row of a skipped pair gets
 * ORBM_TRI_BASELINE. The float sequence of one match, in cv::Mat's arithmetic (DESIGN.md "Pinned
 * semantics"; dot_d / norm_d accumulate (double)a * (double)b from 0 in index order):
 *   invfx = 1.0f / fx; xn = ((u - cx) * invfx, (v - cy) * invfy, 1) in float, both keyframes;
 *   ray = Rwc * xn: ray[i] = R[0][i] * xn[0] + R[1][i] * xn[1] + R[2][i] * xn[2], float products summed in
 *   float (the small-matrix gemm without an addend);
 *   cosParallaxRays = (float)(dot_d(ray1, ray2) / (norm_d(ray1) * norm_d(ray2)));
 *   bStereo_k = mvuRight_k >= 0; cosParallaxStereo1 = cosParallaxStereo2 = cosParallaxRays + 1.0f;
 *   if bStereo1: cosParallaxStereo1 = cosf(2.0f * atan2f(b * 0.5f, depth1)), else if bStereo2 the same for
 *   KF2 (:311-314, the else kept) -- glibc's float overloads; cosParallaxStereo = std::min(1, 2) = 2 < 1 ? 2 : 1;
 *   triangulate iff cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0.0f && (bStereo1 || bStereo2 ||
 *   (double)cosParallaxRays < 0.9998):
 *     A[0] = xn1[0] * Tcw1.row(2) - Tcw1.row(0), A[1] with xn1[1] and row 1, A[2], A[3] from KF2: a float
 *     product, then a float difference;
 *     x = vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV), pinned as OpenCV 3.x's built-in
 *     one-sided Jacobi (no LAPACK) on At = A.t(): W[i] = dot_d(At[i], At[i]), Vt = I; up to 30 sweeps over
 *     the pairs i < j: p = dot_d(At[i], At[j]); skipped when |p| <= (double)(2 * FLT_EPSILON) * sqrt(W[i] *
 *     W[j]); p *= 2, beta = W[i] - W[j], gamma = sqrt(p * p + beta * beta) (OpenCV: hypot), all double;
 *     beta < 0: s = (float)sqrt((gamma - beta) * 0.5 / gamma), c = (float)(p / (gamma * s * 2)); else
 *     c = (float)sqrt((gamma + beta) / (gamma * 2)), s = (float)(p / (gamma * c * 2)); both rows in float:
 *     t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k], W[i] and W[j] re-accumulated from t0, t1 in
 *     double; the same rotation on rows i, j of Vt; stop after a sweep without a rotation; then W[i] =
 *     sqrt(dot_d(At[i], At[i])) and a selection sort, descending, that swaps W and the rows on strict <;
 *     x[3] == 0 -> ORBM_TRI_W_ZERO; x3D = x[0..2] * (float)(1.0 / (double)x[3]);
 *   else if bStereo1 && cosParallaxStereo1 < cosParallaxStereo2: x3D = KF1's orbx_unproject_stereo of idx1;
 *   else if bStereo2 && cosParallaxStereo2 < cosParallaxStereo1: KF2's of idx2; else ORBM_TRI_LOW_PARALLAX;
 *   per keyframe: x, y, z = (float)(dot_d(Rcw.row(r), x3D) + (double)tcw[r]); z1 <= 0 -> Z1, then z2 <= 0 -> Z2;
 *   per keyframe, KF1 first: invz = (float)(1.0 / (double)z); u' = fx * x * invz + cx, v' = fy * y * invz +
 *   cy (float, left to right); e2 = (u' - u)^2 + (v' - v)^2 in float; with mvuRight: u_r = u' - bf * invz,
 *   e2 += (u_r - mvuRight)^2 and (double)e2 > 7.8 * (double)sigma2 rejects, without: > 5.991 * sigma2;
 *   sigma2 = level_sigma2[octave];
 *   normal_k = x3D - Ow_k (float), dist_k = (float)norm_d(normal_k); dist1 == 0 || dist2 == 0 -> DIST_ZERO;
 *   ratioDist = dist2 / dist1, ratioOctave = sf[oct1] / sf[oct2], ratioFactor = 1.5f * sf[1]:
 *   ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor -> SCALE_RATIO;
 *   the MapPoint: position x3D; normal = ((0.0f + normal1 * (float)(1.0 / norm_d(normal1))) + normal2 *
 *   (float)(1.0 / norm_d(normal2))) * 0.5f (the norms as doubles; independent of the map order); reference
 *   keyframe KF1: max_dist = dist1 * sf[oct1], min_dist = max_dist / sf[nlevels - 1] (raw, without the
 *   0.8f / 1.2f); descriptor = desc1 row idx1 (ComputeDistinctiveDescriptors of two observations has both
 *   medians 0 and takes the first in std::map<KeyFrame*, ...> order, which is allocator-dependent: pinned
 *   to the current keyframe); flags = 9 (bit 0 a MapPoint, bit 3 Observations() > 0).
 * Contract (ORBM_TRI_EXCLUDED, no other row is affected): a non-finite pose entry of either keyframe
 * (every matched row); idx2 >= n2; an octave outside [0, nlevels); a non-finite keypoint coordinate or
 * mvuRight; with bStereo1 || bStereo2 a b that is not finite and > 0; a bStereo_k depth that is not finite
 * and > 0 (only atan2f's first quadrant is restated on the device); a non-finite cosParallaxRays, null
 * vector, x3D, camera coordinate, e2, dist or ratioDist.
 * Outputs: status[i], pos3[3i .. +3) (zeros unless created) for every i < n1; the new points in ascending
 * idx1 order (the reference's creation order) in rows [0, *nnew) of tab_* (each with room for n1 rows;
 * tab_desc 32 bytes a row; tab_feat1 / tab_feat2 = idx1 / idx2); *nnew = the reference's nnew for this
 * neighbour. Host only, no device. ORBX_EARG on NULL arguments, n1 < 0, n2 < 0, nlevels outside [1, 16] or
 * fx == 0 || fy == 0, before anything is written. */
int orbx_triangulate_matches(const orbm_tri_geom* geom, int monocular, float median_depth2,
                             const float Tcw1[16], const float Tcw2[16], int n1, const orbx_kp* kps1,
                             const float* uright1, const float* depth1, const uint8_t* desc1, int n2,
                             const orbx_kp* kps2, const float* uright2, const float* depth2,
                             const int32_t* match12, int8_t* status, float* pos3, float* tab_pos,
                             float* tab_normal, float* tab_min_dist, float* tab_max_dist, uint8_t* tab_desc,
                             uint8_t* tab_flags, int32_t* tab_feat1, int32_t* tab_feat2, int32_t* nnew);

/* The same for npairs pairs of one device batch, in the batch matchers' layout so that their outputs
 * plug in unchanged: pair p is current keyframe d_q1[p] against neighbour d_q2[p]; per frame f everything
 * at f*kp_stride (d_kps_un = mvKeysUn, d_uright / d_depth = mvuRight / mvDepth or both NULL = monocular,
 * d_desc, count d_counts[f]) and d_Tcw[16 f .. +16); d_match12[p*kp_stride + i] = the matcher's row;
 * d_median_depth2[p] is read only when monocular != 0 (may be NULL otherwise). Ow is derived per frame on
 * the device, as orbx_unproject_stereo_batch_device does.
 * Per feature: d_status[p*kp_stride + i] and d_pos3[(p*kp_stride + i)*3 .. +3); rows i >= d_counts[d_q1[p]]
 * are not written. Per pair: its new points in ascending idx1 order in rows [p*kp_stride, p*kp_stride +
 * d_nnew[p]) of d_tab_pos, d_tab_normal (x 3), d_tab_min_dist, d_tab_max_dist, d_tab_desc (x 32, 16-byte
 * aligned), d_tab_flags, d_tab_feat1, d_tab_feat2 (each npairs*kp_stride rows: a table of M =
 * npairs*kp_stride MapPoints for orbm_search_local_points_batch_device); d_new_range[2p], [2p+1] =
 * p*kp_stride, p*kp_stride + d_nnew[p]: a d_range pair usable as-is. Bit-identical to the host form, and
 * independent of the order or repetition of the pair list.
 * One launch, one workgroup per pair: the row is walked in chunks of one lane per feature; ballot, prefix
 * over the waves and a running base give every created point its row, so the compaction keeps idx1 order.
 * Validation on the device: every ORBM_TRI_EXCLUDED row also raises the ctx's error flag
 * (orbm_check_error); a pair with a frame index outside [0, nframes) or a count above kp_stride raises it
 * and gets d_nnew = 0, an empty range and ORBM_TRI_NO_MATCH in its whole d_status row (kp_stride entries;
 * d_pos3 zeros), and reads nothing out of range; the other pairs are unaffected.
 * ORBX_EARG before anything is enqueued for NULL arguments, npairs < 0, nframes < 1, kp_stride outside
 * [1, 65536], nlevels outside [1, 16], fx == 0 || fy == 0, only one of d_uright / d_depth, or d_kps_un /
 * d_desc / d_tab_desc not 8- / 16- / 16-byte aligned; npairs == 0 (with a valid ctx, geom and sizes) is a
 * no-op that returns 0. The call only enqueues on `stream`: no upload, no host wait, no scratch. */
int orbm_create_new_map_points_batch_device(
    orbm_ctx* ctx, int npairs, const int32_t* d_q1, const int32_t* d_q2, int nframes, const orbx_kp* d_kps_un,
    const int32_t* d_counts, int kp_stride, const float* d_uright, const float* d_depth, const uint8_t* d_desc,
    const float* d_Tcw, const int32_t* d_match12, const orbm_tri_geom* geom, int monocular,
    const float* d_median_depth2, int8_t* d_status, float* d_pos3, float* d_tab_pos, float* d_tab_normal,
    float* d_tab_min_dist, float* d_tab_max_dist, uint8_t* d_tab_desc, uint8_t* d_tab_flags,
    int32_t* d_tab_feat1, int32_t* d_tab_feat2, int32_t* d_new_range, int32_t* d_nnew, void* stream);

/* ------------------------------------------------------------------------------------
 * Pose optimisation: Optimizer::PoseOptimization(Frame*) (Optimizer.cc:239-451), the one
 * consumer of every match row the tracking searches write (TrackWithMotionModel,
 * TrackReferenceKeyFrame, TrackLocalMap, Relocalization).
 * ---------------------------------------------------------------------------------- */
enum {
    ORBM_POSE_OK = 0,       /* optimised: Tcw, outlier and ninliers are the reference's                */
    ORBM_POSE_TOO_FEW = 1,  /* nInitialCorrespondences < 3 (:364): ninliers = 0, the pose is unchanged */
    ORBM_POSE_EXCLUDED = 2  /* excluded by the contract below: pose and outlier bytes are unchanged    */
};

/* PoseOptimization of one frame on the host. g: fx, fy, cx, cy, bf are read; inv_level_sigma2 = mvInvLevelSigma2
 * (nlevels entries); Tcw = mTcw (row-major 4x4, in and out); kps_un = mvKeysUn, uright = mvuRight (NULL = all
 * monocular); mp_index[i] = the row of feature i's MapPoint in pos (Mrows x 3, GetWorldPos), negative = none.
 * Optimizer.cc is followed literally; g2o and Eigen are not part of the reference tree, so their share is pinned
 * here (DESIGN.md "Pinned semantics"). All arithmetic is double without contraction unless marked.
 *
 *   Edges, i ascending over the features with a MapPoint: Xw = (double)pos row; invSigma2 = (double)
 *   inv_level_sigma2[octave]; uright[i] < 0 -> mono, obs = (x, y), delta = (double)(float)sqrt(5.991); else stereo,
 *   obs = (x, y, uright[i]), delta = (double)(float)sqrt(7.815). outlier[i] = 0, level 0. Fewer than 3 -> TOO_FEW.
 *   The active edges of an evaluation are those at level 0, visited in ascending i (mono and stereo interleaved).
 *
 *   State (q = (x, y, z, w), t). se3_from_Tcw: R, t widened; tr = R00 + R11 + R22; tr > 0: s = sqrt(tr + 1),
 *   w = 0.5 s, s = 0.5 / s, x = (R21 - R12) s, y = (R02 - R20) s, z = (R10 - R01) s; else i = argmax of the diagonal
 *   (first wins; R11 > R00, then R22 > Rii), j, k cyclic: s = sqrt(Rii - Rjj - Rkk + 1), q[i] = 0.5 s, s = 0.5 / s,
 *   w = (Rkj - Rjk) s, q[j] = (Rji + Rij) s, q[k] = (Rki + Rik) s. Normalise: q /= sqrt(x^2 + y^2 + z^2 + w^2); w < 0
 *   negates q. se3_map(X) = q (x) X + t with uv = qv x X; uv = uv + uv; (X + w uv) + qv x uv.
 *   se3_to_Tcw: tx = 2x, ty = 2y, tz = 2z, twx = tx w, twy = ty w, twz = tz w, txx = tx x, txy = ty x, txz = tz x,
 *   tyy = ty y, tyz = tz y, tzz = tz z; R = [1 - (tyy + tzz), txy - twz, txz + twy; txy + twz, 1 - (txx + tzz),
 *   tyz - twx; txz - twy, tyz + twx, 1 - (txx + tyy)], each and t cast to float; last row 0 0 0 1.
 *   se3_exp_mul(d), omega = d[0..3], upsilon = d[3..6]: theta = sqrt(omega . omega), Om = skew(omega), Om2 = Om Om;
 *   theta < 0.00001: R = (I + Om) + Om2, V = R; else (s, c) = so3_sincos(theta), R = (I + (s / theta) Om) +
 *   ((1 - c) / (theta theta)) Om2, V = (I + ((1 - c) / (theta theta)) Om) + ((theta - s) / ((theta theta) theta)) Om2;
 *   qd = quaternion of R (normalised), td = V upsilon; q = normalise(qd (x) q) (Hamilton: w = aw bw - ax bx - ay by
 *   - az bz, x = aw bx + ax bw + ay bz - az by, y = aw by + ay bw + az bx - ax bz, z = aw bz + az bw + ax by - ay bx),
 *   t = td + qd (x) t. 3x3 products and sums row-major, left to right.
 *   so3_sincos: k = (int)(theta (2/pi) + 0.5), r = ((theta - k PIO2_1) - k PIO2_2) - k PIO2_3, Taylor polynomials of degree 17 /
 *   16 in Horner form, the quadrant from k & 3 (csrc/pose_math.h; not libm's).
 *
 *   Edge at the estimate: (X, Y, Z) = se3_map(Xw), invz = 1 / Z, u = (X invz) fx + cx, v = (Y invz) fy + cy, stereo
 *   ur = u - bf invz; e = obs - (u, v[, ur]); chi2 = sum_r e_r (invSigma2 e_r). Huber while the edge has its kernel:
 *   chi2 <= delta^2: rho0 = chi2, rho1 = 1; else sq = sqrt(chi2), rho0 = (2 sq) delta - delta^2, rho1 = delta / sq.
 *   iz2 = invz invz; J row 0 = (((X Y) iz2) fx, -(1 + (X X) iz2) fx, (Y invz) fx, -invz fx, 0, (X iz2) fx), row 1 =
 *   ((1 + (Y Y) iz2) fy, -((X Y) iz2) fy, -(X invz) fy, 0, -invz fy, (Y iz2) fy), stereo row 2 = (J00 - (bf Y) iz2,
 *   J01 + (bf X) iz2, J02, J03, 0, J05 - bf iz2). wgt = rho1 invSigma2; H[a][b] += sum_r J[r][a] (wgt J[r][b]) for
 *   a <= b, mirrored; b[a] += sum_r J[r][a] ((-(invSigma2 e_r)) rho1); the graph's robust chi2 = sum rho0. Inner sums
 *   over r ascending, the accumulation from 0 over the active edges ascending.
 *
 *   Levenberg, one optimize(10): for iter 0..9: evaluate (cur, H, b); iter 0: lambda = 1e-5 max_a |H[a][a]|, nu = 2;
 *   rho = 0, q = 0; repeat { solve (H + lambda I) x = b by LDL^T without pivoting (d_j = A_jj - sum_{k<j} (L_jk d_k)
 *   L_jk, a d_j that is not > 0 fails with x = 0; L_ij = (A_ij - sum_{k<j} (L_ik d_k) L_jk) / d_j; y_i = b_i -
 *   sum_{k<i} L_ik y_k; x_i = y_i / d_i - sum_{k>i} L_ki x_k); save the estimate, apply se3_exp_mul(x), evaluate the
 *   errors only: tmp = sum rho0, DBL_MAX if the solve failed; scale = sum_a x[a] (lambda x[a] + b[a]) + 1e-3; rho =
 *   (cur - tmp) / scale; rho > 0 and tmp finite: alpha = min(1 - (2 rho - 1)^3, 2/3), lambda *= max(1/3, alpha), nu
 *   = 2, cur = tmp; else lambda *= nu, nu *= 2, the saved estimate returns; q++ } while rho < 0 and q < 10. The
 *   iterations end early when q == 10 or rho == 0.
 *
 *   Four rounds (:374-442): the estimate restarts from Tcw, optimize(10) over the active edges (none: no
 *   iteration); then per edge chi2 = (float) of its error -- an active edge's error is that of the last evaluation
 *   (after a rejected last trial: at the rejected estimate), an outlier's is recomputed at the estimate -- and
 *   chi2 > (float)5.991 (mono) / (float)7.815 (stereo) makes it an outlier at level 1, else an inlier at level 0;
 *   after the third round the Huber kernels are removed; fewer than 10 edges: one round only. Tcw = se3_to_Tcw of the
 *   last estimate, *ninliers = nInitialCorrespondences - nBad.
 *
 * outlier[i] (mvbOutlier) is written for features with a MapPoint only. diag (optional, 8 ints, for tests): rounds
 * run, the Levenberg iterations of each of the four rounds, rejected trials, failed solves, and exp calls that took
 * the theta < 0.00001 branch.
 * Contract (ORBM_POSE_EXCLUDED: *ninliers = 0, Tcw and outlier untouched; the reference's behaviour is undefined or
 * meaningless there): a non-finite entry of Tcw's first three rows; on a feature with a MapPoint an octave outside
 * [0, nlevels) or a non-finite keypoint, uright or position; a non-finite robust chi2 at a round's first evaluation.
 * Host only, no device, no allocation. ORBX_EARG on NULL arguments, n outside [0, 65536] (the kp_stride limit of the
 * device entries) or nlevels outside [1, 16], before anything is written. */
int orbx_pose_optimization(const orbm_track_geom* geom, const float* inv_level_sigma2, int nlevels, float Tcw[16],
                           int n, const orbx_kp* kps_un, const float* uright, const int32_t* mp_index,
                           const float* pos, uint8_t* outlier, int32_t* ninliers, int32_t* status, int32_t* diag);

/* The same for njobs jobs over one device batch: job j is the reference call on frame d_frame[j] (everything of a
 * frame at f*kp_stride, count d_counts[f]; d_uright NULL = monocular) with the MapPoints d_mp_index[j*kp_stride + i]
 * (a row of d_pos, mrows x 3; negative = none) and the pose d_Tcw_in[16 f ..). Jobs share nothing; a frame may appear
 * in several jobs. Outputs per job: d_Tcw_out[16 j ..) (may alias d_Tcw_in when d_frame[j] == j for every job:
 * a job reads its pose before it writes it; any other job list needs separate arrays, workgroups are not ordered), d_outlier[j*kp_stride + i] for features with a MapPoint,
 * d_ninliers[j], d_status[j] (ORBM_POSE_*). Optional, in the same launch:
 *   d_mp_flags [njobs x kp_stride]   bit 2 := outlier on features with a MapPoint, the other bits kept: the row
 *                                    orbm_search_by_projection_last_frame_batch_device reads of its LastFrame;
 *   d_frame_mp [njobs x kp_stride]   Tracking's discard loop (Tracking.cc, after each PoseOptimization): an outlier's
 *                                    entry becomes -1 (the array orbm_search_local_points_batch_device reads);
 *   d_nmatches_map [njobs]           nmatchesMap: the kept features whose d_mp_flags bit 3 (Observations() > 0) is set
 *                                    (without d_mp_flags: all kept features).
 * One workgroup per job; H, b and the chi2 sums accumulate in double in ascending feature order, so every output is
 * bit-identical to the host form whatever the schedule.
 * Validation on the device, each raising the ctx's error flag (orbm_check_error): a count above kp_stride is
 * clamped; an mp_index >= mrows counts as no MapPoint; a frame index outside [0, nframes) or a row the contract
 * above excludes gives ORBM_POSE_EXCLUDED with the pose copied through (a bad frame index: d_Tcw_out[16 j ..) is not written), d_ninliers
 * = 0 and the outlier row, d_mp_flags and d_frame_mp untouched (d_nmatches_map = 0). No job affects another.
 * ORBX_EARG for NULL required arguments, njobs < 0, nframes < 1, kp_stride outside [1, 65536], mrows < 0, nlevels
 * outside [1, 16] or d_kps_un not 8-byte aligned; njobs == 0 is a no-op that returns 0. The call only enqueues on
 * `stream`: no upload, no host wait, no scratch. */
int orbm_pose_optimization_batch_device(
    orbm_ctx* ctx, int njobs, const int32_t* d_frame, int nframes, const orbx_kp* d_kps_un, const int32_t* d_counts,
    int kp_stride, const float* d_uright, const orbm_track_geom* geom, const float* inv_level_sigma2,
    const int32_t* d_mp_index, const float* d_pos, int mrows, const float* d_Tcw_in, float* d_Tcw_out,
    uint8_t* d_outlier, uint8_t* d_mp_flags, int32_t* d_frame_mp, int32_t* d_ninliers, int32_t* d_nmatches_map,
    int8_t* d_status, void* stream);

/* ------------------------------------------------------------------------------------
 * Synthetic input: deterministic frame t of agent a, width x height,
 * written to host out (pitch = width). Identical on every machine (integer-only).
 * ---------------------------------------------------------------------------------- */
int orbx_synth_frame(int agent, int t, int width, int height, uint8_t* out);
/* frames t0 .. t0+count-1 of agent a, back to back (frame stride width*height). */
int orbx_synth_frames(int agent, int t0, int count, int width, int height, uint8_t* out);
/* right image of a rectified stereo rig for the same frames: the crop shifted by +dx pixels
 * in x (0 <= dx <= 26), i.e. a fronto-parallel scene at disparity dx. */
int orbx_synth_frames_shifted(int agent, int t0, int count, int width, int height, int dx,
                              uint8_t* out);
/* shared-scene frames: view `view` (an agent) of the texture of `scene`, its crop 12*view pixels
 * further along the pan (mod 600), so several agents see overlapping parts of one environment as
 * A1 and A2 do; view 0 equals orbx_synth_frames_shifted(scene, ...). */
int orbx_synth_scene_frames(int scene, int view, int t0, int count, int width, int height, int dx,
                            uint8_t* out);

/* Stage profiling: a pair of HIP events brackets each stage's kernel on the stream it is
 * launched on (the overlapped schedule is kept, so a stage's time includes sharing the GPU
 * with the stage that runs beside it): stages = {pyramid, fast_cells, octree, blur, describe}.
 * orbx_profile_enable(h, mask) resets the accumulators and brackets the stages in `mask`
 * (bit k = stage k, 0x1F = all, 0 = off); orbx_profile_read waits for the recorded events and
 * returns the summed milliseconds per stage (ms[5], 0 for stages not in the mask) and the
 * number of profiled extraction calls. */
int orbx_profile_enable(orbx_handle* h, int on);
int orbx_profile_read(orbx_handle* h, double* ms, int* ncalls);

/* Schedule hook: every subsequent batched extraction of this handle records `event` (a hipEvent_t
 * created by the caller; NULL = off) on its stream right after the pyramid launch, so another stream
 * can start its own work once this batch's pyramid is done (bench schedules that stagger concurrent
 * extraction graphs by pyramid rather than by whole extraction). */
int orbx_set_pyramid_event(orbx_handle* h, void* event);
/* The same for any of the first two stages: stage 0 = after the pyramid launch (orbx_set_pyramid_event), 1 = after
 * the FAST launch; one event per stage, NULL = off. The bench staggers its graphs by FAST: graph p starts a step
 * once graph p-1's FAST is done, a third of the step apart at 3 graphs. */
int orbx_set_stage_event(orbx_handle* h, int stage, void* event);

/* Library/version and device probe. */
const char* orbx_version(void);
int orbx_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* ORBSLAM_AMD_H */

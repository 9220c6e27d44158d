/*
 * pose_kernels.hip -- Optimizer::PoseOptimization(Frame*) (Optimizer.cc:239-451) over a device batch on gfx950: from
 * the match rows the tracking searches leave in HBM to the optimised poses, mvbOutlier and the inlier counts, with
 * Tracking's discard loop.
 *
 * The arithmetic is pose_math.h's (through frame_math.h), the statement the host unit pose_optimize.c is built from.
 * One launch, one workgroup per job, no host step. Lanes evaluate edges in parallel, one lane per feature in chunks of
 * the workgroup; each writes its 28 terms (21 of H's upper triangle, 6 of b, rho0) to LDS, and 28 lanes then walk one
 * column each in feature order, so every sum has the order of the host loop. Levenberg's uniform part (the 6x6 solve,
 * exp, the quaternion product, accept / reject) runs on lane 0 over state kept in LDS.
 */
#include <hip/hip_runtime.h>

#include "frame_math.h"
#include "matcher_host.h"
#include "orbslam_amd_testing.h"

namespace orbamd {

namespace {

constexpr int kPoseThreads = 128;
constexpr int kPoseWaves = kPoseThreads / 64;
constexpr int kErrPoseJob = 256;    // a frame index outside the batch, a count above kp_stride, an mp_index >= mrows
constexpr int kErrPoseInput = 512;  // a job the PoseOptimization contract excludes

struct PoseArgs {
    const int32_t* frame;
    int nframes;
    const orbx_kp* kps;
    const int32_t* counts;
    int kp_stride;
    const float* uright;
    float fx, fy, cx, cy, bf;
    int nlevels;
    float inv_sigma2[kMaxLevels];
    const int32_t* mp_index;
    const float* pos;
    int mrows;
    const float* Tcw_in;
    float* Tcw_out;
    uint8_t *outlier, *mp_flags;
    int32_t *frame_mp, *ninliers, *nmatches_map;
    int8_t* status;
    int32_t* err;
};

struct PoseEdge {
    double Xw[3], ox, oy, our, w;
    int stereo, octave;
    bool finite;
};

/* feature i of the job: false when it has no MapPoint; the edge's constants otherwise */
__device__ __forceinline__ bool pose_load_edge(const PoseArgs& a, const float* s_inv_sigma2, long long fb, long long jb,
                                               int i, PoseEdge& e) {
    const int mp = a.mp_index[jb + i];
    if (mp < 0 || mp >= a.mrows) return false;
    const uint2* k = (const uint2*)(a.kps + fb + i);
    const uint2 xy = k[0], ro = k[2];  // (x, y) (size, angle) (response, octave)
    const float x = __uint_as_float(xy.x), y = __uint_as_float(xy.y);
    const float ur = a.uright ? a.uright[fb + i] : -1.0f;
    const float X = a.pos[3 * (long long)mp], Y = a.pos[3 * (long long)mp + 1], Z = a.pos[3 * (long long)mp + 2];
    e.octave = (int)ro.y;
    e.finite = finite_f(x) && finite_f(y) && finite_f(ur) && finite_f(X) && finite_f(Y) && finite_f(Z);
    e.stereo = !(ur < 0.0f);
    e.Xw[0] = (double)X, e.Xw[1] = (double)Y, e.Xw[2] = (double)Z;
    e.ox = (double)x, e.oy = (double)y, e.our = e.stereo ? (double)ur : 0.0;
    e.w = (unsigned)e.octave < (unsigned)a.nlevels ? (double)s_inv_sigma2[e.octave] : 0.0;
    return true;
}

/* One evaluation of the active edges at s_est: full = the 28 sums into dst[0..28), else the robust chi2 into dst[0].
 * Ends with a barrier. A lane without an active edge is skipped by the walk, not added as zero. */
__device__ __forceinline__ void pose_eval_pass(const PoseArgs& a, const pm_cam& cam, const float* s_inv_sigma2,
                                               long long fb, long long jb, int n, int full, int robust, double dm,
                                               double ds, const double* s_est, const uint32_t* s_lvl, double* s_terms,
                                               uint8_t* s_act, double* dst) {
    const int tid = threadIdx.x;
    double est[7];
#pragma unroll
    for (int k = 0; k < 7; k++) est[k] = s_est[k];
    double acc = 0.0;
    const bool walker = full ? tid < PM_NTERMS : tid == PM_NTERMS - 1;
    for (int c0 = 0; c0 < n; c0 += kPoseThreads) {
        const int i = c0 + tid;
        bool act = false;
        if (i < n && !((s_lvl[i >> 5] >> (i & 31)) & 1u)) {
            PoseEdge e;
            if (pose_load_edge(a, s_inv_sigma2, fb, jb, i, e)) {
                act = true;
                const double delta = robust ? (e.stereo ? ds : dm) : 0.0;
                pose_edge_eval(&cam, est, e.Xw[0], e.Xw[1], e.Xw[2], e.ox, e.oy, e.our, e.stereo, e.w, delta, full,
                               s_terms + tid, kPoseThreads);
            }
        }
        s_act[tid] = act;
        __syncthreads();
        if (walker) {
            const int cnt = min(kPoseThreads, n - c0);
            const double* col = s_terms + tid * kPoseThreads;
            for (int k = 0; k < cnt; k++)
                if (s_act[k]) acc = __dadd_rn(acc, col[k]);
        }
        __syncthreads();
    }
    if (walker) dst[full ? tid : 0] = acc;
    __syncthreads();
}

__global__ __launch_bounds__(kPoseThreads) void k_pose_optimize(PoseArgs a) {
    __shared__ double s_terms[PM_NTERMS * kPoseThreads];
    __shared__ double s_sum[PM_NTERMS], s_tmp[1], s_est0[7], s_est[7], s_saved[7], s_errst[7], s_x[6];
    __shared__ pm_lm s_lm;
    __shared__ uint32_t s_lvl[65536 / 32];  // bit i = feature i's edge is at level 1 (an outlier)
    __shared__ float s_Tin[16], s_inv_sigma2[kMaxLevels];
    __shared__ uint8_t s_act[kPoseThreads];
    __shared__ int s_ctl[3], s_cnt[4];
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.kp_stride;
    const long long jb = (long long)j * S;
    const int f = a.frame[j];
    if ((unsigned)f >= (unsigned)a.nframes) {  // uniform: nothing of the frame is read, no pose is written
        if (tid == 0) {
            a.status[j] = ORBM_POSE_EXCLUDED;
            a.ninliers[j] = 0;
            if (a.nmatches_map) a.nmatches_map[j] = 0;
            atomicOr(a.err, kErrPoseJob);
        }
        return;
    }
    const long long fb = (long long)f * S;
    int n = max(a.counts[f], 0);
    if (n > S) {
        n = S;
        if (tid == 0) atomicOr(a.err, kErrPoseJob);
    }
    if (tid < 16) s_Tin[tid] = a.Tcw_in[16 * (long long)f + tid];
    if (tid < kMaxLevels) s_inv_sigma2[tid] = a.inv_sigma2[tid];
    if (tid < 4) s_cnt[tid] = 0;
    if (tid < 3) s_ctl[tid] = 0;
    for (int w = tid; w < (n + 31) / 32 + 2 && w < 65536 / 32; w += kPoseThreads) s_lvl[w] = 0;
    __syncthreads();
    {  // nInitialCorrespondences and the contract
        int ninit = 0, bad = 0, oob = 0;
        if (tid < 12 && !finite_f(s_Tin[tid])) bad = 1;
        for (int i = tid; i < n; i += kPoseThreads) {
            PoseEdge e;
            oob |= a.mp_index[jb + i] >= a.mrows;
            if (!pose_load_edge(a, s_inv_sigma2, fb, jb, i, e)) continue;
            ninit++;
            bad |= !e.finite || (unsigned)e.octave >= (unsigned)a.nlevels;
        }
        if (ninit) atomicAdd(&s_cnt[0], ninit);
        if (bad) atomicOr(&s_cnt[1], 1);
        if (oob) atomicOr(&s_cnt[2], 1);
    }
    __syncthreads();
    const int ninit = s_cnt[0];
    if (tid == 0 && s_cnt[2]) atomicOr(a.err, kErrPoseJob);
    int st = s_cnt[1] ? ORBM_POSE_EXCLUDED : ninit < 3 ? ORBM_POSE_TOO_FEW : ORBM_POSE_OK;
    pm_cam cam;
    cam.fx = (double)a.fx, cam.fy = (double)a.fy, cam.cx = (double)a.cx, cam.cy = (double)a.cy, cam.bf = (double)a.bf;
    const double dm = (double)__double2float_rn(__dsqrt_rn(5.991)), ds = (double)__double2float_rn(__dsqrt_rn(7.815));
    int nbad = 0, robust = 1;
    if (st == ORBM_POSE_OK) {
        if (tid == 0) {
            se3_from_Tcw(s_Tin, s_est0);
            s_lm.rejected = s_lm.fails = s_lm.small = 0;
        }
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < 4; it++) {
            if (tid < 7) {
                s_est[tid] = s_est0[tid];
                s_errst[tid] = s_est0[tid];
            }
            if (tid == 0) s_cnt[3] = 0;
            __syncthreads();
            const int nact = ninit - nbad;
#pragma unroll 1
            for (int iter = 0; iter < 10 && nact > 0; iter++) {
                pose_eval_pass(a, cam, s_inv_sigma2, fb, jb, n, 1, robust, dm, ds, s_est, s_lvl, s_terms, s_act, s_sum);
                if (tid == 0) {
#pragma unroll
                    for (int k = 0; k < 7; k++) s_errst[k] = s_est[k];
                    if (iter == 0 && !pm_finite(s_sum[27]))
                        s_ctl[0] = 1;
                    else
                        pm_lm_iter_begin(&s_lm, s_sum, iter);
                }
                __syncthreads();
                if (s_ctl[0]) break;
#pragma unroll 1
                for (;;) {
                    if (tid == 0) pm_lm_trial_step(&s_lm, s_sum, s_x, s_est, s_saved);
                    __syncthreads();
                    pose_eval_pass(a, cam, s_inv_sigma2, fb, jb, n, 0, robust, dm, ds, s_est, s_lvl, s_terms, s_act,
                                   s_tmp);
                    if (tid == 0) {
#pragma unroll
                        for (int k = 0; k < 7; k++) s_errst[k] = s_est[k];
                        s_ctl[1] = pm_lm_trial_end(&s_lm, s_sum, s_tmp[0], s_x, s_est, s_saved);
                        s_ctl[2] = pm_lm_terminate(&s_lm);
                    }
                    __syncthreads();
                    if (!s_ctl[1]) break;
                }
                if (s_ctl[2]) break;
            }
            if (s_ctl[0]) {
                st = ORBM_POSE_EXCLUDED;
                break;
            }
            // :381-438: an inlier's chi2 is the error of the last evaluation, an outlier's is recomputed at the estimate
            double est[7], errst[7];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                est[k] = s_est[k];
                errst[k] = s_errst[k];
            }
            for (int c0 = 0; c0 < n; c0 += kPoseThreads) {
                const int i = c0 + tid;
                bool out = false;
                if (i < n) {
                    PoseEdge e;
                    if (pose_load_edge(a, s_inv_sigma2, fb, jb, i, e)) {
                        const bool lvl = (s_lvl[i >> 5] >> (i & 31)) & 1u;
                        double at[7];
#pragma unroll
                        for (int k = 0; k < 7; k++) at[k] = lvl ? est[k] : errst[k];
                        out = pose_edge_outlier(pose_edge_eval(&cam, at, e.Xw[0], e.Xw[1], e.Xw[2], e.ox, e.oy, e.our,
                                                               e.stereo, e.w, 0.0, 0, nullptr, 0),
                                                e.stereo);
                    }
                }
                const unsigned long long m = __ballot(out);
                if (lane == 0) {
                    const int w = (c0 + wave * 64) >> 5;
                    s_lvl[w] = (uint32_t)m;
                    s_lvl[w + 1] = (uint32_t)(m >> 32);
                    if (m) atomicAdd(&s_cnt[3], __popcll(m));
                }
            }
            __syncthreads();
            nbad = s_cnt[3];
            if (it == 2) robust = 0;
            __syncthreads();  // s_cnt[3] is zeroed by the next round
            if (ninit < 10) break;
        }
    }
    if (st == ORBM_POSE_EXCLUDED) {
        if (tid < 16) a.Tcw_out[16 * (long long)j + tid] = s_Tin[tid];
        if (tid == 0) {
            a.status[j] = ORBM_POSE_EXCLUDED;
            a.ninliers[j] = 0;
            if (a.nmatches_map) a.nmatches_map[j] = 0;
            atomicOr(a.err, kErrPoseInput);
        }
        return;
    }
    if (tid == 0) {
        if (st == ORBM_POSE_OK) {
            float T[16];
            se3_to_Tcw(s_est, T);
#pragma unroll
            for (int k = 0; k < 16; k++) a.Tcw_out[16 * (long long)j + k] = T[k];
        }
        a.status[j] = (int8_t)st;
        a.ninliers[j] = st == ORBM_POSE_OK ? ninit - nbad : 0;
        s_cnt[3] = 0;
    }
    if (st != ORBM_POSE_OK && tid < 16) a.Tcw_out[16 * (long long)j + tid] = s_Tin[tid];
    __syncthreads();
    // mvbOutlier, and Tracking's discard loop after the call
    int kept = 0;
    for (int i = tid; i < n; i += kPoseThreads) {
        const int mp = a.mp_index[jb + i];
        if (mp < 0 || mp >= a.mrows) continue;
        const uint32_t o = st == ORBM_POSE_OK ? (s_lvl[i >> 5] >> (i & 31)) & 1u : 0u;
        a.outlier[jb + i] = (uint8_t)o;
        uint8_t fl = 8;
        if (a.mp_flags) {
            fl = (uint8_t)((a.mp_flags[jb + i] & ~4u) | (o << 2));
            a.mp_flags[jb + i] = fl;
        }
        if (o) {
            if (a.frame_mp) a.frame_mp[jb + i] = -1;
        } else if (fl & 8) {
            kept++;
        }
    }
    if (a.nmatches_map) {
        if (kept) atomicAdd(&s_cnt[3], kept);
        __syncthreads();
        if (tid == 0) a.nmatches_map[j] = s_cnt[3];
    }
}

__global__ void k_so3_selftest(const double* __restrict__ in, double* __restrict__ sn, double* __restrict__ cs,
                               double* __restrict__ sq, double* __restrict__ rc, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s, c;
    so3_sincos(in[i], &s, &c);
    sn[i] = s;
    cs[i] = c;
    sq[i] = __dsqrt_rn(in[i]);
    rc[i] = __ddiv_rn(1.0, in[i]);
}

}  // namespace

}  // namespace orbamd

int orbx_selftest_so3(const double* d_in, double* d_sin, double* d_cos, double* d_sqrt, double* d_rcp, int n,
                      void* stream) {
    if (!d_in || !d_sin || !d_cos || !d_sqrt || !d_rcp || n < 0) return ORBX_EARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(orbamd::k_so3_selftest, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_sin,
                       d_cos, d_sqrt, d_rcp, n);
    HIPR(hipGetLastError());
    return 0;
}

int orbm_pose_optimization_batch_device(
    orbm_ctx* ctx, int njobs, const int32_t* d_frame, int nframes, const orbx_kp* d_kps_un, const int32_t* d_counts,
    int kp_stride, const float* d_uright, const orbm_track_geom* geom, const float* inv_level_sigma2,
    const int32_t* d_mp_index, const float* d_pos, int mrows, const float* d_Tcw_in, float* d_Tcw_out,
    uint8_t* d_outlier, uint8_t* d_mp_flags, int32_t* d_frame_mp, int32_t* d_ninliers, int32_t* d_nmatches_map,
    int8_t* d_status, void* stream) {
    using namespace orbamd;
    if (!ctx || njobs < 0 || nframes < 1 || kp_stride < 1 || kp_stride > 65536 || mrows < 0 || !geom ||
        !inv_level_sigma2 || geom->nlevels < 1 || geom->nlevels > 16)
        return ORBX_EARG;
    if (njobs == 0) return 0;  // nothing to read: an empty job list may come with NULL arrays
    if (!d_frame || !d_kps_un || !d_counts || !d_mp_index || (mrows && !d_pos) || !d_Tcw_in || !d_Tcw_out ||
        !d_outlier || !d_ninliers || !d_status || ((uintptr_t)d_kps_un & 7) ||
        (long long)njobs * kp_stride > 0x7fffffffLL)
        return ORBX_EARG;
    HIPR(hipSetDevice(ctx->device));
    PoseArgs a;
    memset(&a, 0, sizeof(a));
    a.frame = d_frame;
    a.nframes = nframes;
    a.kps = d_kps_un;
    a.counts = d_counts;
    a.kp_stride = kp_stride;
    a.uright = d_uright;
    a.fx = geom->fx, a.fy = geom->fy, a.cx = geom->cx, a.cy = geom->cy, a.bf = geom->bf;
    a.nlevels = geom->nlevels;
    for (int k = 0; k < geom->nlevels; k++) a.inv_sigma2[k] = inv_level_sigma2[k];
    a.mp_index = d_mp_index;
    a.pos = d_pos;
    a.mrows = mrows;
    a.Tcw_in = d_Tcw_in;
    a.Tcw_out = d_Tcw_out;
    a.outlier = d_outlier;
    a.mp_flags = d_mp_flags;
    a.frame_mp = d_frame_mp;
    a.ninliers = d_ninliers;
    a.nmatches_map = d_nmatches_map;
    a.status = d_status;
    a.err = ctx->err.as<int32_t>();
    hipLaunchKernelGGL(k_pose_optimize, dim3(njobs), dim3(kPoseThreads), 0, (hipStream_t)stream, a);
    HIPR(hipGetLastError());
    return 0;
}

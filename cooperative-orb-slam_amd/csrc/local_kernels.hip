/*
 * local_kernels.hip -- local-map tracking over a device batch on gfx950: Frame::isInFrustum (Frame.cc:274-330) of a
 * table of MapPoints under every frame's pose, and Tracking::SearchLocalPoints (Tracking.cc:1143-1193) for every frame
 * of a batch: the two loops of the reference as two launches ordered by the stream, which fill one search call per
 * frame for the k_grid, k_proj_scan and k_proj_resolve kernels (frame_kernels.hip) that
 * ORBmatcher::SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:45-129) already runs on.
 *
 * The float arithmetic of one point is frame_math.h's frustum_point, shared by both frustum kernels; the device logf of
 * MapPoint::PredictScale is orb_math.h's.
 */
#include <hip/hip_runtime.h>

#include <cmath>

#include "frame_math.h"
#include "matcher_host.h"
#include "orbslam_amd_testing.h"

namespace orbamd {

namespace {

constexpr int kFrustumThreads = 256;
constexpr int kLocalThreads = 256;
constexpr int kErrLocalInput = 16;    // a d_frame_mp index >= M or a bad d_range
constexpr int kErrFrustumInput = 32;  // a point or pose the isInFrustum contract excludes

/* grid (ceil(M / kFrustumThreads), nframes), one lane per (point, frame) */
__global__ __launch_bounds__(kFrustumThreads) void k_frustum(orbm_track_geom g, float log_scale_factor, float cos_limit,
                                                             int M, const float* __restrict__ pos,
                                                             const float* __restrict__ normal,
                                                             const float* __restrict__ min_dist,
                                                             const float* __restrict__ max_dist,
                                                             const float* __restrict__ Tcw, uint8_t* in_view,
                                                             float* proj_x, float* proj_y, float* proj_xr,
                                                             int32_t* level, float* view_cos, int32_t* err) {
    const int f = blockIdx.y;
    const int m = blockIdx.x * kFrustumThreads + threadIdx.x;
    int rc = 0;
    if (m < M) {
        const FrustumPose p = frustum_pose(Tcw + 16 * (size_t)f);
        FrustumResult r;
        rc = frustum_point(g, log_scale_factor, p, cos_limit, pos + 3 * (size_t)m, normal + 3 * (size_t)m, min_dist[m],
                           max_dist[m], r);
        const size_t o = (size_t)f * M + m;
        in_view[o] = rc == 1;
        proj_x[o] = r.u;
        proj_y[o] = r.v;
        proj_xr[o] = r.xr;
        level[o] = r.level;
        view_cos[o] = r.view_cos;
    }
    if (__any(rc < 0) && (threadIdx.x & 63) == 0) atomicOr(err, kErrFrustumInput);
}

__global__ void k_logf_selftest(const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = logf_domain(in[i]) ? glibc_logf(in[i]) : __uint_as_float(0x7fc00000u);
}

/* frame f's slice [begin, end) of the table; false (an empty slice) when d_range gives one outside [0, M] */
__device__ __forceinline__ bool local_range(const LocalArgs& a, int f, int& begin, int& end) {
    begin = 0;
    end = a.M;
    if (a.range) {
        begin = a.range[2 * f];
        end = a.range[2 * f + 1];
        if (begin < 0 || end > a.M || begin > end) {
            begin = end = 0;
            return false;
        }
    }
    return true;
}

/* One workgroup per frame: the first loop of SearchLocalPoints (Tracking.cc:1146-1162) over the frame's features --
 * a bad MapPoint counts as none, any other is marked seen (mnLastFrameSeen) and occupies its feature iff it has
 * observations (ORBmatcher.cc:87-89) --, the frame's keypoints as the SoA arrays of ProjCall, and the call itself. The
 * queries (one per point of the slice, in table order) are written by k_local_frustum. */
__global__ __launch_bounds__(kLocalThreads) void k_local_prologue(LocalArgs a, int frame0) {
    const int f = frame0 + blockIdx.x, tid = threadIdx.x;
    const int S = a.kp_stride;
    uint8_t* const fs = a.frame_scratch + (long long)f * a.frame_bytes;
    int begin, end;
    const bool range_ok = local_range(a, f, begin, end);
    const int nq = end - begin;
    const int n = range_ok ? min(max(a.counts[f], 0), S) : 0;
    uint8_t* const seen = fs + a.o_seen;
    for (int j = tid; j < nq; j += kLocalThreads) seen[j] = 0;
    __syncthreads();
    const long long fb = (long long)f * S;
    float* const ox = (float*)(fs + a.o_x);
    float* const oy = (float*)(fs + a.o_y);
    int32_t* const oo = (int32_t*)(fs + a.o_oct);
    uint8_t* const occ = fs + a.o_occ;
    const uint2* kin = (const uint2*)(a.kps + fb);
    int idx_bad = 0;
    for (int i = tid; i < n; i += kLocalThreads) {
        // (x, y) (size, angle) (response, octave)
        const uint2 w0 = kin[3 * i], w2 = kin[3 * i + 2];
        ox[i] = __uint_as_float(w0.x);
        oy[i] = __uint_as_float(w0.y);
        oo[i] = (int32_t)w2.y;
        int mp = a.frame_mp[fb + i];
        if (mp >= a.M) {
            idx_bad = 1;
            mp = -1;
        }
        uint8_t o = 0;
        if (mp >= 0) {
            const int fl = a.mp_flags[mp];
            if (!(fl & 2)) {  // !isBad() (Tracking.cc:1151)
                if (mp >= begin && mp < end) seen[mp - begin] = 1;
                o = (fl & 8) != 0;
            }
        }
        occ[i] = o;
    }
    idx_bad = __syncthreads_or(idx_bad);
    if (!range_ok) {
        int32_t* m = a.match + fb;
        for (int i = tid; i < S; i += kLocalThreads) m[i] = -1;
    }
    if (tid == 0) {
        if (!range_ok || idx_bad) atomicOr(a.err, kErrLocalInput);
        a.ntomatch[f] = 0;
        ProjCall c = {};
        c.x = ox;
        c.y = oy;
        c.angle = nullptr;  // no rotation check in this variant
        c.uright = a.uright ? a.uright + fb : nullptr;
        c.octave = oo;
        c.occ0 = occ;
        c.desc = a.desc + fb * 32;
        c.n = n;
        c.min_x = a.g.min_x;
        c.min_y = a.g.min_y;
        c.gw_inv = a.g.grid_w_inv;
        c.gh_inv = a.g.grid_h_inv;
        c.q = (const ProjQuery*)(fs + a.o_q);
        c.qdesc = a.mp_desc + (long long)begin * 32;
        c.nq = nq;
        c.accept_th = 100;  // TH_HIGH (ORBmatcher.cc:118)
        c.ratio = 1;
        c.nnratio = a.nnratio;
        c.check_ori = 0;
        c.grid_start = (int*)(fs + a.o_gs);
        c.grid_idx = (uint16_t*)(fs + a.o_gi);
        c.scan = (unsigned long long*)(fs + a.o_scan);
        c.scan_cnt = (int*)(fs + a.o_scnt);
        c.res = (int*)(fs + a.o_res);
        c.match = a.match + fb;
        c.nmatches = a.nmatches + f;
        c.direct = 0;
        c.n_out = n;
        c.host_out = nullptr;
        c.seq = 0;
        a.calls[f] = c;
    }
}

/* grid (ceil(M / kLocalThreads), nframes), one lane per (table point, frame): the second loop of SearchLocalPoints
 * (Tracking.cc:1167-1180) and the per-MapPoint head of SearchByProjection (ORBmatcher.cc:51-69). Query m - begin is
 * table point m: a point that is seen, bad or outside the frustum stays in the array as a query with an empty window
 * (what k_proj_scan gives its padding lanes), so the queries reach the in-order resolve in table order with q.src = m
 * and the query descriptors are the table's descriptor rows in place. */
__global__ __launch_bounds__(kLocalThreads) void k_local_frustum(LocalArgs a, int frame0) {
    __shared__ float s_scale[kMaxLevels];
    const int f = frame0 + blockIdx.y, tid = threadIdx.x;
    if (tid < kMaxLevels) s_scale[tid] = a.g.scale_factors[tid];
    __syncthreads();
    const int m = blockIdx.x * kLocalThreads + tid;
    int begin, end;
    local_range(a, f, begin, end);
    const uint8_t* const fs = a.frame_scratch + (long long)f * a.frame_bytes;
    int rc = 0;
    if (m < a.M) {
        const bool inside = m >= begin && m < end;
        if (inside) {
            ProjQuery q;
            q.u = q.v = -1e30f;  // empty window
            q.radius = 0.f;
            q.min_level = 0;
            q.max_level = -1;
            q.ur = 0.f;
            q.er_th = 0.f;
            q.angle = 0.f;
            q.flags = 0;
            q.src = m;
            const int fl = a.mp_flags[m];
            if (!fs[a.o_seen + (m - begin)] && !(fl & 2)) {  // Tracking.cc:1170-1173
                const FrustumPose p = frustum_pose(a.Tcw + 16 * (long long)f);
                FrustumResult r;
                rc = frustum_point(a.g, a.log_scale_factor, p, a.cos_limit, a.pos + 3 * (long long)m,
                                   a.normal + 3 * (long long)m, a.min_dist[m], a.max_dist[m], r);
                if (rc == 1) {
                    float rad = (double)r.view_cos > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos (:131-137)
                    if (a.th != 1.0f) rad = __fmul_rn(rad, a.th);           // bFactor (:49, 65-66)
                    const float radius = __fmul_rn(rad, s_scale[r.level]);
                    q.u = r.u;
                    q.v = r.v;
                    q.radius = radius;
                    q.min_level = r.level - 1;
                    q.max_level = r.level;
                    q.ur = r.xr;
                    q.er_th = radius;
                    q.flags = kProjValid | kProjStereo | ((fl & 8) ? kProjClaims : 0);
                }
            }
            ((ProjQuery*)(fs + a.o_q))[m - begin] = q;
        }
        if (a.in_view) a.in_view[(long long)f * a.M + m] = rc == 1;
    }
    const unsigned long long in = __ballot(rc == 1);
    const bool excluded = __any(rc < 0);
    if ((tid & 63) == 0) {
        if (in) atomicAdd(a.ntomatch + f, __popcll(in));
        if (excluded) atomicOr(a.err, kErrFrustumInput);
    }
}

}  // namespace

hipError_t launch_frustum(const orbm_track_geom& g, float log_scale_factor, float cos_limit, int M, const float* pos,
                          const float* normal, const float* min_dist, const float* max_dist, int nframes,
                          const float* Tcw, uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr,
                          int32_t* level, float* view_cos, int32_t* err, hipStream_t st) {
    const dim3 grid((M + kFrustumThreads - 1) / kFrustumThreads, nframes);
    hipLaunchKernelGGL(k_frustum, grid, dim3(kFrustumThreads), 0, st, g, log_scale_factor, cos_limit, M, pos, normal,
                       min_dist, max_dist, Tcw, in_view, proj_x, proj_y, proj_xr, level, view_cos, err);
    return hipGetLastError();
}

hipError_t launch_local_points(const LocalArgs& a, int frame0, int nframes, hipStream_t st) {
    hipLaunchKernelGGL(k_local_prologue, dim3(nframes), dim3(kLocalThreads), 0, st, a, frame0);
    if (a.M > 0) {
        const dim3 grid((a.M + kLocalThreads - 1) / kLocalThreads, nframes);
        hipLaunchKernelGGL(k_local_frustum, grid, dim3(kLocalThreads), 0, st, a, frame0);
    }
    return hipGetLastError();
}

}  // namespace orbamd

int orbx_selftest_logf(const float* d_in, float* d_out, int n, void* stream) {
    if (!d_in || !d_out || n < 0) return ORBX_EARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(orbamd::k_logf_selftest, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_out,
                       n);
    HIPR(hipGetLastError());
    return 0;
}

static bool track_geom_ok(const orbm_track_geom* g, float log_scale_factor, float cos_limit) {
    return g && g->nlevels >= 1 && g->nlevels <= 16 && log_scale_factor > 0 && std::isfinite(log_scale_factor) &&
           std::isfinite(cos_limit);
}

int orbx_is_in_frustum_batch_device(orbm_ctx* ctx, const orbm_track_geom* geom, float log_scale_factor,
                                    float viewing_cos_limit, int M, const float* d_pos, const float* d_normal,
                                    const float* d_min_dist, const float* d_max_dist, int nframes, const float* d_Tcw,
                                    uint8_t* d_in_view, float* d_proj_x, float* d_proj_y, float* d_proj_xr,
                                    int32_t* d_level, float* d_view_cos, void* stream) {
    if (!ctx || !track_geom_ok(geom, log_scale_factor, viewing_cos_limit) || M < 0 || nframes < 0 || nframes > 65535)
        return ORBX_EARG;
    if (M == 0 || nframes == 0) return 0;
    if (!d_pos || !d_normal || !d_min_dist || !d_max_dist || !d_Tcw || !d_in_view || !d_proj_x || !d_proj_y ||
        !d_proj_xr || !d_level || !d_view_cos)
        return ORBX_EARG;
    HIPR(hipSetDevice(ctx->device));
    HIPR(orbamd::launch_frustum(*geom, log_scale_factor, viewing_cos_limit, M, d_pos, d_normal, d_min_dist, d_max_dist,
                                nframes, d_Tcw, d_in_view, d_proj_x, d_proj_y, d_proj_xr, d_level, d_view_cos,
                                ctx->err.as<int32_t>(), (hipStream_t)stream));
    return 0;
}

int orbm_search_local_points_batch_device(
    orbm_ctx* ctx, int nframes, const orbx_kp* d_kps_un, const uint8_t* d_desc, const int32_t* d_counts, int kp_stride,
    const float* d_uright, const float* d_Tcw, const orbm_track_geom* geom, float log_scale_factor, int M,
    const float* d_pos, const float* d_normal, const float* d_min_dist, const float* d_max_dist,
    const uint8_t* d_mp_desc, const uint8_t* d_mp_flags, const int32_t* d_range, const int32_t* d_frame_mp, float th,
    float nnratio, float viewing_cos_limit, int32_t* d_match, int32_t* d_nmatches, int32_t* d_ntomatch,
    uint8_t* d_in_view, void* stream) {
    using namespace orbamd;
    if (!ctx || nframes < 0 || kp_stride < 1 || kp_stride > 65536 || M < 0 ||
        !track_geom_ok(geom, log_scale_factor, viewing_cos_limit))
        return ORBX_EARG;
    if (nframes == 0) return 0;  // nothing to read: an empty batch may come with NULL arrays
    if (!d_kps_un || !d_desc || !d_counts || !d_Tcw || !d_frame_mp || !d_match || !d_nmatches || !d_ntomatch ||
        (M && (!d_pos || !d_normal || !d_min_dist || !d_max_dist || !d_mp_desc || !d_mp_flags)) ||
        ((uintptr_t)d_kps_un & 7) || ((uintptr_t)d_desc & 15) || ((uintptr_t)d_mp_desc & 15))
        return ORBX_EARG;
    HIPR(hipSetDevice(ctx->device));
    const size_t S = (size_t)kp_stride, Mz = (size_t)M;
    LocalArgs a;
    memset(&a, 0, sizeof(a));
    Carve fc;  // one frame's scratch: its SoA keypoints and occupancy, the seen marks, the queries, the search's arrays
    a.o_x = (long long)fc.take(4 * S);
    a.o_y = (long long)fc.take(4 * S);
    a.o_oct = (long long)fc.take(4 * S);
    a.o_occ = (long long)fc.take(S);
    a.o_seen = (long long)fc.take(Mz);
    a.o_q = (long long)fc.take(sizeof(ProjQuery) * Mz);
    a.o_gs = (long long)fc.take(4 * (kGridCols * kGridRows + 1));
    a.o_gi = (long long)fc.take(2 * S);
    a.o_scan = (long long)fc.take(8 * (size_t)proj_topk() * Mz);
    a.o_scnt = (long long)fc.take(4 * Mz);
    a.o_res = (long long)fc.take(8 * Mz);
    a.frame_bytes = (long long)fc.off;
    Carve cv;
    const size_t o_calls = cv.take(sizeof(ProjCall) * (size_t)nframes);
    const size_t o_frames = cv.take(fc.off * (size_t)nframes);
    if (ctx->scratch.ensure(cv.off)) return ORBX_EDEVICE;
    uint8_t* base = ctx->scratch.as<uint8_t>();
    a.kps = d_kps_un;
    a.desc = d_desc;
    a.counts = d_counts;
    a.kp_stride = kp_stride;
    a.uright = d_uright;
    a.Tcw = d_Tcw;
    a.g = *geom;
    a.log_scale_factor = log_scale_factor;
    a.M = M;
    a.pos = d_pos;
    a.normal = d_normal;
    a.min_dist = d_min_dist;
    a.max_dist = d_max_dist;
    a.mp_desc = d_mp_desc;
    a.mp_flags = d_mp_flags;
    a.range = d_range;
    a.frame_mp = d_frame_mp;
    a.th = th;
    a.nnratio = nnratio;
    a.cos_limit = viewing_cos_limit;
    a.match = d_match;
    a.nmatches = d_nmatches;
    a.ntomatch = d_ntomatch;
    a.in_view = d_in_view;
    a.err = ctx->err.as<int32_t>();
    a.calls = (ProjCall*)(base + o_calls);
    a.frame_scratch = base + o_frames;
    hipStream_t st = (hipStream_t)stream;
    constexpr int kMaxCalls = 32768;  // gridDim.y of k_proj_scan
    for (int f0 = 0; f0 < nframes; f0 += kMaxCalls) {
        const int nf = std::min(kMaxCalls, nframes - f0);
        HIPR(launch_local_points(a, f0, nf, st));
        HIPR(launch_projection(a.calls + f0, nf, M, st));
    }
    return 0;
}

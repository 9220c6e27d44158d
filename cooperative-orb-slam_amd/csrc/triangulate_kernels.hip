/*
 * triangulate_kernels.hip -- new MapPoints from triangulation matches over a device batch on gfx950: the per-match body
 * of LocalMapping::CreateNewMapPoints (LocalMapping.cc:284-450) with its per-pair baseline test (:244-261) and
 * MapPoint::UpdateNormalAndDepth (MapPoint.cc:330-371), from the match rows the batch matchers leave in HBM to a table
 * of MapPoints in the row format orbm_search_local_points_batch_device reads.
 *
 * The float arithmetic of one match is frame_math.h's triangulate_match; the device atan2f and cosf of
 * cosParallaxStereo are orb_math.h's. One launch, one workgroup per pair, no host step.
 */
#include <hip/hip_runtime.h>

#include "frame_math.h"
#include "matcher_host.h"
#include "orbslam_amd_testing.h"

namespace orbamd {

namespace {

constexpr int kTriThreads = 256;
constexpr int kTriWaves = kTriThreads / 64;
constexpr int kErrTriPair = 64;   // a frame index outside the batch or a count above kp_stride
constexpr int kErrTriInput = 128;  // a row the CreateNewMapPoints contract excludes

struct TriArgs {
    const int32_t *q1, *q2;
    int nframes;
    const orbx_kp* kps;
    const int32_t* counts;
    int kp_stride;
    const float *uright, *depth;
    const uint8_t* desc;
    const float* Tcw;
    const int32_t* match12;
    orbm_tri_geom g;
    int monocular;
    const float* median_depth2;
    int8_t* status;
    float *pos3, *tab_pos, *tab_normal, *tab_min_dist, *tab_max_dist;
    uint8_t *tab_desc, *tab_flags;
    int32_t *tab_feat1, *tab_feat2, *new_range, *nnew, *err;
};

/* One workgroup per pair. The row of the current keyframe is walked in chunks of kTriThreads features, one lane per
 * feature; the created points of a chunk get consecutive table rows in feature order from the wave's ballot, the
 * prefix over the chunk's waves and the running base of the chunks before, so the table keeps the reference's creation
 * order whatever the schedule. */
__global__ __launch_bounds__(kTriThreads) void k_create_map_points(TriArgs a) {
    __shared__ float s_sf[kMaxLevels], s_sigma2[kMaxLevels];
    __shared__ float s_pose[2][16];  // rows 0..2 of mTcw, then mOw, of the two keyframes
    __shared__ int s_wave[kTriWaves];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.kp_stride;
    const long long pb = (long long)p * S;
    if (tid < kMaxLevels) {
        s_sf[tid] = a.g.scale_factors[tid];
        s_sigma2[tid] = a.g.level_sigma2[tid];
    }
    const int f1 = a.q1[p], f2 = a.q2[p];
    bool bad = (unsigned)f1 >= (unsigned)a.nframes || (unsigned)f2 >= (unsigned)a.nframes;
    int n1 = 0, n2 = 0;
    if (!bad) {
        n1 = max(a.counts[f1], 0);
        n2 = max(a.counts[f2], 0);
        bad = n1 > S || n2 > S;
    }
    if (bad) {  // uniform: nothing of the frames is read
        for (int i = tid; i < S; i += kTriThreads) {
            a.status[pb + i] = ORBM_TRI_NO_MATCH;
            a.pos3[(pb + i) * 3] = a.pos3[(pb + i) * 3 + 1] = a.pos3[(pb + i) * 3 + 2] = 0.0f;
        }
        if (tid == 0) {
            a.nnew[p] = 0;
            a.new_range[2 * p] = a.new_range[2 * p + 1] = (int32_t)pb;
            atomicOr(a.err, kErrTriPair);
        }
        return;
    }
    bool pose_ok, skip = false;
    {
        const FrustumPose p1 = frustum_pose(a.Tcw + 16 * (long long)f1);
        const FrustumPose p2 = frustum_pose(a.Tcw + 16 * (long long)f2);
        pose_ok = p1.ok && p2.ok;
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 15; k++) {
                s_pose[0][k] = k < 12 ? p1.T[k] : p1.Ow[k - 12];
                s_pose[1][k] = k < 12 ? p2.T[k] : p2.Ow[k - 12];
            }
        }
        if (pose_ok) {  // LocalMapping.cc:244-261
            const float v0 = __fsub_rn(p2.Ow[0], p1.Ow[0]), v1 = __fsub_rn(p2.Ow[1], p1.Ow[1]),
                        v2 = __fsub_rn(p2.Ow[2], p1.Ow[2]);
            const float baseline = __double2float_rn(__dsqrt_rn(dot3_d(v0, v1, v2, v0, v1, v2)));
            if (!a.monocular)
                skip = baseline < a.g.b;
            else
                skip = (double)__fdiv_rn(baseline, a.median_depth2[p]) < 0.01;
        }
    }
    __syncthreads();
    const long long b1 = (long long)f1 * S, b2 = (long long)f2 * S;
    const uint2* k1 = (const uint2*)(a.kps + b1);
    const uint2* k2 = (const uint2*)(a.kps + b2);
    int base = 0, excluded = 0;
    for (int c0 = 0; c0 < n1; c0 += kTriThreads) {
        const int i = c0 + tid;
        int st = ORBM_TRI_NO_MATCH, idx2 = -1;
        TriPoint r;
        r.x[0] = r.x[1] = r.x[2] = r.normal[0] = r.normal[1] = r.normal[2] = r.min_dist = r.max_dist = 0.0f;
        if (i < n1) {
            idx2 = a.match12[pb + i];
            if (idx2 >= 0) {
                if (!pose_ok || idx2 >= n2) {
                    st = ORBM_TRI_EXCLUDED;
                } else if (skip) {
                    st = ORBM_TRI_BASELINE;
                } else {
                    // (x, y) (size, angle) (response, octave)
                    const uint2 w1 = k1[3 * i], o1 = k1[3 * i + 2], w2 = k2[3 * idx2], o2 = k2[3 * idx2 + 2];
                    const float ur1 = a.uright ? a.uright[b1 + i] : -1.0f, d1 = a.uright ? a.depth[b1 + i] : -1.0f;
                    const float ur2 = a.uright ? a.uright[b2 + idx2] : -1.0f,
                                d2 = a.uright ? a.depth[b2 + idx2] : -1.0f;
                    st = triangulate_match(a.g, s_sf, s_sigma2, s_pose[0], s_pose[0] + 12, s_pose[1], s_pose[1] + 12,
                                           __uint_as_float(w1.x), __uint_as_float(w1.y),
                                           (int)o1.y, ur1, d1, __uint_as_float(w2.x), __uint_as_float(w2.y), (int)o2.y,
                                           ur2, d2, r);
                }
            }
        }
        const bool created = st >= ORBM_TRI_TRIANGULATED && st <= ORBM_TRI_STEREO2;
        excluded |= st == ORBM_TRI_EXCLUDED;
        if (i < n1) {
            a.status[pb + i] = (int8_t)st;
            a.pos3[(pb + i) * 3] = created ? r.x[0] : 0.0f;
            a.pos3[(pb + i) * 3 + 1] = created ? r.x[1] : 0.0f;
            a.pos3[(pb + i) * 3 + 2] = created ? r.x[2] : 0.0f;
        }
        const unsigned long long m = __ballot(created);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kTriWaves; w++) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (created) {
            const long long row = pb + base + before + __popcll(m & ((1ull << lane) - 1));
            a.tab_pos[row * 3] = r.x[0];
            a.tab_pos[row * 3 + 1] = r.x[1];
            a.tab_pos[row * 3 + 2] = r.x[2];
            a.tab_normal[row * 3] = r.normal[0];
            a.tab_normal[row * 3 + 1] = r.normal[1];
            a.tab_normal[row * 3 + 2] = r.normal[2];
            a.tab_min_dist[row] = r.min_dist;
            a.tab_max_dist[row] = r.max_dist;
            a.tab_flags[row] = 9;  // a MapPoint with Observations() > 0
            a.tab_feat1[row] = i;
            a.tab_feat2[row] = idx2;
            // the current keyframe's descriptor (DESIGN.md "Pinned semantics")
            const uint4* src = (const uint4*)(a.desc + (b1 + i) * 32);
            uint4* dst = (uint4*)(a.tab_desc + row * 32);
            dst[0] = src[0];
            dst[1] = src[1];
        }
        base += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (__any(excluded) && lane == 0) atomicOr(a.err, kErrTriInput);
    if (tid == 0) {
        a.nnew[p] = base;
        a.new_range[2 * p] = (int32_t)pb;
        a.new_range[2 * p + 1] = (int32_t)(pb + base);
    }
}

__global__ void k_atan2f_selftest(const float* __restrict__ y, const float* __restrict__ x, float* __restrict__ at,
                                  float* __restrict__ cs, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = __uint_as_float(0x7fc00000u), c = a, s;
    if (atan2f_domain(y[i], x[i])) {
        a = glibc_atan2f(y[i], x[i]);
        glibc_sincosf(__fmul_rn(2.0f, a), &s, &c);
    }
    at[i] = a;
    cs[i] = c;
}

}  // namespace

}  // namespace orbamd

int orbx_selftest_atan2f(const float* d_y, const float* d_x, float* d_atan, float* d_cos, int n, void* stream) {
    if (!d_y || !d_x || !d_atan || !d_cos || n < 0) return ORBX_EARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(orbamd::k_atan2f_selftest, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_y, d_x,
                       d_atan, d_cos, n);
    HIPR(hipGetLastError());
    return 0;
}

int orbm_create_new_map_points_batch_device(
    orbm_ctx* ctx, int npairs, const int32_t* d_q1, const int32_t* d_q2, int nframes, const orbx_kp* d_kps_un,
    const int32_t* d_counts, int kp_stride, const float* d_uright, const float* d_depth, const uint8_t* d_desc,
    const float* d_Tcw, const int32_t* d_match12, const orbm_tri_geom* geom, int monocular,
    const float* d_median_depth2, int8_t* d_status, float* d_pos3, float* d_tab_pos, float* d_tab_normal,
    float* d_tab_min_dist, float* d_tab_max_dist, uint8_t* d_tab_desc, uint8_t* d_tab_flags, int32_t* d_tab_feat1,
    int32_t* d_tab_feat2, int32_t* d_new_range, int32_t* d_nnew, void* stream) {
    using namespace orbamd;
    if (!ctx || npairs < 0 || nframes < 1 || kp_stride < 1 || kp_stride > 65536 || !geom || geom->nlevels < 1 ||
        geom->nlevels > 16 || geom->fx == 0 || geom->fy == 0)
        return ORBX_EARG;
    if (npairs == 0) return 0;  // nothing to read: an empty pair list may come with NULL arrays
    if (!d_q1 || !d_q2 || !d_kps_un || !d_counts || !d_desc || !d_Tcw || !d_match12 || !d_status || !d_pos3 ||
        !d_tab_pos || !d_tab_normal || !d_tab_min_dist || !d_tab_max_dist || !d_tab_desc || !d_tab_flags ||
        !d_tab_feat1 || !d_tab_feat2 || !d_new_range || !d_nnew || (monocular && !d_median_depth2) ||
        (!d_uright) != (!d_depth) || ((uintptr_t)d_kps_un & 7) || ((uintptr_t)d_desc & 15) ||
        ((uintptr_t)d_tab_desc & 15) || (long long)npairs * kp_stride > 0x7fffffffLL)
        return ORBX_EARG;
    HIPR(hipSetDevice(ctx->device));
    TriArgs a;
    memset(&a, 0, sizeof(a));
    a.q1 = d_q1;
    a.q2 = d_q2;
    a.nframes = nframes;
    a.kps = d_kps_un;
    a.counts = d_counts;
    a.kp_stride = kp_stride;
    a.uright = d_uright;
    a.depth = d_depth;
    a.desc = d_desc;
    a.Tcw = d_Tcw;
    a.match12 = d_match12;
    a.g = *geom;
    a.monocular = monocular ? 1 : 0;
    a.median_depth2 = d_median_depth2;
    a.status = d_status;
    a.pos3 = d_pos3;
    a.tab_pos = d_tab_pos;
    a.tab_normal = d_tab_normal;
    a.tab_min_dist = d_tab_min_dist;
    a.tab_max_dist = d_tab_max_dist;
    a.tab_desc = d_tab_desc;
    a.tab_flags = d_tab_flags;
    a.tab_feat1 = d_tab_feat1;
    a.tab_feat2 = d_tab_feat2;
    a.new_range = d_new_range;
    a.nnew = d_nnew;
    a.err = ctx->err.as<int32_t>();
    hipLaunchKernelGGL(k_create_map_points, dim3(npairs), dim3(kTriThreads), 0, (hipStream_t)stream, a);
    HIPR(hipGetLastError());
    return 0;
}

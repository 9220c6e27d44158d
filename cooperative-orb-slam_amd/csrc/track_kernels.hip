/*
 * track_kernels.hip -- frame-to-frame tracking over a device batch on gfx950: Frame::UnprojectStereo (Frame.cc:667-681)
 * of every keypoint, and the prologue of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
 * (ORBmatcher.cc:1328-1470) for a batch of frame pairs, which turns device-resident frames into the ProjCall /
 * ProjQuery arrays that k_grid, k_proj_scan and k_proj_resolve (frame_kernels.hip) already take, one call per pair.
 *
 * cv::Mat's float arithmetic as pinned in DESIGN.md "Pinned semantics", every operation stated with a rounding
 * intrinsic so that nothing contracts: the small-matrix gemm (a row's float products summed in float, the addend
 * joined in double, one rounding), the GEMM_1_T path (double accumulation from 0, one rounding) and the correctly
 * rounded fp64 divide. The same sequences on the host: unproject.c and projection.cpp
 * (orbm_search_by_projection_last_frame); in Python: tests/unproject_py.py.
 */
#include <hip/hip_runtime.h>

#include "extract_host.h"
#include "frame_math.h"
#include "matcher_host.h"

namespace orbamd {

namespace {

constexpr int kUnprojectThreads = 256;
constexpr int kTrackThreads = 256;

/* grid (ceil(kp_stride / kUnprojectThreads), nframes), one lane per keypoint. The first 8 bytes of the 24-byte
 * orbx_kp record are (x, y). */
__global__ __launch_bounds__(kUnprojectThreads) void k_unproject(float cx, float cy, float invfx, float invfy,
                                                                 const float2* __restrict__ kps,
                                                                 const float* __restrict__ depth,
                                                                 const int32_t* __restrict__ counts, int kp_stride,
                                                                 const float* __restrict__ Tcw,
                                                                 float* __restrict__ pos, uint8_t* mp_flags,
                                                                 int valid_flags) {
    const int f = blockIdx.y;
    const int i = blockIdx.x * kUnprojectThreads + threadIdx.x;
    const int n = min(counts[f], kp_stride);
    if (i >= n) return;
    const float* T = Tcw + 16 * (size_t)f;
    const size_t rec = (size_t)f * kp_stride + i;
    const float2 uv = kps[rec * 3];
    const float z = depth[rec];
    const bool valid = z > 0;
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (valid) {
        const float t0 = T[3], t1 = T[7], t2 = T[11];
        const float Ow[3] = {gemm_t_neg(T, 0, t0, t1, t2), gemm_t_neg(T, 1, t0, t1, t2), gemm_t_neg(T, 2, t0, t1, t2)};
        unproject_point(cx, cy, invfx, invfy, T, Ow, uv.x, uv.y, z, p);
    }
    pos[rec * 3] = p[0];
    pos[rec * 3 + 1] = p[1];
    pos[rec * 3 + 2] = p[2];
    if (mp_flags) mp_flags[rec] = valid ? (uint8_t)valid_flags : (uint8_t)0;
}

/* One workgroup per frame pair: ORBmatcher.cc:1339-1405 up to the GetFeaturesInArea call, as
 * orbm_search_by_projection_last_frame (projection.cpp) states it. Query i is the last frame's feature i: a feature
 * the reference skips or rejects stays in the array as a query with an empty window (what k_proj_scan gives its
 * padding lanes), so the queries keep the reference's order, q.src = i and the query descriptors are the last
 * frame's descriptor rows in place. The current frame's keypoints are written as the SoA arrays of ProjCall. */
__global__ __launch_bounds__(kTrackThreads) void k_track_prologue(TrackArgs a, int pair0) {
    __shared__ float s_scale[kMaxLevels];
    const int p = pair0 + blockIdx.x, tid = threadIdx.x;
    if (tid < kMaxLevels) s_scale[tid] = a.g.scale_factors[tid];
    __syncthreads();
    const int S = a.kp_stride;
    uint8_t* const ps = a.pair_scratch + (long long)p * a.pair_bytes;
    ProjQuery* const oq = (ProjQuery*)(ps + a.o_q);
    int cur = a.cur[p], last = a.last[p];
    bool bad = (unsigned)cur >= (unsigned)a.nframes || (unsigned)last >= (unsigned)a.nframes;
    if (bad) cur = last = 0;  // nothing of them is read
    int ncur = 0, nl = 0;
    if (!bad) {
        ncur = min(max(a.counts[cur], 0), S);
        nl = max(a.counts[last], 0);
        if (nl > S) {
            bad = true;
            nl = 0;
        }
    }
    const long long cb = (long long)cur * S, lb = (long long)last * S;
    int oct_bad = 0;
    if (!bad) {
        const float* Tc = a.Tcw + 16 * (long long)cur;
        const float* Tl = a.Tcw + 16 * (long long)last;
        const float tc0 = Tc[3], tc1 = Tc[7], tc2 = Tc[11];
        // twc = -Rcw.t() * tcw, tlc = Rlw * twc + tlw (ORBmatcher.cc:1339-1348); only tlc.z is used
        const float twc0 = gemm_t_neg(Tc, 0, tc0, tc1, tc2), twc1 = gemm_t_neg(Tc, 1, tc0, tc1, tc2),
                    twc2 = gemm_t_neg(Tc, 2, tc0, tc1, tc2);
        const float tlcz = gemm_row(Tl[8], Tl[9], Tl[10], twc0, twc1, twc2, Tl[11]);
        const bool bForward = tlcz > a.g.b && !a.mono;
        const bool bBackward = -tlcz > a.g.b && !a.mono;
        const float r00 = Tc[0], r01 = Tc[1], r02 = Tc[2], r10 = Tc[4], r11 = Tc[5], r12 = Tc[6], r20 = Tc[8],
                    r21 = Tc[9], r22 = Tc[10];
        for (int i = tid; i < nl; i += kTrackThreads) {
            ProjQuery q;
            q.u = q.v = -1e30f;  // empty window
            q.radius = 0.f;
            q.min_level = 0;
            q.max_level = -1;
            q.ur = 0.f;
            q.er_th = 0.f;
            q.angle = 0.f;
            q.flags = 0;
            q.src = i;
            const int fl = a.mp_flags[lb + i];
            if ((fl & 1) && !(fl & 4)) {  // pMP && !LastFrame.mvbOutlier[i] (:1355-1359)
                const float* P = a.pos + (lb + i) * 3;
                const float X = P[0], Y = P[1], Z = P[2];
                const float xc = gemm_row(r00, r01, r02, X, Y, Z, tc0);
                const float yc = gemm_row(r10, r11, r12, X, Y, Z, tc1);
                const float zc = gemm_row(r20, r21, r22, X, Y, Z, tc2);
                const float invzc = __double2float_rn(__ddiv_rn(1.0, (double)zc));
                const float u = __fadd_rn(__fmul_rn(__fmul_rn(a.g.fx, xc), invzc), a.g.cx);
                const float v = __fadd_rn(__fmul_rn(__fmul_rn(a.g.fy, yc), invzc), a.g.cy);
                const bool out = invzc < 0 || u < a.g.min_x || u > a.g.max_x || v < a.g.min_y || v > a.g.max_y;
                if (!out) {
                    const orbx_kp* k = a.kps + lb + i;
                    const int oct = k->octave;  // LastFrame.mvKeys[i].octave (:1378)
                    if ((unsigned)oct >= (unsigned)a.g.nlevels) {
                        oct_bad = 1;
                    } else {
                        const float radius = __fmul_rn(a.th, s_scale[oct]);
                        q.u = u;
                        q.v = v;
                        q.radius = radius;
                        q.min_level = bForward ? oct : bBackward ? 0 : oct - 1;
                        q.max_level = bForward ? -1 : bBackward ? oct : oct + 1;
                        q.ur = __fsub_rn(u, __fmul_rn(a.g.bf, invzc));
                        q.er_th = radius;
                        q.angle = k->angle;
                        q.flags = kProjValid | kProjStereo | ((fl & 8) ? kProjClaims : 0);
                    }
                }
            }
            oq[i] = q;
        }
        float* const ox = (float*)(ps + a.o_x);
        float* const oy = (float*)(ps + a.o_y);
        float* const oa = (float*)(ps + a.o_ang);
        int32_t* const oo = (int32_t*)(ps + a.o_oct);
        const uint2* kin = (const uint2*)(a.kps + cb);
        for (int i = tid; i < ncur; i += kTrackThreads) {
            // (x, y) (size, angle) (response, octave)
            const uint2 w0 = kin[3 * i], w1 = kin[3 * i + 1], w2 = kin[3 * i + 2];
            ox[i] = __uint_as_float(w0.x);
            oy[i] = __uint_as_float(w0.y);
            oa[i] = __uint_as_float(w1.y);
            oo[i] = (int32_t)w2.y;
        }
    }
    oct_bad = __syncthreads_or(oct_bad);
    const bool fail = bad || oct_bad;
    if (fail) {
        int32_t* m = a.match + (long long)p * S;
        for (int i = tid; i < S; i += kTrackThreads) m[i] = -1;
        if (tid == 0) atomicOr(a.err, bad ? 2 : 4);
    }
    if (tid == 0) {
        ProjCall c = {};
        c.x = (const float*)(ps + a.o_x);
        c.y = (const float*)(ps + a.o_y);
        c.angle = (const float*)(ps + a.o_ang);
        c.uright = a.uright ? a.uright + cb : nullptr;
        c.octave = (const int32_t*)(ps + a.o_oct);
        c.occ0 = a.occupied ? a.occupied + cb : nullptr;
        c.desc = a.desc + cb * 32;
        c.n = fail ? 0 : ncur;
        c.min_x = a.g.min_x;
        c.min_y = a.g.min_y;
        c.gw_inv = a.g.grid_w_inv;
        c.gh_inv = a.g.grid_h_inv;
        c.q = oq;
        c.qdesc = a.desc + lb * 32;
        c.nq = fail ? 0 : nl;
        c.accept_th = 100;  // TH_HIGH (ORBmatcher.cc:1413)
        c.ratio = 0;
        c.nnratio = 0.f;
        c.check_ori = a.check_ori;
        c.grid_start = (int*)(ps + a.o_gs);
        c.grid_idx = (uint16_t*)(ps + a.o_gi);
        c.scan = (unsigned long long*)(ps + a.o_scan);
        c.scan_cnt = (int*)(ps + a.o_scnt);
        c.res = (int*)(ps + a.o_res);
        c.match = a.match + (long long)p * S;
        c.nmatches = a.nmatches + p;
        c.direct = 0;
        c.n_out = c.n;
        c.host_out = nullptr;
        c.seq = 0;
        a.calls[p] = c;
    }
}

}  // namespace

hipError_t launch_unproject(float cx, float cy, float invfx, float invfy, int nframes, const orbx_kp* kps_un,
                            const float* depth, const int32_t* counts, int kp_stride, const float* Tcw, float* pos,
                            uint8_t* mp_flags, int valid_flags, hipStream_t st) {
    const dim3 grid((kp_stride + kUnprojectThreads - 1) / kUnprojectThreads, nframes);
    hipLaunchKernelGGL(k_unproject, grid, dim3(kUnprojectThreads), 0, st, cx, cy, invfx, invfy, (const float2*)kps_un,
                       depth, counts, kp_stride, Tcw, pos, mp_flags, valid_flags);
    return hipGetLastError();
}

hipError_t launch_track_prologue(const TrackArgs& a, int pair0, int npairs, hipStream_t st) {
    hipLaunchKernelGGL(k_track_prologue, dim3(npairs), dim3(kTrackThreads), 0, st, a, pair0);
    return hipGetLastError();
}

}  // namespace orbamd

int orbx_unproject_stereo_batch_device(orbx_handle* h, const orbx_camera* cam, int nframes, const orbx_kp* d_kps_un,
                                       const float* d_depth, const int32_t* d_counts, int kp_stride,
                                       const float* d_Tcw, float* d_pos, uint8_t* d_mp_flags, int valid_flags,
                                       void* stream) {
    if (!h || !cam || cam->fx == 0 || cam->fy == 0 || nframes < 0 || nframes > 65535 || kp_stride < 1 || !d_kps_un ||
        !d_depth || !d_counts || !d_Tcw || !d_pos || ((uintptr_t)d_kps_un & 7))
        return ORBX_EARG;
    if (nframes == 0) return 0;
    HIPR(hipSetDevice(h->device));
    // Frame.cc:104-105: invfx = 1.0f / fx, in float, once per camera
    HIPR(orbamd::launch_unproject(cam->cx, cam->cy, 1.0f / cam->fx, 1.0f / cam->fy, nframes, d_kps_un, d_depth,
                                  d_counts, kp_stride, d_Tcw, d_pos, d_mp_flags, valid_flags, (hipStream_t)stream));
    return 0;
}

int orbm_search_by_projection_last_frame_batch_device(
    orbm_ctx* ctx, int npairs, const int32_t* d_cur, const int32_t* d_last, int nframes, const orbx_kp* d_kps_un,
    const uint8_t* d_desc, const int32_t* d_counts, int kp_stride, const float* d_uright, const uint8_t* d_occupied,
    const float* d_pos, const uint8_t* d_mp_flags, const float* d_Tcw, const orbm_track_geom* geom, float th, int mono,
    int check_ori, int32_t* d_match, int32_t* d_nmatches, void* stream) {
    using namespace orbamd;
    if (!ctx || npairs < 0 || nframes < 1 || kp_stride < 1 || kp_stride > 65536 || !geom || geom->nlevels < 1 ||
        geom->nlevels > 16)
        return ORBX_EARG;
    if (npairs == 0) return 0;  // nothing to read: an empty pair list may come with NULL arrays
    if (!d_cur || !d_last || !d_kps_un || !d_desc || !d_counts || !d_pos || !d_mp_flags || !d_Tcw || !d_match ||
        !d_nmatches || ((uintptr_t)d_kps_un & 7) || ((uintptr_t)d_desc & 15))
        return ORBX_EARG;
    HIPR(hipSetDevice(ctx->device));
    const size_t S = (size_t)kp_stride;
    TrackArgs a;
    memset(&a, 0, sizeof(a));
    Carve pc;  // one pair's scratch: the current frame's SoA keypoints, the queries, the grid, scan and result arrays
    a.o_x = (long long)pc.take(4 * S);
    a.o_y = (long long)pc.take(4 * S);
    a.o_ang = (long long)pc.take(4 * S);
    a.o_oct = (long long)pc.take(4 * S);
    a.o_q = (long long)pc.take(sizeof(ProjQuery) * S);
    a.o_gs = (long long)pc.take(4 * (kGridCols * kGridRows + 1));
    a.o_gi = (long long)pc.take(2 * S);
    a.o_scan = (long long)pc.take(8 * (size_t)proj_topk() * S);
    a.o_scnt = (long long)pc.take(4 * S);
    a.o_res = (long long)pc.take(8 * S);
    a.pair_bytes = (long long)pc.off;
    Carve cv;
    const size_t o_calls = cv.take(sizeof(ProjCall) * (size_t)npairs);
    const size_t o_pairs = cv.take(pc.off * (size_t)npairs);
    if (ctx->scratch.ensure(cv.off)) return ORBX_EDEVICE;
    uint8_t* base = ctx->scratch.as<uint8_t>();
    a.cur = d_cur;
    a.last = d_last;
    a.nframes = nframes;
    a.kps = d_kps_un;
    a.desc = d_desc;
    a.counts = d_counts;
    a.kp_stride = kp_stride;
    a.uright = d_uright;
    a.occupied = d_occupied;
    a.pos = d_pos;
    a.mp_flags = d_mp_flags;
    a.Tcw = d_Tcw;
    a.g = *geom;
    a.th = th;
    a.mono = mono ? 1 : 0;
    a.check_ori = check_ori ? 1 : 0;
    a.match = d_match;
    a.nmatches = d_nmatches;
    a.err = ctx->err.as<int32_t>();
    a.calls = (ProjCall*)(base + o_calls);
    a.pair_scratch = base + o_pairs;
    hipStream_t st = (hipStream_t)stream;
    constexpr int kMaxCalls = 32768;  // gridDim.y of k_proj_scan
    for (int p0 = 0; p0 < npairs; p0 += kMaxCalls) {
        const int np = std::min(kMaxCalls, npairs - p0);
        HIPR(launch_track_prologue(a, p0, np, st));
        HIPR(launch_projection(a.calls + p0, np, kp_stride, st));
    }
    return 0;
}

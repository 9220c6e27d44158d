/*
 * orb_match_dev.h -- the reference matcher's rules (ORBmatcher.cc), each stated once for every matcher kernel
 * of match_kernels.hip, exchange_kernels.hip and frame_kernels.hip: descriptor distance, the epipolar tests
 * and candidate rule of SearchForTriangulation, the common-node lookup, SearchByBoW's best / second-best
 * selection, the rotation bin and the rotation-consistency filter. Device-only and inlined; the kernels keep
 * their own loops, staging and merges across slices (DESIGN.md "Matcher semantics").
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orb_match.h"
#include "orb_wave.h"

namespace orbamd {

/* ---- descriptors: 32 bytes = eight words; DescriptorDistance (ORBmatcher.cc:1647-1663) ---- */
__device__ __forceinline__ void load_desc8(uint32_t* w, uint4 a, uint4 b) {
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void load_desc8(uint32_t* w, const uint4* d) { load_desc8(w, d[0], d[1]); }
__device__ __forceinline__ void load_desc8(uint32_t* w, const uint8_t* d) { load_desc8(w, (const uint4*)d); }
/* lane l's descriptor v, broadcast to every lane (l wave-uniform) */
__device__ __forceinline__ void load_desc8_lane(uint32_t* w, const uint32_t* v, int l) {
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = (uint32_t)__builtin_amdgcn_readlane((int)v[k], l);
}
__device__ __forceinline__ float readlane_f(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

__device__ __forceinline__ int hamming8(const uint32_t* a, const uint32_t* b) {
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) d += __popc(a[k] ^ b[k]);
    return d;
}
__device__ __forceinline__ int hamming8(const uint32_t* a, uint4 b0, uint4 b1) {
    uint32_t b[8];
    load_desc8(b, b0, b1);
    return hamming8(a, b);
}
__device__ __forceinline__ int hamming8(uint4 a0, uint4 a1, uint4 b0, uint4 b1) {
    uint32_t a[8];
    load_desc8(a, a0, a1);
    return hamming8(a, b0, b1);
}
__device__ __forceinline__ int hamming8_lane(const uint32_t* a, const uint32_t* v, int l) {
    uint32_t b[8];
    load_desc8_lane(b, v, l);
    return hamming8(a, b);
}

/* ---- SearchForTriangulation (ORBmatcher.cc:657-823) ---- */
/* the epipolar line (a, b, c) of kp1 = (x1, y1) in the second image, CheckDistEpipolarLine's float operations
 * (ORBmatcher.cc:143-146); F = F12 row-major */
__device__ __forceinline__ void epi_line(const float* F, float x1, float y1, float* a, float* b, float* c) {
    *a = __fadd_rn(__fadd_rn(__fmul_rn(x1, F[0]), __fmul_rn(y1, F[3])), F[6]);
    *b = __fadd_rn(__fadd_rn(__fmul_rn(x1, F[1]), __fmul_rn(y1, F[4])), F[7]);
    *c = __fadd_rn(__fadd_rn(__fmul_rn(x1, F[2]), __fmul_rn(y1, F[5])), F[8]);
}

/* CheckDistEpipolarLine (ORBmatcher.cc:140-157) with kp1's line precomputed; `dsqr < 3.84*sigma2` compared in
 * double: th384 = 3.84 * (double)mvLevelSigma2[octave of kp2] */
__device__ __forceinline__ bool epi_ok(float a, float b, float c, float x2, float y2, double th384) {
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(a, x2), __fmul_rn(b, y2)), c);
    const float den = __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b));
    if (den == 0.f) return false;
    const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
    return (double)dsqr < th384;
}

/* epipole-radius rejection (ORBmatcher.cc:743-749): th100 = 100 * mvScaleFactors[octave of kp2], a float product */
__device__ __forceinline__ bool near_epipole(float ex, float ey, float x2, float y2, float th100) {
    const float dx = __fsub_rn(ex, x2), dy = __fsub_rn(ey, y2);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < th100;
}

/* The candidate rule of the scan (ORBmatcher.cc:704-776): skip dist > TH_LOW or dist > bestDist; the epipole
 * radius only for a monocular pair (!bStereo1 && !bStereo2); CheckDistEpipolarLine. The caller makes an accepted
 * candidate its new best, so equal distances go to the later candidate. (a, b, c): epi_line of kp1. kp2's side
 * comes by accessors, each called where the reference reads the value: xy2() (float2) for a candidate that passes
 * the distance test, th100() before near_epipole, th384() before epi_ok. A load hoisted above the test it belongs
 * to stays in flight across iterations of the caller's scan and makes its hot path wait for it. */
constexpr int kThLow = 50;  // TH_LOW (ORBmatcher.cc:36)
template <class XY, class Th100, class Th384>
__device__ __forceinline__ bool tri_accepts(int dist, int bestDist, bool mono_pair, float ex, float ey, float a,
                                            float b, float c, XY&& xy2, Th100&& th100, Th384&& th384) {
    if (dist > kThLow || dist > bestDist) return false;
    const float2 p2 = xy2();
    if (mono_pair && near_epipole(ex, ey, p2.x, p2.y, th100())) return false;
    return epi_ok(a, b, c, p2.x, p2.y, th384());
}

/* position of `node` among n ascending FeatureVector node ids, -1 when it is absent: the reference's merge walk
 * over two FeatureVectors (ORBmatcher.cc:184-264, 545-631, 691-789) visits exactly the ids present in both */
__device__ __forceinline__ int find_node(const uint32_t* nodes, int n, uint32_t node) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (nodes[mid] < node) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && nodes[lo] == node ? lo : -1;
}

/* ---- SearchByBoW (ORBmatcher.cc:159-288 (KF,F) = mode 0, :522-655 (KF,KF) = mode 1) ---- */
/* accept best1 <= TH_LOW (:228) / best1 < TH_LOW (:598) and (float)best1 < mfNNratio * (float)best2 */
__device__ __forceinline__ bool bow_accepts(int b1, int b2, int mode, float nnratio) {
    const bool ok_th = mode == 0 ? (b1 <= kThLow) : (b1 < kThLow);
    return ok_th && __fmul_rn(1.0f, (float)b1) < __fmul_rn(nnratio, (float)b2);
}

/* best / second best of the sequential scan (:205-225): b1 = the first strict minimum at position i1, b2 = the
 * second smallest of the multiset */
struct Top2 { int b1, i1, b2; };
__device__ __forceinline__ Top2 top2_merge(Top2 A, Top2 B) {
    Top2 r;
    const bool takeB = (B.b1 < A.b1) || (B.b1 == A.b1 && B.i1 >= 0 && (A.i1 < 0 || B.i1 < A.i1));
    r.b1 = takeB ? B.b1 : A.b1;
    r.i1 = takeB ? B.i1 : A.i1;
    r.b2 = min(max(A.b1, B.b1), min(A.b2, B.b2));
    return r;
}
/* this lane's positions lane, lane + 64, ... of nc candidates; dist_of(j) < 0: j takes no part */
template <class Dist>
__device__ __forceinline__ Top2 top2_scan(int lane, int nc, Dist&& dist_of) {
    Top2 r = {256, -1, 256};
    for (int j = lane; j < nc; j += 64) {
        const int dist = dist_of(j);
        if (dist < 0) continue;
        if (dist < r.b1) { r.b2 = r.b1; r.b1 = dist; r.i1 = j; }
        else if (dist < r.b2) { r.b2 = dist; }
    }
    return r;
}
__device__ __forceinline__ Top2 top2_wave(Top2 r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top2 o2;
        o2.b1 = __shfl_xor(r.b1, o, 64);
        o2.i1 = __shfl_xor(r.i1, o, 64);
        o2.b2 = __shfl_xor(r.b2, o, 64);
        r = top2_merge(r, o2);
    }
    return r;
}

/* One wave's greedy walk over a node's queries in order, descriptors and eligibility read from global memory:
 * a query with a good MapPoint takes best / second over the node's not yet matched candidates (mode 1: those
 * with a good MapPoint); an accept marks the candidate (vpMapPointMatches / vbMatched2 within the node) and
 * lane 0 calls emit(idxq, idxc). matched[0 .. nc) is the workgroup's, zeroed here. */
template <class GoodQ, class GoodC, class Emit>
__device__ __forceinline__ void bow_greedy_scan(int lane, const int32_t* featq, int nq, const uint8_t* descq,
                                                const int32_t* featc, int nc, const uint8_t* descc, uint8_t* matched,
                                                int mode, float nnratio, GoodQ&& good_q, GoodC&& good_c, Emit&& emit) {
    for (int j = lane; j < nc; j += 64) matched[j] = 0;
    __syncthreads();
    for (int k = 0; k < nq; k++) {
        const int idxq = featq[k];
        if (!good_q(idxq)) continue;
        uint32_t q[8];
        load_desc8(q, descq + (long long)idxq * 32);
        const Top2 r = top2_wave(top2_scan(lane, nc, [&](int j) {
            if (matched[j]) return -1;
            const int idxc = featc[j];
            if (mode == 1 && !good_c(idxc)) return -1;
            return hamming8(q, (const uint32_t*)(descc + (long long)idxc * 32));
        }));
        if (r.i1 >= 0 && bow_accepts(r.b1, r.b2, mode, nnratio)) {
            const int idxc = featc[r.i1];
            __syncthreads();
            if (lane == 0) {
                matched[r.i1] = 1;
                emit(idxq, idxc);
            }
            __syncthreads();
        }
    }
}

/* The greedy chain of a node of <= 64 candidates over up to 64 of its queries, in registers: candidate j =
 * lane j (descriptor cdw, feature index idxc, elig), query k = lane k (descriptor qdw, feature index myq or -1
 * without a good MapPoint), broadcast by readlane. Per query best1 = the first strict minimum = min over the
 * eligible lanes of dist << 6 | j, best2 = min dist of the other eligible lanes (ORBmatcher.cc:205-225); a
 * claimed candidate drops out of its lane. accept(na, idxq, idxc, k, i1) runs wave-uniformly for the na-th
 * accept (query lane k, candidate lane i1); returns na advanced by the accepts. */
template <class Accept>
__device__ __forceinline__ int bow_greedy_lanes(int lane, int nq, int myq, const uint32_t* qdw, const uint32_t* cdw,
                                                int idxc, bool& elig, int mode, float nnratio, int na,
                                                Accept&& accept) {
    for (int k = 0; k < nq; k++) {
        const int idxq = __builtin_amdgcn_readlane(myq, k);
        if (idxq < 0) continue;  // no good MapPoint (uniform)
        const int dist = hamming8_lane(cdw, qdw, k);
        const uint32_t m1 = wave_min_u32(elig ? ((uint32_t)dist << 6 | (uint32_t)lane) : 0xFFFFFFFFu);
        if (m1 == 0xFFFFFFFFu) continue;  // no eligible candidate left
        const int i1 = (int)(m1 & 63u), b1 = (int)(m1 >> 6);
        const int b2 = (int)wave_min_u32((elig && lane != i1) ? (uint32_t)dist : 256u);
        if (bow_accepts(b1, b2, mode, nnratio)) {
            const int idxc_w = __builtin_amdgcn_readlane(idxc, i1);
            if (lane == i1) elig = false;
            accept(na, idxq, idxc_w, k, i1);
            na++;
        }
    }
    return na;
}

/* ---- rotation consistency (ORBmatcher.cc:236-246, 267-285; ComputeThreeMaxima: orb_match.h) ---- */
/* Histogram bin of rot = a1 - a2 (:236-246, :1423-1430). Keypoint angles are in [0, 360), so the bin is 0..12
 * and the clamp never fires on what the extractor produces; it keeps a NaN or huge angle from indexing outside
 * a 30-entry histogram. */
__device__ __forceinline__ int rot_bin(float a1, float a2) {
    float rot = __fsub_rn(a1, a2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, 1.0f / 30));
    if (bin == 30) bin = 0;
    return min(max(bin, 0), 29);
}

/* The filter over one row m[0 .. n) by a 256-thread workgroup: histogram of bin_of(i, m[i]) over the matches,
 * ComputeThreeMaxima, every match outside the three bins set to -1. hist[30], keep[3]: LDS. Returns this
 * thread's count of kept matches. */
template <class Bin>
__device__ __forceinline__ int rot_filter_rows(int n, int32_t* m, Bin&& bin_of, int* hist, int* keep) {
    const int tid = threadIdx.x;
    if (tid < 30) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int j = m[i];
        if (j >= 0) atomicAdd(&hist[bin_of(i, j)], 1);
    }
    __syncthreads();
    if (tid == 0) three_maxima(hist, keep);
    __syncthreads();
    int local = 0;
    for (int i = tid; i < n; i += 256) {
        const int j = m[i];
        if (j < 0) continue;
        const int bin = bin_of(i, j);
        if (bin != keep[0] && bin != keep[1] && bin != keep[2]) m[i] = -1;
        else local++;
    }
    return local;
}

}  // namespace orbamd

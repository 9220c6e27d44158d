/*
 * undistort_kernels.hip -- Frame::UndistortKeyPoints (Frame.cc:405-435) on gfx950 for every frame of a batched
 * extraction: mvKeysUn from mvKeys where the extractor left them, so the matchers that are written on mvKeysUn
 * (ORBmatcher.cc:743-760) read device-resident coordinates for a distorted camera too.
 *
 * cv::undistortPoints(src, dst, K, D, noArray(), K) of OpenCV 3.x as undistort.c states it (the yardstick is
 * tests/undistort_py.py): double arithmetic with explicitly rounded intrinsics (no contraction), the correctly
 * rounded fp64 divide, five iterations, one rounding to float. One lane per keypoint; the 24-byte orbx_kp record is
 * 8-byte aligned and moves as three 8-byte words. The camera travels in the kernel arguments.
 */
#include <hip/hip_runtime.h>

#include "extract_host.h"

namespace orbamd {

namespace {

constexpr int kUndistortThreads = 256;

struct CamD {
    double fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2, k3;
};

__device__ __forceinline__ float2 undistort_one(const CamD& c, float2 p) {
    double x = __dmul_rn(__dsub_rn((double)p.x, c.cx), c.ifx);
    double y = __dmul_rn(__dsub_rn((double)p.y, c.cy), c.ify);
    const double x0 = x, y0 = y;
    const double p1x2 = __dmul_rn(2.0, c.p1), p2x2 = __dmul_rn(2.0, c.p2);  // the first product of 2*p1*x*y, 2*p2*x*y
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const double r2 = __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y));
        const double poly = __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(c.k3, r2), c.k2), r2), c.k1), r2);
        const double icdist = __ddiv_rn(1.0, __dadd_rn(1.0, poly));
        const double dX = __dadd_rn(__dmul_rn(__dmul_rn(p1x2, x), y),
                                    __dmul_rn(c.p2, __dadd_rn(r2, __dmul_rn(__dmul_rn(2.0, x), x))));
        const double dY = __dadd_rn(__dmul_rn(c.p1, __dadd_rn(r2, __dmul_rn(__dmul_rn(2.0, y), y))),
                                    __dmul_rn(__dmul_rn(p2x2, x), y));
        x = __dmul_rn(__dsub_rn(x0, dX), icdist);
        y = __dmul_rn(__dsub_rn(y0, dY), icdist);
    }
    // P = mK, R = I: xx = fx*x + 0*y + cx, yy = 0*x + fy*y + cy, ww = 1./(0*x + 0*y + 1)
    const double zx = __dmul_rn(0.0, x), zy = __dmul_rn(0.0, y);
    const double xx = __dadd_rn(__dadd_rn(__dmul_rn(c.fx, x), zy), c.cx);
    const double yy = __dadd_rn(__dadd_rn(zx, __dmul_rn(c.fy, y)), c.cy);
    const double ww = __ddiv_rn(1.0, __dadd_rn(__dadd_rn(zx, zy), 1.0));
    return make_float2(__double2float_rn(__dmul_rn(xx, ww)), __double2float_rn(__dmul_rn(yy, ww)));
}

/* grid (ceil(kp_stride / kUndistortThreads), nframes). in == out is allowed: a lane reads its own record before it
 * writes it and no lane reads another's. kDeliver (the one-frame host call, orbx_extract with a camera): the
 * keypoints and the count come from device memory and the kernel also delivers them as they are (raw_out,
 * count_out: the call's mapped pinned buffer), so nothing is read across PCIe. */
template <bool kDeliver>
__global__ __launch_bounds__(kUndistortThreads) void k_undistort(orbx_camera cam, const uint2* in,
                                                                 const int32_t* __restrict__ counts, int kp_stride,
                                                                 uint2* out, float2* kun, uint2* raw_out,
                                                                 int32_t* count_out) {
    const int f = blockIdx.y;
    const int i = blockIdx.x * kUndistortThreads + threadIdx.x;
    if (kDeliver && i == 0) count_out[f] = counts[f];
    const int n = min(counts[f], kp_stride);
    if (i >= n) return;
    const size_t rec = (size_t)f * kp_stride + i;
    const uint2 w0 = in[rec * 3], w1 = in[rec * 3 + 1], w2 = in[rec * 3 + 2];
    if (kDeliver) {
        raw_out[rec * 3] = w0;
        raw_out[rec * 3 + 1] = w1;
        raw_out[rec * 3 + 2] = w2;
    }
    float2 p = make_float2(__uint_as_float(w0.x), __uint_as_float(w0.y));
    if (cam.k1 != 0.0f) {  // mDistCoef.at<float>(0)==0.0 (Frame.cc:407): uniform, k1 alone decides
        CamD c;
        c.fx = cam.fx, c.fy = cam.fy, c.cx = cam.cx, c.cy = cam.cy;
        c.ifx = __ddiv_rn(1.0, c.fx), c.ify = __ddiv_rn(1.0, c.fy);
        c.k1 = cam.k1, c.k2 = cam.k2, c.p1 = cam.p1, c.p2 = cam.p2, c.k3 = cam.k3;
        p = undistort_one(c, p);
    }
    out[rec * 3] = make_uint2(__float_as_uint(p.x), __float_as_uint(p.y));
    out[rec * 3 + 1] = w1;
    out[rec * 3 + 2] = w2;
    if (kun) kun[rec] = p;
}

}  // namespace

hipError_t launch_undistort(const orbx_camera& cam, int nframes, const orbx_kp* kps, const int32_t* counts,
                            int kp_stride, orbx_kp* kps_un, float* kun, hipStream_t st) {
    const dim3 grid((kp_stride + kUndistortThreads - 1) / kUndistortThreads, nframes);
    hipLaunchKernelGGL(k_undistort<false>, grid, dim3(kUndistortThreads), 0, st, cam, (const uint2*)kps, counts,
                       kp_stride, (uint2*)kps_un, (float2*)kun, (uint2*)nullptr, (int32_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_undistort_deliver(const orbx_camera& cam, const orbx_kp* kps, const int32_t* count, int kp_stride,
                                    orbx_kp* raw_out, orbx_kp* un_out, int32_t* count_out, hipStream_t st) {
    const dim3 grid((kp_stride + kUndistortThreads - 1) / kUndistortThreads, 1);
    hipLaunchKernelGGL(k_undistort<true>, grid, dim3(kUndistortThreads), 0, st, cam, (const uint2*)kps, count,
                       kp_stride, (uint2*)un_out, (float2*)nullptr, (uint2*)raw_out, count_out);
    return hipGetLastError();
}

}  // namespace orbamd

int orbx_undistort_batch_device(orbx_handle* h, const orbx_camera* cam, int nframes, const orbx_kp* d_kps,
                                const int32_t* d_counts, int kp_stride, orbx_kp* d_kps_un, float* d_kun,
                                void* stream) {
    if (!h || !cam || cam->fx == 0 || cam->fy == 0 || nframes < 0 || nframes > 65535 || kp_stride < 1 || !d_kps ||
        !d_counts || !d_kps_un || (((uintptr_t)d_kps | (uintptr_t)d_kps_un | (uintptr_t)d_kun) & 7))
        return ORBX_EARG;
    if (nframes == 0) return 0;
    HIPR(hipSetDevice(h->device));
    HIPR(orbamd::launch_undistort(*cam, nframes, d_kps, d_counts, kp_stride, d_kps_un, d_kun, (hipStream_t)stream));
    return 0;
}

/*
 * unproject.c -- Frame::UnprojectStereo (Frame.cc:667-681) on the host for every keypoint of a frame: the world
 * positions of Tracking::StereoInitialization, UpdateLastFrame and CreateNewKeyFrame. Plain C, no device; built with
 * -ffp-contract=off.
 *
 * cv::Mat float arithmetic as pinned in DESIGN.md "Pinned semantics" (the same sequence is stated in Python,
 * tests/unproject_py.py, the yardstick, and in track_kernels.hip):
 *   invfx = 1.0f / fx in float (Frame.cc:104-105);
 *   x = (u - cx) * z * invfx, y = (v - cy) * z * invfy in float, in that order;
 *   mRwc = mRcw.t(), an exact transpose (Frame.cc:264);
 *   mOw = -mRcw.t() * mtcw (Frame.cc:266): the GEMM_1_T path, double accumulation, one rounding to float;
 *   mRwc * x3Dc + mOw: the small-matrix gemm, a row's three float products summed in float, then
 *   (float)((double)t + (double)mOw[i]);
 *   z <= 0 (or NaN) gives no point (cv::Mat() in the reference).
 */
#include "../../include/orbslam_amd.h"

int orbx_unproject_stereo(const orbx_camera* cam, const float Tcw[16], int n, const orbx_kp* kps_un,
                          const float* depth, float* pos, uint8_t* valid) {
    if (!cam || cam->fx == 0 || cam->fy == 0 || !Tcw || n < 0 || (n && (!kps_un || !depth || !pos))) return ORBX_EARG;
    const float invfx = 1.0f / cam->fx, invfy = 1.0f / cam->fy;
    const float cx = cam->cx, cy = cam->cy;
    float Ow[3];
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)Tcw[4 * k + i] * (double)Tcw[4 * k + 3];
        Ow[i] = (float)(-1.0 * s);
    }
    for (int j = 0; j < n; j++) {
        const float z = depth[j];
        float* p = pos + 3 * (size_t)j;
        if (!(z > 0)) {
            p[0] = p[1] = p[2] = 0.0f;
            if (valid) valid[j] = 0;
            continue;
        }
        const float u = kps_un[j].x, v = kps_un[j].y;
        const float x = (u - cx) * z * invfx;
        const float y = (v - cy) * z * invfy;
        for (int i = 0; i < 3; i++) { /* row i of mRwc = column i of mRcw */
            const float t0 = Tcw[i] * x + Tcw[4 + i] * y + Tcw[8 + i] * z;
            p[i] = (float)((double)t0 * 1.0 + (double)Ow[i] * 1.0);
        }
        if (valid) valid[j] = 1;
    }
    return 0;
}

/*
 * Frame_undistort_amd.cc -- Frame::UndistortKeyPoints (Frame.cc:405-435) and Frame::ComputeImageBounds
 * (Frame.cc:437-465, 213-214) over the C ABI (see Frame_undistort_amd.h).
 *
 * ORBAMD_UNDISTORT_HOST_ONLY leaves the extractor overload out, so the host functions build against
 * csrc/undistort.c alone (the sanitizer build of tests/cpp/test_undistort.cpp).
 */
#include "Frame_undistort_amd.h"

#include <cstring>

#ifndef ORBAMD_UNDISTORT_HOST_ONLY
#include "ORBextractor.h"
#include "orbamd_status.h"
#endif

namespace ORB_SLAM2 {
namespace amd {

void UndistortKeyPoints(const std::vector<cv::KeyPoint>& keys, const cv::Mat& K, const cv::Mat& distCoef,
                        std::vector<cv::KeyPoint>& keysUn) {
    keysUn = keys;  // cv::KeyPoint kp = mvKeys[i] (Frame.cc:430): every field but pt carried
    const int N = (int)keys.size();
    if (N == 0 || DistCoefAt(distCoef, 0) == 0.0) return;  // Frame.cc:407-411
    const orbx_camera cam = MakeCamera(K, distCoef);
    std::vector<float> xy(2 * (size_t)N);
    for (int i = 0; i < N; i++) {
        xy[2 * i] = keys[i].pt.x;
        xy[2 * i + 1] = keys[i].pt.y;
    }
    // a camera the library rejects (fx or fy zero; cv::undistortPoints would divide by it) leaves the copy
    if (orbx_undistort_points(&cam, N, xy.data(), xy.data()) != ORBX_OK) return;
    for (int i = 0; i < N; i++) {
        keysUn[i].pt.x = xy[2 * i];
        keysUn[i].pt.y = xy[2 * i + 1];
    }
}

void ComputeImageBounds(int cols, int rows, const cv::Mat& K, const cv::Mat& distCoef, float& minX, float& maxX,
                        float& minY, float& maxY, float& gridWInv, float& gridHInv) {
    orbx_camera cam = MakeCamera(K, distCoef);
    float b[4] = {0.0f, (float)cols, 0.0f, (float)rows};
    float gw = 64.0f / (float)(b[1] - b[0]), gh = 48.0f / (float)(b[3] - b[2]);
    orbx_image_bounds(&cam, cols, rows, b, &gw, &gh);  // on ORBX_EARG (fx or fy zero) the image's own bounds stay
    minX = b[0];
    maxX = b[1];
    minY = b[2];
    maxY = b[3];
    gridWInv = gw;
    gridHInv = gh;
}

#ifndef ORBAMD_UNDISTORT_HOST_ONLY
void UndistortKeyPoints(ORBextractor* extractor, const std::vector<cv::KeyPoint>& keys, const cv::Mat& K,
                        const cv::Mat& distCoef, std::vector<cv::KeyPoint>& keysUn) {
    const int N = (int)keys.size();
    const orbx_camera cam = MakeCamera(K, distCoef);
    if (extractor && N > 0 && extractor->DeviceHandle() && extractor->HasCamera() &&
        !memcmp(&cam, &extractor->Camera(), sizeof(cam))) {
        std::vector<orbx_kp> un((size_t)N);
        int n = 0;
        // ORBX_EARG here only says the last call delivered none (e.g. it ran stage-profiled): the host path serves
        if (orbx_last_keypoints_un(extractor->DeviceHandle(), un.data(), N, &n) == ORBX_OK && n == N) {
            keysUn = keys;
            for (int i = 0; i < N; i++) {
                keysUn[i].pt.x = un[i].x;
                keysUn[i].pt.y = un[i].y;
            }
            return;
        }
    }
    UndistortKeyPoints(keys, K, distCoef, keysUn);
}
#endif

}  // namespace amd
}  // namespace ORB_SLAM2

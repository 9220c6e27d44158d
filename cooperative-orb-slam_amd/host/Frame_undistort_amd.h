/*
 * Frame_undistort_amd.h -- drop-in bodies of Frame::UndistortKeyPoints (ORB_SLAM2/src/Frame.cc:405-435) and
 * Frame::ComputeImageBounds (Frame.cc:437-465, with the grid cell sizes of Frame.cc:213-214) as free functions, so
 * Frame.h stays the reference's (INTEGRATION.md gives the two member bodies that call them).
 *
 * cv::undistortPoints is restated in the library (include/orbslam_amd.h "Undistorted keypoints"; parity with OpenCV
 * unpinned, DESIGN.md "Pinned semantics"). The reference's quirk stays: mDistCoef.at<float>(0) == 0.0 means a copy
 * and the image's own bounds, whatever the other coefficients are.
 */
#ifndef FRAME_UNDISTORT_AMD_H
#define FRAME_UNDISTORT_AMD_H

#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>
#include <vector>

#include "orbslam_amd.h"

namespace ORB_SLAM2 {

class ORBextractor;

namespace amd {

/* element i of mDistCoef (a 4x1 or 5x1 CV_32F column, Tracking.cc:66-77; a row is read too) */
inline float DistCoefAt(const cv::Mat& d, int i) { return d.rows == 1 ? d.at<float>(0, i) : d.at<float>(i, 0); }

/* mK (3x3 CV_32F) and mDistCoef (4 or 5 entries) as the library's camera */
inline orbx_camera MakeCamera(const cv::Mat& K, const cv::Mat& distCoef) {
    orbx_camera c;
    c.fx = K.at<float>(0, 0);
    c.fy = K.at<float>(1, 1);
    c.cx = K.at<float>(0, 2);
    c.cy = K.at<float>(1, 2);
    c.k1 = DistCoefAt(distCoef, 0);
    c.k2 = DistCoefAt(distCoef, 1);
    c.p1 = DistCoefAt(distCoef, 2);
    c.p2 = DistCoefAt(distCoef, 3);
    c.k3 = distCoef.rows * distCoef.cols >= 5 ? DistCoefAt(distCoef, 4) : 0.f;
    return c;
}

/* Frame::UndistortKeyPoints on the host (orbx_undistort_points): keysUn[i] = keys[i] with only pt replaced. */
void UndistortKeyPoints(const std::vector<cv::KeyPoint>& keys, const cv::Mat& K, const cv::Mat& distCoef,
                        std::vector<cv::KeyPoint>& keysUn);

/* The same after `extractor` produced `keys` in its last operator(): when the extractor has this camera set
 * (ORBextractor::SetCamera) and that call delivered mvKeysUn from its own graph (orbx_last_keypoints_un), they are
 * taken from there; otherwise (no camera set, another camera, no device, a failed call) the host function runs. */
void UndistortKeyPoints(ORBextractor* extractor, const std::vector<cv::KeyPoint>& keys, const cv::Mat& K,
                        const cv::Mat& distCoef, std::vector<cv::KeyPoint>& keysUn);

/* Frame::ComputeImageBounds of a cols x rows image and Frame.cc:213-214: mnMinX, mnMaxX, mnMinY, mnMaxY,
 * mfGridElementWidthInv, mfGridElementHeightInv. */
void ComputeImageBounds(int cols, int rows, const cv::Mat& K, const cv::Mat& distCoef, float& minX, float& maxX,
                        float& minY, float& maxY, float& gridWInv, float& gridHInv);

}  // namespace amd
}  // namespace ORB_SLAM2
#endif

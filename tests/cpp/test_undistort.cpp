// test_undistort.cpp -- the drop-in Frame::UndistortKeyPoints / ComputeImageBounds (host/Frame_undistort_amd.h)
// against vectors the Python restatement wrote (tests/golden/undistort_vectors.txt, tests/undistort_py.py), bit for
// bit, with cv::KeyPoint's carried fields.
//   test_undistort <fixture>            host functions, and the extractor overload's device-less fallback
//   test_undistort <fixture> gpu        also the extractor overload after a real operator() with SetCamera
// Built with -DORBAMD_UNDISTORT_HOST_ONLY (the sanitizer build: this file, Frame_undistort_amd.cc and
// csrc/undistort.c, no library) only the host functions are tested.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "Frame_undistort_amd.h"
#ifndef ORBAMD_UNDISTORT_HOST_ONLY
#include "ORBextractor.h"
#endif

namespace {

int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            fails++;                                               \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
        }                                                          \
    } while (0)

float fbits(unsigned u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
bool same(float a, float b) { return !memcmp(&a, &b, 4); }

struct Case {
    std::string name;
    int cols = 0, rows = 0;
    float cam[9];
    float bounds[6];
    std::vector<float> in, un;  // x, y pairs
};

std::vector<Case> load(const char* path) {
    std::vector<Case> out;
    FILE* f = fopen(path, "r");
    if (!f) return out;
    char name[64];
    Case c;
    unsigned u[9];
    while (fscanf(f, " camera %63s %d %d %x %x %x %x %x %x %x %x %x", name, &c.cols, &c.rows, &u[0], &u[1], &u[2], &u[3],
                  &u[4], &u[5], &u[6], &u[7], &u[8]) == 12) {
        c.name = name;
        for (int i = 0; i < 9; i++) c.cam[i] = fbits(u[i]);
        if (fscanf(f, " bounds %x %x %x %x %x %x", &u[0], &u[1], &u[2], &u[3], &u[4], &u[5]) != 6) break;
        for (int i = 0; i < 6; i++) c.bounds[i] = fbits(u[i]);
        int n = 0;
        if (fscanf(f, " points %d", &n) != 1) break;
        c.in.clear();
        c.un.clear();
        for (int i = 0; i < n; i++) {
            if (fscanf(f, " %x %x %x %x", &u[0], &u[1], &u[2], &u[3]) != 4) break;
            c.in.push_back(fbits(u[0]));
            c.in.push_back(fbits(u[1]));
            c.un.push_back(fbits(u[2]));
            c.un.push_back(fbits(u[3]));
        }
        if ((int)c.in.size() != 2 * n) break;
        out.push_back(c);
    }
    fclose(f);
    return out;
}

void mats(const Case& c, cv::Mat& K, cv::Mat& D) {
    K = cv::Mat(3, 3, CV_32F);  // cv::Mat::eye with fx, fy, cx, cy (Tracking.cc:59-64)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) K.at<float>(i, j) = i == j ? 1.f : 0.f;
    K.at<float>(0, 0) = c.cam[0];
    K.at<float>(1, 1) = c.cam[1];
    K.at<float>(0, 2) = c.cam[2];
    K.at<float>(1, 2) = c.cam[3];
    const int nd = c.cam[8] != 0 ? 5 : 4;  // DistCoef.resize(5) only for k3 != 0 (Tracking.cc:71-76)
    D = cv::Mat(nd, 1, CV_32F);
    for (int i = 0; i < nd; i++) D.at<float>(i, 0) = c.cam[4 + i];
}

std::vector<cv::KeyPoint> keys_of(const Case& c) {
    std::vector<cv::KeyPoint> k;
    for (size_t i = 0; i < c.in.size() / 2; i++)
        k.push_back(cv::KeyPoint(c.in[2 * i], c.in[2 * i + 1], 31.f + (float)(i % 7), (float)(i % 360) + 0.25f,
                                 (float)(20 + i % 100), (int)(i % 8), (int)i - 3));
    return k;
}

void check_keys(const Case& c, const std::vector<cv::KeyPoint>& k, const std::vector<cv::KeyPoint>& un) {
    CHECK(un.size() == k.size());
    int bad = 0;
    for (size_t i = 0; i < k.size() && i < un.size(); i++) {
        bad += !same(un[i].pt.x, c.un[2 * i]) || !same(un[i].pt.y, c.un[2 * i + 1]);
        bad += !same(un[i].size, k[i].size) || !same(un[i].angle, k[i].angle) || !same(un[i].response, k[i].response) ||
               un[i].octave != k[i].octave || un[i].class_id != k[i].class_id;
    }
    if (bad) printf("%s: %d keypoints differ\n", c.name.c_str(), bad);
    CHECK(bad == 0);
}

}  // namespace

int main(int argc, char** argv) {
    using namespace ORB_SLAM2;
    if (argc < 2) {
        printf("usage: test_undistort <tests/golden/undistort_vectors.txt> [gpu]\n");
        return 2;
    }
    const std::vector<Case> cases = load(argv[1]);
    CHECK(cases.size() == 4);
    bool saw_copy = false;
    for (const Case& c : cases) {
        cv::Mat K, D;
        mats(c, K, D);
        const std::vector<cv::KeyPoint> k = keys_of(c);
        CHECK(k.size() >= 100);
        std::vector<cv::KeyPoint> un(3);  // stale content is replaced
        amd::UndistortKeyPoints(k, K, D, un);
        check_keys(c, k, un);
        if (c.cam[4] == 0) {  // k1 == 0: a copy, whatever k2, p1, p2, k3 are
            saw_copy = true;
            CHECK(c.cam[5] != 0 && c.cam[6] != 0 && c.cam[7] != 0);
            for (size_t i = 0; i < k.size(); i++) CHECK(same(un[i].pt.x, k[i].pt.x) && same(un[i].pt.y, k[i].pt.y));
        }
        float b[6] = {0};
        amd::ComputeImageBounds(c.cols, c.rows, K, D, b[0], b[1], b[2], b[3], b[4], b[5]);
        for (int i = 0; i < 6; i++) CHECK(same(b[i], c.bounds[i]));
        std::vector<cv::KeyPoint> none, un0(2);
        amd::UndistortKeyPoints(none, K, D, un0);
        CHECK(un0.empty());
#ifndef ORBAMD_UNDISTORT_HOST_ONLY
        // the extractor overload without a delivered mvKeysUn (no call yet, and no device on a CPU box): host path
        ORBextractor ext(1000, 1.2f, 8, 20, 7);
        std::vector<cv::KeyPoint> un1;
        amd::UndistortKeyPoints(&ext, k, K, D, un1);  // no camera set
        check_keys(c, k, un1);
        ext.SetCamera(K, D);
        CHECK(ext.HasCamera() && same(ext.Camera().k1, c.cam[4]) && same(ext.Camera().k3, c.cam[8]));
        std::vector<cv::KeyPoint> un2;
        amd::UndistortKeyPoints(&ext, k, K, D, un2);  // camera set, nothing delivered
        check_keys(c, k, un2);
        std::vector<cv::KeyPoint> un3;
        amd::UndistortKeyPoints((ORBextractor*)nullptr, k, K, D, un3);
        check_keys(c, k, un3);
#endif
    }
    CHECK(saw_copy);
#ifndef ORBAMD_UNDISTORT_HOST_ONLY
    if (argc > 2 && !strcmp(argv[2], "gpu")) {
        // a real frame: the overload takes mvKeysUn from the extractor's own call and equals the host function
        const Case& c = cases[0];
        cv::Mat K, D;
        mats(c, K, D);
        const int W = 640, H = 480;
        ORBextractor ext(1000, 1.2f, 8, 20, 7);
        ext.SetCamera(K, D);
        for (int t = 0; t < 3; t++) {  // eager, capturing, replayed
            cv::Mat img(H, W, CV_8UC1), desc;
            CHECK(orbx_synth_frame(0, t, W, H, img.data) == 0);
            std::vector<cv::KeyPoint> k, un_dev, un_host;
            ext(img, cv::Mat(), k, desc);
            CHECK(ext.LastStatus() == 0 && k.size() > 500);
            orbx_kp probe;
            int n = 0;
            CHECK(orbx_last_keypoints_un(ext.DeviceHandle(), &probe, 0, &n) == ORBX_ECAPACITY);  // it was delivered
            amd::UndistortKeyPoints(&ext, k, K, D, un_dev);
            amd::UndistortKeyPoints(k, K, D, un_host);
            CHECK(un_dev.size() == k.size() && un_host.size() == k.size());
            int bad = 0, moved = 0;
            for (size_t i = 0; i < k.size(); i++) {
                bad += !same(un_dev[i].pt.x, un_host[i].pt.x) || !same(un_dev[i].pt.y, un_host[i].pt.y) ||
                       !same(un_dev[i].angle, k[i].angle) || un_dev[i].octave != k[i].octave;
                moved += !same(un_dev[i].pt.x, k[i].pt.x);
            }
            CHECK(bad == 0 && moved > 0);
        }
    }
#endif
    if (fails)
        printf("FAILED (%d)\n", fails);
    else
        printf("ALL PASS\n");
    return fails ? 1 : 0;
}

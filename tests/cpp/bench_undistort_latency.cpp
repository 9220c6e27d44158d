// bench_undistort_latency.cpp -- what mvKeysUn costs per frame on the one-frame path, from C++ (no Python in the
// loop): the median wall time of `reps` orbx_extract calls at 640x480 / 1000 features in three settings,
//   a  camera off                                  (ORBextractor::operator() alone)
//   b  camera on + orbx_last_keypoints_un          (the undistort node inside the call's graph)
//   c  camera off + host orbx_undistort_keypoints  (what the reference pays: Frame::UndistortKeyPoints on the CPU)
// in `rounds` interleaved rounds, plus the host undistortion alone (row "host_only"). b and c must deliver the same
// bits. One JSON line per round and a summary line. Built with -DEXTRACT_ONLY the program runs setting a alone and
// uses no entry point younger than orbx_extract, so it also links against an older library for an A/B of setting a.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "orbslam_amd.h"

namespace {

// the textured scene of bench_latency.cpp
std::vector<uint8_t> scene(int W, int H, unsigned seed) {
    std::mt19937 rs(1234), rn(seed);
    std::vector<int> img((size_t)W * H);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) img[(size_t)y * W + x] = 40 + (x + y) / 16;
    for (int r = 0; r < 700; r++) {
        const int w = 6 + rs() % 40, h = 6 + rs() % 40, x0 = rs() % W, y0 = rs() % H, v = rs() % 200;
        for (int y = std::max(0, y0); y < std::min(H, y0 + h); y++)
            for (int x = std::max(0, x0); x < std::min(W, x0 + w); x++) img[(size_t)y * W + x] = v + 30;
    }
    std::vector<uint8_t> out(img.size());
    for (size_t i = 0; i < img.size(); i++) out[i] = (uint8_t)std::min(255, std::max(0, img[i] + (int)(rn() % 7) - 3));
    return out;
}

double median_us(int reps, const std::function<void()>& f) {
    for (int i = 0; i < std::max(3, reps / 20); i++) f();
    std::vector<double> t(reps);
    for (int i = 0; i < reps; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        t[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    std::nth_element(t.begin(), t.begin() + reps / 2, t.end());
    return t[reps / 2];
}

}  // namespace

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 1000;
    const int rounds = argc > 2 ? atoi(argv[2]) : 3;
    const int W = 640, H = 480;
    orbx_params prm = {1000, 1.2f, 8, 20, 7};
    orbx_handle* off = nullptr;
    if (orbx_create(&prm, 0, W, H, 1, &off)) {
        printf("orbx_create failed\n");
        return 1;
    }
    const int cap = orbx_max_keypoints(off, W, H);
    const std::vector<uint8_t> img = scene(W, H, 1);
    std::vector<orbx_kp> kp(cap), kb(cap), un_b(cap), un_c(cap);
    std::vector<uint8_t> d(32 * (size_t)cap);
    int n = 0, bad = 0;
    const auto extract_off = [&] { bad |= orbx_extract(off, img.data(), W, H, W, kp.data(), d.data(), cap, &n); };
#ifdef EXTRACT_ONLY
    for (int r = 0; r < rounds; r++) {
        const double a = median_us(reps, extract_off);
        printf("{\"row\": \"extract_only\", \"round\": %d, \"reps\": %d, \"a_camera_off_us\": %.2f, \"n\": %d}\n",
               r, reps, a, n);
        fflush(stdout);
    }
    orbx_destroy(off);
    return bad ? 1 : 0;
#else
    // my.yaml:8-17
    const orbx_camera cam = {715.092024f, 719.025258f, 334.298489f, 256.326097f, 0.085908f, -0.07019499f, 0.0062169f,
                             0.010791f, 0.f};
    orbx_handle* on = nullptr;
    if (orbx_create(&prm, 0, W, H, 1, &on) || orbx_set_camera(on, &cam)) {
        printf("orbx_create / orbx_set_camera failed\n");
        return 1;
    }
    int nb = 0, nu = 0;
    std::vector<double> A, B, Cc;
    for (int r = 0; r < rounds; r++) {
        const double a = median_us(reps, extract_off);
        const double b = median_us(reps, [&] {
            bad |= orbx_extract(on, img.data(), W, H, W, kb.data(), d.data(), cap, &nb);
            bad |= orbx_last_keypoints_un(on, un_b.data(), cap, &nu);
        });
        const double c = median_us(reps, [&] {
            bad |= orbx_extract(off, img.data(), W, H, W, kp.data(), d.data(), cap, &n);
            bad |= orbx_undistort_keypoints(&cam, n, kp.data(), un_c.data());
        });
        const double host = median_us(reps, [&] { bad |= orbx_undistort_keypoints(&cam, n, kp.data(), un_c.data()); });
        const bool same = n == nb && nb == nu && n > 0 && !memcmp(kp.data(), kb.data(), sizeof(orbx_kp) * n) &&
                          !memcmp(un_b.data(), un_c.data(), sizeof(orbx_kp) * n);
        bad |= !same;
        printf("{\"row\": \"undistort_one_frame\", \"round\": %d, \"reps\": %d, \"a_camera_off_us\": %.2f, "
               "\"b_camera_on_us\": %.2f, \"c_host_undistort_us\": %.2f, \"host_only_us\": %.2f, \"identical\": %s, "
               "\"n\": %d}\n", r, reps, a, b, c, host, same ? "true" : "false", n);
        fflush(stdout);
        A.push_back(a), B.push_back(b), Cc.push_back(c);
    }
    auto spread = [](const std::vector<double>& v) {
        return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end());
    };
    double margin = 1e30;
    for (int r = 0; r < rounds; r++) margin = std::min(margin, Cc[r] - B[r]);
    const double noise = std::max(spread(B), spread(Cc));
    printf("{\"row\": \"undistort_one_frame_summary\", \"least_c_minus_b_us\": %.2f, \"round_to_round_b_us\": %.2f, "
           "\"round_to_round_c_us\": %.2f, \"round_to_round_a_us\": %.2f, \"in_graph_wins\": %s}\n",
           margin, spread(B), spread(Cc), spread(A), margin > noise ? "true" : "false");
    orbx_destroy(on);
    orbx_destroy(off);
    return bad ? 1 : 0;
#endif
}

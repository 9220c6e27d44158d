/*
 * undistort.c -- Frame::UndistortKeyPoints (Frame.cc:405-435) and Frame::ComputeImageBounds (Frame.cc:437-465, with
 * the grid cell sizes of Frame.cc:213-214) on the host. Plain C, no device; built with -ffp-contract=off.
 *
 * cv::undistortPoints(src, dst, K, D, noArray(), K) of OpenCV 3.x, restated from its published algorithm (parity
 * unpinned, DESIGN.md "Pinned semantics"): every operation in double, in the order written here, no fma, five
 * iterations with no convergence test and no special case for a negative icdist. The rational and thin-prism terms
 * of OpenCV's loop have zero coefficients for a 4- or 5-entry mDistCoef (they add +0.0) and are left out. The same
 * sequence is stated in Python (tests/undistort_py.py, the yardstick) and in undistort_kernels.hip.
 */
#include "../../include/orbslam_amd.h"

typedef struct {
    double fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2, k3;
} cam_d;

static void widen(const orbx_camera* c, cam_d* d) {
    d->fx = c->fx;
    d->fy = c->fy;
    d->cx = c->cx;
    d->cy = c->cy;
    d->ifx = 1. / d->fx;
    d->ify = 1. / d->fy;
    d->k1 = c->k1;
    d->k2 = c->k2;
    d->p1 = c->p1;
    d->p2 = c->p2;
    d->k3 = c->k3;
}

static void undistort_one(const cam_d* c, float px, float py, float* ox, float* oy) {
    double x = ((double)px - c->cx) * c->ifx;
    double y = ((double)py - c->cy) * c->ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = 1 / (1 + ((c->k3 * r2 + c->k2) * r2 + c->k1) * r2);
        const double dX = 2 * c->p1 * x * y + c->p2 * (r2 + 2 * x * x);
        const double dY = c->p1 * (r2 + 2 * y * y) + 2 * c->p2 * x * y;
        x = (x0 - dX) * icdist;
        y = (y0 - dY) * icdist;
    }
    /* P = mK, R = I */
    const double xx = c->fx * x + 0 * y + c->cx;
    const double yy = 0 * x + c->fy * y + c->cy;
    const double ww = 1. / (0 * x + 0 * y + 1);
    *ox = (float)(xx * ww);
    *oy = (float)(yy * ww);
}

static int cam_bad(const orbx_camera* cam) { return !cam || cam->fx == 0 || cam->fy == 0; }

int orbx_undistort_points(const orbx_camera* cam, int n, const float* xy_in, float* xy_out) {
    if (cam_bad(cam) || n < 0 || (n && (!xy_in || !xy_out))) return ORBX_EARG;
    if (cam->k1 == 0.0) { /* mDistCoef.at<float>(0)==0.0 (Frame.cc:407): k1 alone decides */
        if (xy_out != xy_in)
            for (int i = 0; i < 2 * n; i++) xy_out[i] = xy_in[i];
        return 0;
    }
    cam_d c;
    widen(cam, &c);
    for (int i = 0; i < n; i++) {
        float ox, oy;
        undistort_one(&c, xy_in[2 * i], xy_in[2 * i + 1], &ox, &oy);
        xy_out[2 * i] = ox;
        xy_out[2 * i + 1] = oy;
    }
    return 0;
}

int orbx_undistort_keypoints(const orbx_camera* cam, int n, const orbx_kp* in, orbx_kp* out) {
    if (cam_bad(cam) || n < 0 || (n && (!in || !out))) return ORBX_EARG;
    const int copy = cam->k1 == 0.0;
    cam_d c;
    widen(cam, &c);
    for (int i = 0; i < n; i++) {
        orbx_kp k = in[i]; /* cv::KeyPoint kp = mvKeys[i] (Frame.cc:430) */
        if (!copy) undistort_one(&c, k.x, k.y, &k.x, &k.y);
        out[i] = k;
    }
    return 0;
}

int orbx_image_bounds(const orbx_camera* cam, int cols, int rows, float bounds[4], float* grid_w_inv,
                      float* grid_h_inv) {
    if (cam_bad(cam) || !bounds) return ORBX_EARG;
    float minx, maxx, miny, maxy;
    if (cam->k1 != 0.0) {
        const float corner[4][2] = {{0.0f, 0.0f}, {(float)cols, 0.0f}, {0.0f, (float)rows}, {(float)cols, (float)rows}};
        float u[4][2];
        cam_d c;
        widen(cam, &c);
        for (int i = 0; i < 4; i++) undistort_one(&c, corner[i][0], corner[i][1], &u[i][0], &u[i][1]);
        /* std::min(a, b) = b < a ? b : a, std::max(a, b) = a < b ? b : a (Frame.cc:452-455) */
        minx = u[2][0] < u[0][0] ? u[2][0] : u[0][0];
        maxx = u[1][0] < u[3][0] ? u[3][0] : u[1][0];
        miny = u[1][1] < u[0][1] ? u[1][1] : u[0][1];
        maxy = u[2][1] < u[3][1] ? u[3][1] : u[2][1];
    } else {
        minx = 0.0f;
        maxx = (float)cols;
        miny = 0.0f;
        maxy = (float)rows;
    }
    bounds[0] = minx;
    bounds[1] = maxx;
    bounds[2] = miny;
    bounds[3] = maxy;
    if (grid_w_inv) *grid_w_inv = 64.0f / (float)(maxx - minx);
    if (grid_h_inv) *grid_h_inv = 48.0f / (float)(maxy - miny);
    return 0;
}

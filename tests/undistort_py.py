"""Pure-Python restatement of Frame::UndistortKeyPoints (Frame.cc:405-435) and Frame::ComputeImageBounds
(Frame.cc:437-465, grid cell sizes Frame.cc:213-214): the yardstick of tests/test_undistort.py and
tests/test_gpu_undistort.py.

cv::undistortPoints(src, dst, K, D, noArray(), K) of OpenCV 3.x, restated from its published algorithm (OpenCV is
not available; parity unpinned, DESIGN.md "Pinned semantics"). Python floats are IEEE doubles and Python never
contracts a*b+c, so every line below is one correctly rounded double operation after another, in the order written.
"""
import numpy as np

ITERS = 5  # OpenCV 3.x: a fixed count, no convergence test


def f32(v):
    return float(np.float32(v))


class Camera:
    """The float members of mK / mDistCoef, widened to double (k3 = 0 for a 4-entry mDistCoef)."""
    NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")

    def __init__(self, fx, fy, cx, cy, k1, k2, p1, p2, k3=0.0):
        for k, v in zip(self.NAMES, (fx, fy, cx, cy, k1, k2, p1, p2, k3)):
            setattr(self, k, f32(v))

    def astuple(self):
        return tuple(getattr(self, k) for k in self.NAMES)


# the cameras of the reference's settings files, with the image size they are used at
MY_YAML = (Camera(715.092024, 719.025258, 334.298489, 256.326097, 0.085908, -0.07019499, 0.0062169, 0.010791), 640, 480)
TUM1 = (Camera(517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314),
        640, 480)
EUROC = (Camera(458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05), 752, 480)
CAMERAS = {"my": MY_YAML, "tum1": TUM1, "euroc": EUROC}
# k1 == 0 with every other coefficient set: the reference copies (Frame.cc:407-411, 458-464)
K1_ZERO = (Camera(715.092024, 719.025258, 334.298489, 256.326097, 0.0, -0.07019499, 0.0062169, 0.010791, 0.5), 640, 480)


def normalized(cam, px, py, iters=ITERS):
    """the iteration alone: (x, y) in normalised coordinates, doubles (before the projection with P = mK)"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam.astuple()
    ifx = 1. / fx
    ify = 1. / fy
    x = (f32(px) - cx) * ifx
    y = (f32(py) - cy) * ify
    x0 = x
    y0 = y
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dX) * icdist
        y = (y0 - dY) * icdist
    return x, y


def cv_undistort_point(cam, px, py, iters=ITERS):
    """one point of cv::undistortPoints(src, dst, K, D, noArray(), K): (np.float32, np.float32)"""
    x, y = normalized(cam, px, py, iters)
    xx = cam.fx * x + 0 * y + cam.cx
    yy = 0 * x + cam.fy * y + cam.cy
    ww = 1. / (0 * x + 0 * y + 1)
    return np.float32(xx * ww), np.float32(yy * ww)  # round to nearest even


def distort_normalized(cam, x, y):
    """the closed-form forward model (normalised undistorted -> distorted pixel), for the sanity check only"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam.astuple()
    r2 = x * x + y * y
    cdist = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * cdist + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cdist + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def undistort_points(cam, xy, iters=ITERS):
    """Frame.cc:407-424 over float32 [n, 2]: a copy when k1 == 0, else cv::undistortPoints"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    if cam.k1 == 0.0:
        return xy.copy()
    out = np.empty_like(xy)
    for i in range(len(xy)):
        out[i] = cv_undistort_point(cam, xy[i, 0], xy[i, 1], iters)
    return out


def undistort_keypoints(cam, kps):
    """Frame::UndistortKeyPoints: mvKeysUn[i] = mvKeys[i] with only pt replaced (structured orbx_kp array)"""
    out = kps.copy()
    if len(kps):
        xy = undistort_points(cam, np.stack([kps["x"], kps["y"]], 1))
        out["x"], out["y"] = xy[:, 0], xy[:, 1]
    return out


def image_bounds(cam, cols, rows):
    """Frame::ComputeImageBounds and Frame.cc:213-214: ((mnMinX, mnMaxX, mnMinY, mnMaxY) float32, grid_w_inv,
    grid_h_inv float32); std::min(a, b) = b < a ? b : a, std::max(a, b) = a < b ? b : a"""
    if cam.k1 != 0.0:
        c = [cv_undistort_point(cam, x, y) for x, y in ((0, 0), (cols, 0), (0, rows), (cols, rows))]
        minx = c[2][0] if c[2][0] < c[0][0] else c[0][0]
        maxx = c[3][0] if c[1][0] < c[3][0] else c[1][0]
        miny = c[1][1] if c[1][1] < c[0][1] else c[0][1]
        maxy = c[3][1] if c[2][1] < c[3][1] else c[2][1]
    else:
        minx, maxx, miny, maxy = np.float32(0), np.float32(cols), np.float32(0), np.float32(rows)
    b = np.array([minx, maxx, miny, maxy], np.float32)
    gw = np.float32(64.0) / np.float32(b[1] - b[0])
    gh = np.float32(48.0) / np.float32(b[3] - b[2])
    return b, np.float32(gw), np.float32(gh)


def test_points(cols, rows, cam, n_random=500, seed=11):
    """float32 [n, 2]: the four corners, the principal point, points outside the image (negative, beyond cols /
    rows) and n_random seeded random points (sub-pixel coordinates, as keypoints of the upper levels have)"""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (cols, 0), (0, rows), (cols, rows), (cam.cx, cam.cy), (-7.5, -3.25), (-20, rows / 2),
             (cols + 12.5, rows + 9), (cols / 2, rows + 30), (cols + 25, -10)]
    rnd = np.stack([rng.uniform(0, cols, n_random), rng.uniform(0, rows, n_random)], 1)
    return np.concatenate([np.array(fixed, np.float64), rnd]).astype(np.float32)


def test_keypoints(cols, rows, cam, n_random=500, seed=11):
    """the same points as an orbx_kp array with every carried field set to a distinct bit pattern"""
    from orbamd import kp_dtype
    xy = test_points(cols, rows, cam, n_random, seed)
    rng = np.random.default_rng(seed + 1)
    k = np.zeros(len(xy), kp_dtype)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["octave"] = rng.integers(0, 8, len(xy))
    k["size"] = (31 * 1.2 ** k["octave"]).astype(np.int32)
    k["angle"] = rng.uniform(0, 360, len(xy)).astype(np.float32)
    k["response"] = rng.integers(7, 200, len(xy)).astype(np.float32)
    return k


FIXTURE = "undistort_vectors.txt"  # under tests/golden/


def fixture_text(n_random=120):
    """the vectors tests/cpp/test_undistort.cpp reads, every float as the hex of its bits: per camera a line
    `camera <name> <cols> <rows> <fx fy cx cy k1 k2 p1 p2 k3>`, a line `bounds <minx maxx miny maxy gw gh>`, a line
    `points <n>` and n lines `<x y x_un y_un>`. The k1 == 0 camera is among them."""
    def hx(v):
        return "%08x" % int(np.array(v, np.float32).view(np.uint32))
    lines = []
    for name, (cam, cols, rows) in list(CAMERAS.items()) + [("k1zero", K1_ZERO)]:
        lines.append("camera %s %d %d %s" % (name, cols, rows, " ".join(hx(v) for v in cam.astuple())))
        b, gw, gh = image_bounds(cam, cols, rows)
        lines.append("bounds %s" % " ".join(hx(v) for v in list(b) + [gw, gh]))
        xy = test_points(cols, rows, cam, n_random)
        un = undistort_points(cam, xy)
        lines.append("points %d" % len(xy))
        lines += ["%s %s %s %s" % (hx(a[0]), hx(a[1]), hx(u[0]), hx(u[1])) for a, u in zip(xy, un)]
    return "\n".join(lines) + "\n"


test_points.__test__ = False
test_keypoints.__test__ = False

if __name__ == "__main__":
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", FIXTURE), "w") as f:
        f.write(fixture_text())

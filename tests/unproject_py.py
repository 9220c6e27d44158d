"""Frame::UnprojectStereo (Frame.cc:667-681) restated in pure Python on numpy float32 / float64 scalars, one operation
per rounding: the yardstick of csrc/unproject.c and of k_unproject (track_kernels.hip).

cv::Mat float arithmetic as pinned in DESIGN.md "Pinned semantics":
  invfx = 1.0f / fx in float (Frame.cc:104-105);
  x = (u - cx) * z * invfx, y = (v - cy) * z * invfy, in float and in that order;
  mRwc = mRcw.t();  mOw = -mRcw.t() * mtcw: GEMM_1_T, double accumulation from 0, (float)(-1.0 * s);
  mRwc * x3Dc + mOw: the small-matrix gemm, the row's three float products summed in float, then
  (float)((double)t + (double)mOw[i]);
  z <= 0 gives no point.
"""
import os
import sys

import numpy as np

f32, f64 = np.float32, np.float64


def camera_center(Tcw):
    """mOw of mTcw (4x4)"""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    Ow = []
    for i in range(3):
        s = f64(0)
        for k in range(3):
            s = s + f64(T[k, i]) * f64(T[k, 3])
        Ow.append(f32(f64(-1.0) * s))
    return Ow


def unproject_one(fx, fy, cx, cy, Tcw, Ow, u, v, z):
    """the world point (three float32) or None (the reference's empty cv::Mat)"""
    z = f32(z)
    if not z > 0:
        return None
    T = np.asarray(Tcw, f32).reshape(4, 4)
    invfx = f32(1.0) / f32(fx)
    invfy = f32(1.0) / f32(fy)
    x = f32(f32(f32(u) - f32(cx)) * z) * invfx
    y = f32(f32(f32(v) - f32(cy)) * z) * invfy
    out = []
    for i in range(3):  # row i of mRwc = column i of mRcw
        t0 = f32(f32(T[0, i] * x) + f32(T[1, i] * y)) + f32(T[2, i] * z)
        out.append(f32(f64(t0) + f64(Ow[i])))
    return out


def unproject_stereo(cam, Tcw, kps_un, depth):
    """(pos float32 [n, 3], valid uint8 [n]) as orbx_unproject_stereo writes them; cam has fx, fy, cx, cy"""
    n = len(kps_un)
    pos = np.zeros((n, 3), f32)
    valid = np.zeros(n, np.uint8)
    Ow = camera_center(Tcw)
    with np.errstate(all="ignore"):
        for i in range(n):
            p = unproject_one(cam.fx, cam.fy, cam.cx, cam.cy, Tcw, Ow, kps_un["x"][i], kps_un["y"][i], depth[i])
            if p is not None:
                pos[i] = p
                valid[i] = 1
    return pos, valid


DENORMAL = np.array(1000, np.uint32).view(f32)[()]  # 1.4e-42
EDGE_DEPTHS = [-1.0, 0.0, -0.0, DENORMAL, 1e6, np.finfo(f32).tiny, 0.25]


def poses(seed=5):
    """the identity and two poses of proj_scenes.rot / pose (a small and a large rotation)"""
    import proj_scenes as ps
    rng = np.random.default_rng(seed)
    return [np.eye(4, dtype=f32), ps.pose(ps.rot(rng, 2.0), rng.normal(0, 0.05, 3)),
            ps.pose(ps.rot(rng, 60.0), rng.normal(0, 2.0, 3))]


def test_inputs(cols, rows, cam, n_random=200, seed=23):
    """(keypoints orbx_kp [n], depth float32 [n]): undistort_py's points with the edge depths first, then random
    depths of which a fifth is -1 (no stereo match, as ComputeStereoMatches leaves it)"""
    import undistort_py as U
    kps = U.test_keypoints(cols, rows, cam, n_random, seed)
    rng = np.random.default_rng(seed + 2)
    d = rng.uniform(0.3, 40.0, len(kps)).astype(f32)
    d[rng.random(len(kps)) < 0.2] = -1.0
    d[:len(EDGE_DEPTHS)] = np.array(EDGE_DEPTHS, f32)
    return kps, d


FIXTURE = "unproject_vectors.txt"  # under tests/golden/


def fixture_text(n_random=30):
    """the vectors tests/cpp/test_unproject.c reads, every float as the hex of its bits: per camera and pose a line
    `case <name> <fx fy cx cy>`, a line `pose <16 words>`, a line `points <n>` and n lines
    `<u v depth valid x y z>`."""
    import undistort_py as U

    def hx(v):
        return "%08x" % int(np.array(v, f32).view(np.uint32))
    lines = []
    for name, (cam, cols, rows) in U.CAMERAS.items():
        kps, d = test_inputs(cols, rows, cam, n_random)
        for T in poses():
            pos, valid = unproject_stereo(cam, T, kps, d)
            lines.append("case %s %s" % (name, " ".join(hx(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))))
            lines.append("pose %s" % " ".join(hx(v) for v in np.asarray(T, f32).reshape(16)))
            lines.append("points %d" % len(kps))
            lines += ["%s %s %s %d %s %s %s" % (hx(k["x"]), hx(k["y"]), hx(z), v, hx(p[0]), hx(p[1]), hx(p[2]))
                      for k, z, v, p in zip(kps, d, valid, pos)]
    return "\n".join(lines) + "\n"


test_inputs.__test__ = False

if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (os.path.join(root, "cooperative-orb-slam_amd"), os.path.join(root, "oracle"), here):
        sys.path.insert(0, p)
    with open(os.path.join(here, "golden", FIXTURE), "w") as f:
        f.write(fixture_text())

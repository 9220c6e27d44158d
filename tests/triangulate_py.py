"""The per-match body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:284-450) with its per-pair baseline test
(:244-261) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:330-371) of a point with its two observations, restated in
pure Python on numpy float32 / float64 scalars, one operation per rounding and one match at a time: the yardstick of
csrc/triangulate.c and of k_create_map_points (triangulate_kernels.hip, frame_math.h). It also holds the scenes the
tests use.

cv::Mat float arithmetic as pinned in DESIGN.md "Pinned semantics" (include/orbslam_amd.h states every line):
  xn = ((u - cx) * invfx, (v - cy) * invfy, 1), invfx = 1.0f / fx; ray = Rwc * xn, the small-matrix gemm without an
  addend (three float products summed in float); cosParallaxRays = (float)(dot_d / (norm_d * norm_d));
  cosParallaxStereo = cosf(2 * atan2f(mb / 2, depth)), libm's float overloads; the 4x4 system of :322-326 in float
  (product, then difference); cv::SVD::compute = OpenCV 3.x's one-sided Jacobi on the transposed matrix (svd4_null);
  x3D / w = x * (float)(1.0 / (double)w); z = (float)(dot_d(Rcw.row(2), x3D) + (double)tcw[2]), x and y likewise;
  invz = (float)(1.0 / (double)z); u, v, u_r in float, left to right; err2 in float, compared in double with
  5.991 * sigma2 (7.8 with mvuRight); dist = (float)norm_d(x3D - Ow); the two float comparisons of :430;
  normal = ((0 + n1 * (float)(1.0 / norm_d(n1))) + n2 * (float)(1.0 / norm_d(n2))) * 0.5f; max = dist1 * sf[oct1],
  min = max / sf[nlevels - 1].
"""
import ctypes
import os
import sys

import numpy as np

import unproject_py as UP

f32, f64 = np.float32, np.float64

# one code per outcome, in the order of the reference's tests
(NO_MATCH, TRIANGULATED, STEREO1, STEREO2, BASELINE, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, DIST_ZERO,
 SCALE_RATIO, EXCLUDED) = range(14)
NAMES = ("NO_MATCH", "TRIANGULATED", "STEREO1", "STEREO2", "BASELINE", "LOW_PARALLAX", "W_ZERO", "Z1", "Z2", "REPROJ1",
         "REPROJ2", "DIST_ZERO", "SCALE_RATIO", "EXCLUDED")
CREATED = (TRIANGULATED, STEREO1, STEREO2)

_libm = ctypes.CDLL("libm.so.6")
_libm.atan2f.restype, _libm.atan2f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
_libm.cosf.restype, _libm.cosf.argtypes = ctypes.c_float, [ctypes.c_float]


def atan2f(y, x):
    return f32(_libm.atan2f(float(y), float(x)))


def cosf(x):
    return f32(_libm.cosf(float(x)))


def cos_parallax_stereo(mb, depth):
    """:312 / :314: cos(2 * atan2(mb / 2, depth)) on floats = cosf(2 * atan2f(...))"""
    return cosf(f32(f32(2.0) * atan2f(f32(f32(mb) * f32(0.5)), f32(depth))))


class TriGeom:
    """what the loop reads of the two keyframes (both use it): camera, mbf, mb, mnScaleLevels, mvScaleFactors,
    mvLevelSigma2"""

    def __init__(self, fx, fy, cx, cy, bf, b=None, nlevels=8, scale_factor=1.2):
        self.fx, self.fy, self.cx, self.cy, self.bf = (f32(v) for v in (fx, fy, cx, cy, bf))
        self.b = f32(self.bf / self.fx) if b is None else f32(b)
        self.nlevels = int(nlevels)
        s = [f32(1.0)]
        for _ in range(1, 16):
            s.append(f32(s[-1] * f32(scale_factor)))
        self.scale_factors = np.array(s, f32)
        self.level_sigma2 = np.array([f32(v * v) for v in s], f32)

    def cstruct(self):
        from orbamd._lib import OrbmTriGeom
        g = OrbmTriGeom()
        g.fx, g.fy, g.cx, g.cy, g.bf, g.b = (float(v) for v in (self.fx, self.fy, self.cx, self.cy, self.bf, self.b))
        g.nlevels = self.nlevels
        for i in range(16):
            g.scale_factors[i] = float(self.scale_factors[i])
            g.level_sigma2[i] = float(self.level_sigma2[i])
        return g


def camera_geom(name, bf=40.0):
    import undistort_py as U
    cam = U.CAMERAS[name][0]
    return TriGeom(cam.fx, cam.fy, cam.cx, cam.cy, bf)


def norm_d(v):
    s = f64(0)
    for k in range(len(v)):
        s = s + f64(v[k]) * f64(v[k])
    return np.sqrt(s)


def dot_d(a, b):
    s = f64(0)
    for k in range(len(a)):
        s = s + f64(a[k]) * f64(b[k])
    return s


def baseline_skips(Ow1, Ow2, monocular, mb, median_depth2):
    """:244-261"""
    vb = [f32(Ow2[k] - Ow1[k]) for k in range(3)]
    baseline = f32(norm_d(vb))
    if not monocular:
        return bool(baseline < f32(mb))
    return bool(f64(f32(baseline / f32(median_depth2))) < f64(0.01))


def svd4_null(A, stats=None):
    """vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a 4x4 float A: JacobiSVDImpl_ of OpenCV 3.x
    (a build without LAPACK) on At = A.t(), with sqrt(p*p + beta*beta) where OpenCV calls hypot"""
    At = [[f32(A[k][i]) for k in range(4)] for i in range(4)]
    Vt = [[f32(1.0) if i == k else f32(0.0) for k in range(4)] for i in range(4)]
    W = [dot_d(At[i], At[i]) for i in range(4)]
    eps = f32(np.finfo(f32).eps * f32(2))
    sweeps = 0
    for _ in range(30):
        changed = False
        sweeps += 1
        for i in range(3):
            for j in range(i + 1, 4):
                a, b = W[i], W[j]
                p = dot_d(At[i], At[j])
                if abs(p) <= f64(eps) * np.sqrt(a * b):
                    continue
                p = p * f64(2)
                beta = a - b
                gamma = np.sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * f64(0.5)
                    s = f32(np.sqrt(delta / gamma))
                    c = f32(p / (gamma * f64(s) * f64(2)))
                else:
                    c = f32(np.sqrt((gamma + beta) / (gamma * f64(2))))
                    s = f32(p / (gamma * f64(c) * f64(2)))
                a = b = f64(0)
                for k in range(4):
                    t0 = f32(f32(c * At[i][k]) + f32(s * At[j][k]))
                    t1 = f32(f32(f32(-s) * At[i][k]) + f32(c * At[j][k]))
                    At[i][k], At[j][k] = t0, t1
                    a = a + f64(t0) * f64(t0)
                    b = b + f64(t1) * f64(t1)
                W[i], W[j] = a, b
                changed = True
                for k in range(4):
                    t0 = f32(f32(c * Vt[i][k]) + f32(s * Vt[j][k]))
                    t1 = f32(f32(f32(-s) * Vt[i][k]) + f32(c * Vt[j][k]))
                    Vt[i][k], Vt[j][k] = t0, t1
        if not changed:
            break
    if stats is not None:
        stats["sweeps"] = max(stats.get("sweeps", 0), sweeps)
    W = [np.sqrt(dot_d(At[i], At[i])) for i in range(4)]
    for i in range(3):  # selection sort, descending, strict <
        j = i
        for k in range(i + 1, 4):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    return Vt[3]


def system_matrix(T1, T2, xn1, xn2):
    """:322-326"""
    A = []
    for T, xn in ((T1, xn1), (T2, xn2)):
        for r in range(2):
            A.append([f32(f32(xn[r] * T[2, k]) - T[r, k]) for k in range(4)])
    return A


def _finite(*v):
    return bool(np.isfinite(np.array(v, f64)).all())


def triangulate_one(g, T1, Ow1, T2, Ow2, kp1, ur1, d1, kp2, ur2, d2, stats=None):
    """one match of a pair that passed the baseline test: (status, x3D, normal, min_dist, max_dist); kp = (x, y,
    octave). T1 / T2 finite 4x4 float32."""
    none = ([f32(0)] * 3, [f32(0)] * 3, f32(0), f32(0))
    u1, v1, o1 = f32(kp1[0]), f32(kp1[1]), int(kp1[2])
    u2, v2, o2 = f32(kp2[0]), f32(kp2[1]), int(kp2[2])
    ur1, ur2, d1, d2 = f32(ur1), f32(ur2), f32(d1), f32(d2)
    if not (0 <= o1 < g.nlevels and 0 <= o2 < g.nlevels and _finite(u1, v1, u2, v2, ur1, ur2)):
        return (EXCLUDED,) + none
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)  # :293, :297
    if (st1 or st2) and not (np.isfinite(g.b) and g.b > 0):
        return (EXCLUDED,) + none
    if (st1 and not (np.isfinite(d1) and d1 > 0)) or (st2 and not (np.isfinite(d2) and d2 > 0)):
        return (EXCLUDED,) + none
    invfx, invfy = f32(1.0) / g.fx, f32(1.0) / g.fy
    xn1 = [f32(f32(u1 - g.cx) * invfx), f32(f32(v1 - g.cy) * invfy), f32(1.0)]  # :300-301
    xn2 = [f32(f32(u2 - g.cx) * invfx), f32(f32(v2 - g.cy) * invfy), f32(1.0)]
    ray1 = [f32(f32(f32(T1[0, i] * xn1[0]) + f32(T1[1, i] * xn1[1])) + f32(T1[2, i] * xn1[2])) for i in range(3)]
    ray2 = [f32(f32(f32(T2[0, i] * xn2[0]) + f32(T2[1, i] * xn2[1])) + f32(T2[2, i] * xn2[2])) for i in range(3)]
    cos_rays = f32(dot_d(ray1, ray2) / (norm_d(ray1) * norm_d(ray2)))  # :305
    if not np.isfinite(cos_rays):
        return (EXCLUDED,) + none
    cs1 = cs2 = f32(cos_rays + f32(1.0))
    if st1:
        cs1 = cos_parallax_stereo(g.b, d1)
    elif st2:
        cs2 = cos_parallax_stereo(g.b, d2)
    cs = cs2 if cs2 < cs1 else cs1  # std::min
    if cos_rays < cs and cos_rays > f32(0) and (st1 or st2 or f64(cos_rays) < f64(0.9998)):  # :319
        x4 = svd4_null(system_matrix(T1, T2, xn1, xn2), stats)
        if not _finite(*x4):
            return (EXCLUDED,) + none
        if x4[3] == f32(0):
            return (W_ZERO,) + none
        sc = f32(f64(1.0) / f64(x4[3]))
        x3D = [f32(x4[k] * sc) for k in range(3)]
        made = TRIANGULATED
    elif st1 and cs1 < cs2:
        x3D = UP.unproject_one(g.fx, g.fy, g.cx, g.cy, T1, Ow1, u1, v1, d1)
        made = STEREO1
    elif st2 and cs2 < cs1:
        x3D = UP.unproject_one(g.fx, g.fy, g.cx, g.cy, T2, Ow2, u2, v2, d2)
        made = STEREO2
    else:
        return (LOW_PARALLAX,) + none
    if not _finite(*x3D):
        return (EXCLUDED,) + none
    cam = []
    for T in (T1, T2):
        cam.append([f32(dot_d(T[r, :3], x3D) + f64(T[r, 3])) for r in range(3)])
    if not _finite(*(cam[0] + cam[1])):
        return (EXCLUDED,) + none
    if cam[0][2] <= 0:
        return (Z1,) + none
    if cam[1][2] <= 0:
        return (Z2,) + none
    for which, (x, y, z), u, v, ur, st, o in ((REPROJ1, cam[0], u1, v1, ur1, st1, o1),
                                              (REPROJ2, cam[1], u2, v2, ur2, st2, o2)):
        sigma2 = g.level_sigma2[o]
        invz = f32(f64(1.0) / f64(z))
        pu = f32(f32(f32(g.fx * x) * invz) + g.cx)
        pv = f32(f32(f32(g.fy * y) * invz) + g.cy)
        ex, ey = f32(pu - u), f32(pv - v)
        e2 = f32(f32(ex * ex) + f32(ey * ey))
        th = f64(5.991)
        if st:
            pur = f32(pu - f32(g.bf * invz))  # KF1's mbf for both (:380, :406)
            er = f32(pur - ur)
            e2 = f32(e2 + f32(er * er))
            th = f64(7.8)
        if not np.isfinite(e2):
            return (EXCLUDED,) + none
        if f64(e2) > th * f64(sigma2):
            return (which,) + none
    n1 = [f32(x3D[k] - Ow1[k]) for k in range(3)]
    n2 = [f32(x3D[k] - Ow2[k]) for k in range(3)]
    nd1, nd2 = norm_d(n1), norm_d(n2)
    dist1, dist2 = f32(nd1), f32(nd2)
    if not _finite(dist1, dist2):
        return (EXCLUDED,) + none
    if dist1 == 0 or dist2 == 0:
        return (DIST_ZERO,) + none
    ratio_dist = f32(dist2 / dist1)
    ratio_octave = f32(g.scale_factors[o1] / g.scale_factors[o2])
    ratio_factor = f32(f32(1.5) * g.scale_factors[1])
    if not np.isfinite(ratio_dist):
        return (EXCLUDED,) + none
    if f32(ratio_dist * ratio_factor) < ratio_octave or ratio_dist > f32(ratio_octave * ratio_factor):
        return (SCALE_RATIO,) + none
    s1, s2 = f32(f64(1.0) / nd1), f32(f64(1.0) / nd2)
    normal = [f32(f32(f32(f32(0.0) + f32(n1[k] * s1)) + f32(n2[k] * s2)) * f32(0.5)) for k in range(3)]
    max_dist = f32(dist1 * g.scale_factors[o1])
    min_dist = f32(max_dist / g.scale_factors[g.nlevels - 1])
    return made, x3D, normal, min_dist, max_dist


class Result:
    """what orbx_triangulate_matches writes for one pair"""

    def __init__(self, n1):
        self.status = np.zeros(n1, np.int8)
        self.pos3 = np.zeros((n1, 3), f32)
        self.tab_pos, self.tab_normal = np.zeros((n1, 3), f32), np.zeros((n1, 3), f32)
        self.tab_min, self.tab_max = np.zeros(n1, f32), np.zeros(n1, f32)
        self.tab_desc = np.zeros((n1, 32), np.uint8)
        self.tab_flags = np.zeros(n1, np.uint8)
        self.feat1, self.feat2 = np.zeros(n1, np.int32), np.zeros(n1, np.int32)
        self.nnew = 0

    FIELDS = ("status", "pos3", "tab_pos", "tab_normal", "tab_min", "tab_max", "tab_desc", "tab_flags", "feat1",
              "feat2")

    def same_as(self, other):
        """raw bits of every array (table rows past nnew are not compared) and nnew"""
        if self.nnew != other.nnew or len(self.status) != len(other.status):
            return False
        for k in self.FIELDS:
            a, b = getattr(self, k), getattr(other, k)
            if k not in ("status", "pos3"):
                a, b = a[:self.nnew], b[:self.nnew]
            if np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes():
                return False
        return True


def triangulate_matches(g, monocular, median_depth2, T1, T2, kps1, ur1, d1, desc1, kps2, ur2, d2, match12, stats=None):
    """one pair (current keyframe 1, neighbour 2): kps = orbx_kp structured arrays (mvKeysUn), ur / d = mvuRight /
    mvDepth or None (monocular, all -1), desc1 uint8 [n1, 32], match12 int32 [n1] (idx2 or negative)"""
    n1, n2 = len(kps1), len(kps2)
    R = Result(n1)
    T1 = np.asarray(T1, f32).reshape(4, 4)
    T2 = np.asarray(T2, f32).reshape(4, 4)
    ur1 = np.full(n1, -1, f32) if ur1 is None else ur1
    d1 = np.full(n1, -1, f32) if d1 is None else d1
    ur2 = np.full(n2, -1, f32) if ur2 is None else ur2
    d2 = np.full(n2, -1, f32) if d2 is None else d2
    with np.errstate(all="ignore"):
        pose_ok = _finite(*T1[:3].ravel()) and _finite(*T2[:3].ravel())
        Ow1, Ow2 = UP.camera_center(T1), UP.camera_center(T2)
        skip = pose_ok and baseline_skips(Ow1, Ow2, monocular, g.b, median_depth2)
        for i in range(n1):
            idx2 = int(match12[i])
            if idx2 < 0:
                continue
            if not pose_ok or idx2 >= n2:
                R.status[i] = EXCLUDED
                continue
            if skip:
                R.status[i] = BASELINE
                continue
            k1, k2 = kps1[i], kps2[idx2]
            st, x3D, normal, mind, maxd = triangulate_one(
                g, T1, Ow1, T2, Ow2, (k1["x"], k1["y"], k1["octave"]), ur1[i], d1[i],
                (k2["x"], k2["y"], k2["octave"]), ur2[idx2], d2[idx2], stats)
            R.status[i] = st
            if st in CREATED:
                R.pos3[i] = x3D
                r = R.nnew
                R.tab_pos[r], R.tab_normal[r], R.tab_min[r], R.tab_max[r] = x3D, normal, mind, maxd
                R.tab_desc[r] = desc1[i]  # the current keyframe's descriptor (DESIGN.md "Pinned semantics")
                R.tab_flags[r] = 9
                R.feat1[r], R.feat2[r] = i, idx2
                R.nnew += 1
    return R


# ------------------------------------------------------------------------------------------------ scenes
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])


def rot_xyz(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(f32)


def relative_poses():
    """(name, Tcw1, Tcw2): a lateral baseline, a forward motion, a rotation plus translation"""
    R0 = rot_xyz(0.02, -0.03, 0.01)
    T1 = pose(R0, [0.1, -0.2, 0.3])
    out = [("lateral", T1, pose(R0, [0.1 - 0.6, -0.2, 0.3])),
           ("forward", T1, pose(R0, [0.1 + 0.05, -0.2, 0.3 - 0.8])),
           ("rot+trans", T1, pose(rot_xyz(0.05, 0.12, -0.04) @ R0, [0.1 - 0.5, -0.1, 0.2]))]
    return out


class Pair:
    """one pair's inputs as the host unit takes them"""

    def __init__(self, name, g, T1, T2, kps1, ur1, d1, desc1, kps2, ur2, d2, match12, monocular=0, median_depth2=1.0):
        self.name, self.g, self.T1, self.T2 = name, g, T1, T2
        self.kps1, self.ur1, self.d1, self.desc1 = kps1, ur1, d1, desc1
        self.kps2, self.ur2, self.d2, self.match12 = kps2, ur2, d2, match12
        self.monocular, self.median_depth2 = monocular, median_depth2

    def run(self, fn, **kw):
        return fn(self.g, self.monocular, self.median_depth2, self.T1, self.T2, self.kps1, self.ur1, self.d1,
                  self.desc1, self.kps2, self.ur2, self.d2, self.match12, **kw)


def _project(g, T, X):
    Xc = X @ np.asarray(T, f64)[:3, :3].T + np.asarray(T, f64)[:3, 3]
    z = Xc[:, 2]
    return float(g.fx) * Xc[:, 0] / z + float(g.cx), float(g.fy) * Xc[:, 1] / z + float(g.cy), z


def generated_pair(g, name, T1, T2, mode, n, seed, n2_extra=20):
    """n matches between two views of random points: mode 'stereo' (every keypoint has mvuRight), 'mono' (none) or
    'mixed' (each side at random). A share of the rows is pushed towards each test of the loop: far points (low
    parallax), points behind a camera, pixel noise beyond the chi-square bounds, wrong octaves (scale ratio), a wrong
    stereo depth; and rows the contract excludes."""
    rng = np.random.default_rng(seed)
    n2 = n + n2_extra
    T1d = np.asarray(T1, f64)
    R1, t1 = T1d[:3, :3], T1d[:3, 3]
    kind = rng.choice(12, n, p=[0.34, 0.1, 0.06, 0.06, 0.08, 0.08, 0.08, 0.05, 0.05, 0.04, 0.03, 0.03])
    z = rng.uniform(2.0, 12.0, n)
    z[kind == 1] = rng.uniform(300.0, 3000.0, (kind == 1).sum())  # far: parallax below the thresholds
    behind2 = (kind == 3) & (name == "forward")  # in front of camera 1, behind camera 2, which moved past them
    z[behind2] = rng.uniform(0.15, 0.6, behind2.sum())
    u = rng.uniform(40, 600, n)
    v = rng.uniform(40, 440, n)
    Xc = np.stack([(u - float(g.cx)) / float(g.fx) * z, (v - float(g.cy)) / float(g.fy) * z, z], 1)
    X = (Xc - t1) @ R1  # world
    u1, v1, z1 = _project(g, T1, X)
    u2, v2, z2 = _project(g, T2, X)
    noise = lambda s: rng.normal(0, s, n)  # noqa: E731
    u1, v1, u2, v2 = u1 + noise(0.3), v1 + noise(0.3), u2 + noise(0.3), v2 + noise(0.3)
    # kind 2 / 3: a match whose rays meet behind camera 1 / 2 (the second pixel mirrored about the first)
    m = kind == 2
    u2[m] = 2 * u1[m] - u2[m] + 30
    m = (kind == 3) & ~behind2
    u2[m] = u2[m] + np.where(rng.random(m.sum()) < 0.5, -1, 1) * rng.uniform(80, 200, m.sum())
    # kind 4 / 5: pixel noise beyond the chi-square bound in view 1 / 2, across the epipolar line
    v1[kind == 4] += rng.choice([-1, 1], (kind == 4).sum()) * rng.uniform(4, 12, (kind == 4).sum())
    v2[kind == 5] += rng.choice([-1, 1], (kind == 5).sum()) * rng.uniform(4, 12, (kind == 5).sum())
    oct1 = rng.integers(0, 3, n)
    oct2 = oct1.copy()
    m = kind == 6  # octaves that contradict the distance ratio
    oct1[m] = np.where(rng.random(m.sum()) < 0.5, 0, 7)
    oct2[m] = 7 - oct1[m]
    if mode == "stereo":
        s1, s2 = np.ones(n, bool), np.ones(n, bool)
    elif mode == "mono":
        s1, s2 = np.zeros(n, bool), np.zeros(n, bool)
    else:
        s1, s2 = rng.random(n) < 0.5, rng.random(n) < 0.5
    d1 = z1.copy()
    d2 = z2.copy()
    m = kind == 9  # a stereo depth far off the triangulated one
    d1[m] *= rng.uniform(1.5, 3.0, m.sum())
    d2[m] *= rng.uniform(1.5, 3.0, m.sum())
    bf = float(g.bf)
    ur1 = np.where(s1, u1 - bf / d1, -1.0)
    ur2 = np.where(s2, u2 - bf / d2, -1.0)
    s1 &= (ur1 >= 0) & (d1 > 0)  # a keypoint has mvuRight only with a positive mvDepth
    s2 &= (ur2 >= 0) & (d2 > 0)
    ur1, ur2 = np.where(s1, ur1, -1.0), np.where(s2, ur2, -1.0)
    d1, d2 = np.where(s1, d1, -1.0), np.where(s2, d2, -1.0)
    kps1, kps2 = np.zeros(n, KP), np.zeros(n2, KP)
    perm = rng.permutation(n2)[:n]  # idx2 of row i
    kps1["x"], kps1["y"], kps1["octave"] = u1, v1, oct1
    kps2["x"], kps2["y"] = rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)
    kps2["octave"] = rng.integers(0, 8, n2)
    kps2["x"][perm], kps2["y"][perm], kps2["octave"][perm] = u2, v2, oct2
    U2, D2 = np.full(n2, -1.0), np.full(n2, -1.0)
    U2[perm], D2[perm] = ur2, d2
    match = perm.astype(np.int32)
    match[kind == 10] = -1 - rng.integers(0, 2, (kind == 10).sum())  # no match (-1 / -2)
    ex = np.flatnonzero(kind == 11)  # excluded by the contract, four ways
    for j, i in enumerate(ex):
        if j % 4 == 0:
            match[i] = n2 + j
        elif j % 4 == 1:
            kps1["octave"][i] = 8 + j
        elif j % 4 == 2:
            kps2["octave"][match[i]] = -1
        else:
            kps1["y"][i] = np.nan
    desc1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return Pair("%s/%s" % (name, mode), g, T1, T2, kps1, ur1.astype(f32), d1.astype(f32), desc1, kps2, U2.astype(f32),
                D2.astype(f32), match)


def near_stereo_pair(g, T1, mode, n, seed):
    """a neighbour 1.5 baselines ahead looking at near points: the rays' parallax is below the stereo rig's own, so
    the points come from a keyframe's stereo (:340-347); KF1's where it has mvuRight, else KF2's"""
    rng = np.random.default_rng(seed)
    T1d = np.asarray(T1, f64)
    R1, t1 = T1d[:3, :3], T1d[:3, 3]
    T2 = pose(R1, t1 + np.array([0.0, 0.0, -1.5 * float(g.b)]))  # forward: little parallax near the image centre
    z = rng.uniform(1.0, 4.0, n)
    u, v = float(g.cx) + rng.uniform(-90, 90, n), float(g.cy) + rng.uniform(-90, 90, n)
    Xc = np.stack([(u - float(g.cx)) / float(g.fx) * z, (v - float(g.cy)) / float(g.fy) * z, z], 1)
    X = (Xc - t1) @ R1
    u1, v1, z1 = _project(g, T1, X)
    u2, v2, z2 = _project(g, T2, X)
    u1, v1, u2, v2 = (a + rng.normal(0, 0.2, n) for a in (u1, v1, u2, v2))
    s1 = rng.random(n) < (1.0 if mode == "stereo" else 0.5)
    s2 = np.ones(n, bool) if mode == "stereo" else ~s1 | (rng.random(n) < 0.3)
    bf = float(g.bf)
    ur1, ur2 = np.where(s1, u1 - bf / z1, -1.0), np.where(s2, u2 - bf / z2, -1.0)
    s1 &= ur1 >= 0
    s2 &= ur2 >= 0
    kps1, kps2 = np.zeros(n, KP), np.zeros(n, KP)
    kps1["x"], kps1["y"], kps2["x"], kps2["y"] = u1, v1, u2, v2
    kps1["octave"] = kps2["octave"] = rng.integers(0, 4, n)
    desc1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return Pair("near/%s" % mode, g, T1, T2, kps1, np.where(s1, ur1, -1.0).astype(f32),
                np.where(s1, z1, -1.0).astype(f32), desc1, kps2, np.where(s2, ur2, -1.0).astype(f32),
                np.where(s2, z2, -1.0).astype(f32), np.arange(n, dtype=np.int32))


def short_baseline_pair(g, T1, monocular, n=12, seed=3):
    """a neighbour closer than mb (stereo) or than a hundredth of the scene's median depth (monocular): :251, :259"""
    rng = np.random.default_rng(seed)
    T2 = np.array(T1, f32)
    T2[0, 3] = f32(T2[0, 3] - f32(0.5) * g.b)
    kps1, kps2 = np.zeros(n, KP), np.zeros(n, KP)
    for k in (kps1, kps2):
        k["x"], k["y"] = rng.uniform(50, 600, n), rng.uniform(50, 400, n)
    match = np.arange(n, dtype=np.int32)
    match[::6] = -1
    desc1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return Pair("short-baseline/%d" % monocular, g, T1, T2, kps1, None, None, desc1, kps2, None, None, match,
                monocular=monocular, median_depth2=f32(float(g.b) * 0.5 / 0.009))


def w_zero_pair(g, n=12):
    """w == 0 needs parallel rays, which the parallax test rejects under rigid poses; the 4x4 system reads mTcw and
    the rays read mRwc, so a neighbour "pose" that is no rigid motion separates them: column 0 of the system is zero
    for both views (the null vector is (1, 0, 0, 0), untouched by the Jacobi rotations) while the rays keep an angle.
    KF1 looks along world x at its principal point; KF2's column 0 is its own xn (exactly, z row 1)."""
    T1 = np.array([[0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]], f32)
    kps1, kps2 = np.zeros(n, KP), np.zeros(n, KP)
    kps1["x"], kps1["y"] = g.cx, g.cy
    u2, v2 = f32(g.cx + f32(64.0)), f32(g.cy - f32(32.0))
    kps2["x"], kps2["y"] = u2, v2
    xn = [f32(f32(u2 - g.cx) * (f32(1.0) / g.fx)), f32(f32(v2 - g.cy) * (f32(1.0) / g.fy))]
    T2 = np.array([[xn[0], 0.5, -1, 0.25], [xn[1], 1, 0.5, -0.5], [1, 0.5, 0.25, 1.0], [0, 0, 0, 1]], f32)
    kps1["octave"] = np.arange(n) % 3
    kps2["octave"] = np.arange(n) % 2
    desc1 = np.arange(n * 32, dtype=np.uint8).reshape(n, 32)
    return Pair("w-zero", g, T1, T2, kps1, None, None, desc1, kps2, None, None, np.arange(n, dtype=np.int32))


def dist_zero_pair(g, n=12):
    """dist == 0 needs x3D == mOw, where a rigid pose has z == 0; under a "pose" with mRcw = 2 I and mtcw = (0, 0, -1),
    mOw = (0, 0, 2) and z1 = 3 there. KF1's stereo point at depth 1e-30 is mOw itself; KF2 (identity) sees it at its
    principal point."""
    T1 = np.array([[2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 2, -1], [0, 0, 0, 1]], f32)
    T2 = np.eye(4, dtype=f32)
    kps1, kps2 = np.zeros(n, KP), np.zeros(n, KP)
    kps1["x"], kps1["y"], kps2["x"], kps2["y"] = g.cx, g.cy, g.cx, g.cy
    kps2["x"] += (np.arange(n) % 4).astype(f32) * f32(0.25)
    kps1["octave"] = kps2["octave"] = np.arange(n) % 3
    invz = f32(f64(1.0) / f64(3.0))
    ur1 = np.full(n, f32(g.cx - f32(g.bf * invz)), f32)
    d1 = np.full(n, 1e-30, f32)
    desc1 = np.arange(n * 32, dtype=np.uint8).reshape(n, 32)
    return Pair("dist-zero", g, T1, T2, kps1, ur1, d1, desc1, kps2, None, None, np.arange(n, dtype=np.int32))


def camera_scene(name, n=300):
    """every pair of one camera's scene: three relative poses x (stereo, mono, mixed) of n matches, near points for
    the stereo creation branches, both baseline skips and the two degenerate pairs"""
    g = camera_geom(name)
    ci = sorted(("my", "tum1", "euroc")).index(name) if name in ("my", "tum1", "euroc") else 7
    pairs = []
    for pi, (pname, T1, T2) in enumerate(relative_poses()):
        for mi, mode in enumerate(("stereo", "mono", "mixed")):
            pairs.append(generated_pair(g, pname, T1, T2, mode, n, 1000 * ci + 10 * pi + mi))
    T1 = relative_poses()[0][1]
    pairs.append(near_stereo_pair(g, T1, "stereo", 40, 50 + ci))
    pairs.append(near_stereo_pair(g, T1, "mixed", 60, 60 + ci))
    pairs.append(short_baseline_pair(g, T1, 0))
    pairs.append(short_baseline_pair(g, T1, 1))
    pairs.append(w_zero_pair(g))
    pairs.append(dist_zero_pair(g))
    return g, pairs


FIXTURE = "triangulate_vectors.txt"  # under tests/golden/


def fixture_pairs():
    g = camera_geom("euroc")
    _, T1, T2 = relative_poses()[1]
    return [generated_pair(g, "forward", T1, T2, "mixed", 60, 4242), near_stereo_pair(g, T1, "mixed", 30, 4243),
            short_baseline_pair(g, T1, 0), short_baseline_pair(g, T1, 1), w_zero_pair(g, 4), dist_zero_pair(g, 4)]


def fixture_text():
    """the vectors tests/cpp/test_triangulate.c reads, every float as the hex of its bits. Per pair: a line `pair
    <name> <monocular> <median_depth2> <n1> <n2> <nnew>`, `geom <fx fy cx cy bf b> <nlevels> <16 scale factors> <16
    sigma2>`, `pose <16 words>` twice, n1 lines `<x y> <octave> <uright depth> <match12> <status> <pos3>`, n2 lines
    `<x y> <octave> <uright depth>`, nnew lines `<pos 3> <normal 3> <min max> <feat1> <feat2>`. The program makes up
    the descriptors."""
    def hx(v):
        return "%08x" % int(np.array(v, f32).view(np.uint32))

    def hs(vs):
        return " ".join(hx(v) for v in vs)
    lines = []
    for p in fixture_pairs():
        g = p.g
        r = p.run(triangulate_matches)
        n1, n2 = len(p.kps1), len(p.kps2)
        lines.append("pair %s %d %s %d %d %d" % (p.name, p.monocular, hx(p.median_depth2), n1, n2, r.nnew))
        lines.append("geom %s %d %s %s" % (hs((g.fx, g.fy, g.cx, g.cy, g.bf, g.b)), g.nlevels, hs(g.scale_factors),
                                           hs(g.level_sigma2)))
        lines.append("pose %s" % hs(np.asarray(p.T1, f32).reshape(16)))
        lines.append("pose %s" % hs(np.asarray(p.T2, f32).reshape(16)))
        ur1 = np.full(n1, -1, f32) if p.ur1 is None else p.ur1
        d1 = np.full(n1, -1, f32) if p.d1 is None else p.d1
        ur2 = np.full(n2, -1, f32) if p.ur2 is None else p.ur2
        d2 = np.full(n2, -1, f32) if p.d2 is None else p.d2
        for i in range(n1):
            k = p.kps1[i]
            lines.append("%s %d %s %d %d %s" % (hs((k["x"], k["y"])), k["octave"], hs((ur1[i], d1[i])), p.match12[i],
                                                r.status[i], hs(r.pos3[i])))
        for i in range(n2):
            k = p.kps2[i]
            lines.append("%s %d %s" % (hs((k["x"], k["y"])), k["octave"], hs((ur2[i], d2[i]))))
        for j in range(r.nnew):
            lines.append("%s %s %s %d %d" % (hs(r.tab_pos[j]), hs(r.tab_normal[j]), hs((r.tab_min[j], r.tab_max[j])),
                                             r.feat1[j], r.feat2[j]))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    with open(os.path.join(here, "golden", FIXTURE), "w") as f:
        f.write(fixture_text())
    for cam in ("my", "tum1", "euroc"):
        g, pairs = camera_scene(cam)
        tot = np.zeros(14, int)
        st = {}
        for p in pairs:
            r = p.run(triangulate_matches, stats=st)
            c = np.bincount(r.status, minlength=14)
            tot += c
            print(cam, p.name, dict((NAMES[k], int(c[k])) for k in range(14) if c[k]))
        print(cam, "total", dict(zip(NAMES, tot.tolist())), st)

"""Frame::isInFrustum (Frame.cc:274-330) with MapPoint::PredictScale (MapPoint.cc:385-417) restated in pure Python on
numpy float32 / float64 scalars, one operation per rounding: the yardstick of csrc/frustum.c and of the frustum kernels
(local_kernels.hip, frame_math.h).

cv::Mat float arithmetic as pinned in DESIGN.md "Pinned semantics":
  Pc = mRcw * P + mtcw: the small-matrix gemm, the row's three float products summed in float, then
       (float)((double)t + (double)mtcw[i]);
  PcZ < 0.0f rejects; invz = 1.0f / PcZ, a float divide;
  u = fx * PcX * invz + cx, v = fy * PcY * invz + cy in float, left to right; the four bounds tests;
  mOw = -mRcw.t() * mtcw: GEMM_1_T, double accumulation from 0, (float)(-1.0 * s); PO = P - mOw in float;
  dist = (float)sqrt(sum of (double)PO^2); dist < 0.8f * min_dist || dist > 1.2f * max_dist rejects;
  viewCos = (float)(dot in double / (double)dist); viewCos < limit rejects;
  ratio = max_dist / dist; level = ceilf(logf(ratio) / log_scale_factor) clamped to [0, nlevels - 1], logf = libm's;
  xr = u - bf * invz.
The contract (include/orbslam_amd.h): a non-finite pose entry or point field, a non-finite Pc, u, v, dist or viewCos,
PcZ == +-0, dist == 0 and a ratio that is not a positive normal float reject the point (EXCLUDED).
"""
import ctypes
import math
import os
import sys

import numpy as np

f32, f64 = np.float32, np.float64

# why a point is not in view, in the order of the tests; IN_VIEW = it is
IN_VIEW, DEPTH, BOUNDS_U, BOUNDS_V, DISTANCE, VIEW_COS, EXCLUDED = range(7)
REJECTIONS = (DEPTH, BOUNDS_U, BOUNDS_V, DISTANCE, VIEW_COS)

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]


def logf(x):
    return f32(_libm.logf(float(x)))


def positive_normal(x):
    u = int(np.array(x, f32).view(np.uint32))
    return 0x00800000 <= u < 0x7f800000


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


class Geom:
    """what isInFrustum reads of the Frame: camera, mbf, image bounds, mnScaleLevels, mfLogScaleFactor (and the grid
    inverses and mvScaleFactors, which the search after it reads)"""

    def __init__(self, fx, fy, cx, cy, bf, bounds, nlevels=8, scale_factor=1.2, b=None):
        self.fx, self.fy, self.cx, self.cy, self.bf = (f32(v) for v in (fx, fy, cx, cy, bf))
        self.b = f32(self.bf / self.fx) if b is None else f32(b)
        self.min_x, self.max_x, self.min_y, self.max_y = (f32(v) for v in bounds)
        self.grid_w_inv = f32(f32(64.0) / f32(self.max_x - self.min_x))
        self.grid_h_inv = f32(f32(48.0) / f32(self.max_y - self.min_y))
        self.nlevels = int(nlevels)
        s = [f32(1.0)]
        for _ in range(1, nlevels):  # mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor (ORBextractor.cc:416-424)
            s.append(f32(s[-1] * f32(scale_factor)))
        self.scale_factors = np.array(s, f32)
        self.log_scale_factor = f32(math.log(float(f32(scale_factor))))  # mfLogScaleFactor = log(mfScaleFactor)

    def cstruct(self):
        from orbamd.frame import track_geom
        return track_geom(self.fx, self.fy, self.cx, self.cy, self.bf, self.b,
                          (self.min_x, self.max_x, self.min_y, self.max_y), self.grid_w_inv, self.grid_h_inv,
                          self.scale_factors)


def camera_geom(name, bf=40.0):
    """the Geom of one of undistort_py's reference cameras (its undistorted image bounds)"""
    import undistort_py as U
    cam, cols, rows = U.CAMERAS[name]
    b, _, _ = U.image_bounds(cam, cols, rows)
    return Geom(cam.fx, cam.fy, cam.cx, cam.cy, bf, b)


# cx = cy = 0 and a power-of-two focal length: with the identity pose and PcZ = 1, u = 512 X and v = 512 Y exactly, so
# an ulp of X is an ulp of u
EXACT = Geom(512.0, 512.0, 0.0, 0.0, 32.0, (-640.0, 640.0, -384.0, 384.0))


def camera_center(Tcw):
    T = np.asarray(Tcw, f32).reshape(4, 4)
    Ow = []
    for i in range(3):
        s = f64(0)
        for k in range(3):
            s = s + f64(T[k, i]) * f64(T[k, 3])
        Ow.append(f32(f64(-1.0) * s))
    return Ow


def frustum_one(g, Tcw, Ow, limit, P, Pn, min_dist, max_dist):
    """(why, u, v, xr, level, viewCos): why = IN_VIEW with the five tracking fields, or the test that rejected the
    point with zeros"""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    P = [f32(v) for v in P]
    Pn = [f32(v) for v in Pn]
    min_dist, max_dist, limit = f32(min_dist), f32(max_dist), f32(limit)
    out = (f32(0), f32(0), f32(0), 0, f32(0))
    if not (np.isfinite(T[:3]).all() and np.isfinite(P).all() and np.isfinite(Pn).all() and np.isfinite(min_dist)
            and np.isfinite(max_dist)):
        return (EXCLUDED,) + out
    Pc = []
    for i in range(3):
        t0 = f32(f32(T[i, 0] * P[0]) + f32(T[i, 1] * P[1])) + f32(T[i, 2] * P[2])
        Pc.append(f32(f64(t0) + f64(T[i, 3])))
    if not np.isfinite(Pc).all():
        return (EXCLUDED,) + out
    if Pc[2] < f32(0.0):
        return (DEPTH,) + out
    if Pc[2] == f32(0.0):
        return (EXCLUDED,) + out
    invz = f32(1.0) / Pc[2]
    u = f32(f32(g.fx * Pc[0]) * invz) + g.cx
    v = f32(f32(g.fy * Pc[1]) * invz) + g.cy
    if not (np.isfinite(u) and np.isfinite(v)):
        return (EXCLUDED,) + out
    if u < g.min_x or u > g.max_x:
        return (BOUNDS_U,) + out
    if v < g.min_y or v > g.max_y:
        return (BOUNDS_V,) + out
    PO = [f32(P[k] - Ow[k]) for k in range(3)]
    s = f64(0)
    for k in range(3):
        s = s + f64(PO[k]) * f64(PO[k])
    dist = f32(np.sqrt(s))
    if not np.isfinite(dist) or dist == f32(0.0):
        return (EXCLUDED,) + out
    if dist < f32(f32(0.8) * min_dist) or dist > f32(f32(1.2) * max_dist):
        return (DISTANCE,) + out
    d = f64(0)
    for k in range(3):
        d = d + f64(PO[k]) * f64(Pn[k])
    view_cos = f32(d / f64(dist))
    if not np.isfinite(view_cos):
        return (EXCLUDED,) + out
    if view_cos < limit:
        return (VIEW_COS,) + out
    ratio = f32(max_dist / dist)
    if not positive_normal(ratio):
        return (EXCLUDED,) + out
    fl = np.ceil(f32(logf(ratio) / g.log_scale_factor))
    level = 0 if fl < 0 else g.nlevels - 1 if fl >= g.nlevels else int(fl)
    return IN_VIEW, u, v, f32(u - f32(g.bf * invz)), level, view_cos


class Fields:
    """the six arrays of orbx_is_in_frustum for n points, and why each point is or is not in view"""

    def __init__(self, n):
        self.in_view = np.zeros(n, np.uint8)
        self.proj_x, self.proj_y, self.proj_xr, self.view_cos = (np.zeros(n, f32) for _ in range(4))
        self.level = np.zeros(n, np.int32)
        self.why = np.zeros(n, np.int32)

    def same_as(self, in_view, proj_x, proj_y, proj_xr, level, view_cos):
        b = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)  # noqa: E731
        return (np.array_equal(self.in_view, in_view) and np.array_equal(b(self.proj_x), b(proj_x)) and
                np.array_equal(b(self.proj_y), b(proj_y)) and np.array_equal(b(self.proj_xr), b(proj_xr)) and
                np.array_equal(self.level, level) and np.array_equal(b(self.view_cos), b(view_cos)))


def is_in_frustum(g, Tcw, limit, pos, normal, min_dist, max_dist):
    n = len(pos)
    F = Fields(n)
    Ow = camera_center(Tcw)
    with np.errstate(all="ignore"):
        for j in range(n):
            why, u, v, xr, lv, vc = frustum_one(g, Tcw, Ow, limit, pos[j], normal[j], min_dist[j], max_dist[j])
            F.why[j] = why
            if why == IN_VIEW:
                F.in_view[j], F.proj_x[j], F.proj_y[j], F.proj_xr[j], F.level[j], F.view_cos[j] = 1, u, v, xr, lv, vc
    return F


# ------------------------------------------------------------------------------------------------ inputs
def poses(seed=5):
    import unproject_py as UP
    return UP.poses(seed)


def cloud(g, Tcw, n, seed):
    """n MapPoints around the frustum of (g, Tcw): back-projected pixels of a region a quarter larger than the image
    at depths -2..14, normals towards the camera (a tenth away from it), distance bounds around the true distance (a
    tenth out of range): (pos [n, 3], normal [n, 3], min_dist [n], max_dist [n]) float32"""
    rng = np.random.default_rng(seed)
    w, h = float(g.max_x - g.min_x), float(g.max_y - g.min_y)
    u = rng.uniform(float(g.min_x) - w / 8, float(g.max_x) + w / 8, n)
    v = rng.uniform(float(g.min_y) - h / 8, float(g.max_y) + h / 8, n)
    z = rng.uniform(-2.0, 14.0, n)
    xc = np.stack([(u - float(g.cx)) / float(g.fx) * z, (v - float(g.cy)) / float(g.fy) * z, z], 1)
    T = np.asarray(Tcw, f64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    pos = (xc - t) @ R
    Ow = -(R.T @ t)
    po = pos - Ow
    dist = np.linalg.norm(po, axis=1)
    nrm = po / dist[:, None] + rng.normal(0, 0.5, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[rng.random(n) < 0.1] *= -1
    maxd = dist * 1.2 ** rng.uniform(-1.5, 9.5, n)
    mind = maxd / 1.2 ** 7
    far = rng.random(n) < 0.05
    maxd[far] = dist[far] * 0.5
    near = rng.random(n) < 0.05
    mind[near] = dist[near] * 2.0
    return pos.astype(f32), nrm.astype(f32), mind.astype(f32), maxd.astype(f32)


def scale_ratios():
    """the floats 1.2f^k, k = -2..9: PredictScale's level steps and both clamps"""
    r = {0: f32(1.0)}
    for k in range(1, 10):
        r[k] = f32(r[k - 1] * f32(1.2))
    for k in (-1, -2):
        r[k] = f32(r[k + 1] / f32(1.2))
    return [r[k] for k in range(-2, 10)]


def factor_for(c, target):
    """a float m with (float)(c * m) == target, c a float constant (0.8f, 1.2f); None if the products skip target"""
    c, target = f32(c), f32(target)
    m = f32(target / c)
    lo = m
    for _ in range(6):
        lo = down(lo)
    for _ in range(13):
        if f32(c * lo) == target:
            return lo
        lo = up(lo)
    return None


IDENTITY = np.eye(4, dtype=f32)
ZERO_ROT = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1]], f32)  # Pc = (0, 0, 1), mOw = 0
NZ = (0.0, 0.0, 1.0)


def directed_rows():
    """rows at a boundary of every test and one ulp either side of it, under the EXACT geometry, limit 0.5:
    [(label, Tcw, P, Pn, min_dist, max_dist, why)] with why the expected outcome, or None where the restatement alone
    decides. Under the identity pose Pc = PO = P."""
    rows = []

    def add(label, P, Pn=NZ, mind=0.01, maxd=100.0, why=None, T=IDENTITY):
        rows.append((label, T, tuple(f32(v) for v in P), tuple(f32(v) for v in Pn), f32(mind), f32(maxd), why))
    tiny = np.finfo(f32).tiny
    den = np.array(1, np.uint32).view(f32)[()]
    # PcZ around 0
    add("z=-denormal", (0, 0, -den), why=DEPTH)
    add("z=-1", (0, 0, -1.0), why=DEPTH)
    add("z=-0", (0, 0, -0.0), why=EXCLUDED)
    add("z=+0", (0, 0, 0.0), why=EXCLUDED)
    add("z=+denormal", (den, 0, den), why=EXCLUDED)  # invz = inf
    add("z=FLT_MIN", (0, 0, tiny), mind=0.0, maxd=tiny, why=IN_VIEW)
    # u and v at the image bounds: u = 512 X, v = 512 Y at Z = 1
    for lab, axis, edge in (("u=min_x", 0, -1.25), ("u=max_x", 0, 1.25), ("v=min_y", 1, -0.75), ("v=max_y", 1, 0.75)):
        outer, inner = (down, up) if edge < 0 else (up, down)
        for tag, val, why in (("", f32(edge), IN_VIEW), ("+out", outer(edge), BOUNDS_U + axis),
                              ("+in", inner(edge), IN_VIEW)):
            P = [0.0, 0.0, 1.0]
            P[axis] = val
            add(lab + tag, P, why=why)
    # dist = 3 exactly at (2, 1, 2): 0.8f * min_dist at dist and one ulp either side
    for tag, target, why in (("", f32(3.0), IN_VIEW), ("+1ulp", up(3.0), DISTANCE), ("-1ulp", down(3.0), IN_VIEW)):
        add("dist=0.8min" + tag, (2, 1, 2), mind=factor_for(0.8, target), why=why)
    # dist = 1.125 exactly at (0.75, 0.375, 0.75): 1.2f * max_dist likewise (max_dist in the binade below dist's)
    for tag, target, why in (("", f32(1.125), IN_VIEW), ("+1ulp", up(1.125), IN_VIEW), ("-1ulp", down(1.125), DISTANCE)):
        add("dist=1.2max" + tag, (0.75, 0.375, 0.75), maxd=factor_for(1.2, target), why=why)
    # viewCos = 2 nz / 3 at (2, 1, 2) with Pn = (0, 0, nz): 0.5 at nz = 0.75
    add("cos=limit", (2, 1, 2), Pn=(0, 0, 0.75), why=IN_VIEW)
    add("cos=limit+1ulp", (2, 1, 2), Pn=(0, 0, up(0.75)), why=IN_VIEW)
    add("cos=limit-1ulp", (2, 1, 2), Pn=(0, 0, down(0.75)), why=VIEW_COS)
    # ratio = max_dist / 2 at (0, 0, 2): 1.0f (logf's early return) and the powers of 1.2f
    add("ratio=1", (0, 0, 2), maxd=2.0, why=IN_VIEW)
    add("ratio=1+1ulp", (0, 0, 2), maxd=up(2.0), why=IN_VIEW)
    add("ratio=1-1ulp", (0, 0, 2), maxd=down(2.0), why=IN_VIEW)
    for k, r in zip(range(-2, 10), scale_ratios()):
        for tag, rr in (("", r), ("+1ulp", up(r)), ("-1ulp", down(r))):
            add("ratio=1.2^%d%s" % (k, tag), (0, 0, 2), maxd=f32(f32(2.0) * rr))
    # the contract's exclusions
    for i in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            P, Pn = [0.0, 0.0, 2.0], [0.0, 0.0, 1.0]
            P[i] = bad
            add("pos[%d]=%s" % (i, bad), P, why=EXCLUDED)
            Pn[i] = bad
            add("normal[%d]=%s" % (i, bad), (0, 0, 2), Pn=Pn, why=EXCLUDED)
    for bad in (np.nan, np.inf, -np.inf):
        add("min=%s" % bad, (0, 0, 2), mind=bad, why=EXCLUDED)
        add("max=%s" % bad, (0, 0, 2), maxd=bad, why=EXCLUDED)
    add("Pc overflows", (3e38, 3e38, 3e38), why=EXCLUDED, T=np.array(
        [[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32))
    add("dist=0", (0, 0, 0), why=EXCLUDED, T=ZERO_ROT)
    add("ratio=inf", (0, 0, 0.5), mind=0.0, maxd=3e38, why=EXCLUDED)
    for k in (0, 3, 11):
        T = IDENTITY.copy()
        T.reshape(16)[k] = np.nan
        add("pose[%d]=nan" % k, (0, 0, 2), why=EXCLUDED, T=T)
    return rows


FIXTURE = "frustum_vectors.txt"  # under tests/golden/


def fixture_text(n=40):
    """the vectors tests/cpp/test_frustum.c reads, every float as the hex of its bits: per camera and pose a line
    `case <name> <fx fy cx cy bf min_x min_y max_x max_y> <nlevels> <log_scale_factor> <limit>`, a line
    `pose <16 words>`, a line `points <n>` and n lines `<pos 3> <normal 3> <min> <max> <in_view> <x y xr> <level>
    <view_cos>`."""
    import undistort_py as U

    def hx(v):
        return "%08x" % int(np.array(v, f32).view(np.uint32))
    lines = []
    for ci, name in enumerate(U.CAMERAS):
        g = camera_geom(name)
        for pi, T in enumerate(poses()):
            pos, nrm, mind, maxd = cloud(g, T, n, 100 * ci + pi)
            F = is_in_frustum(g, T, 0.5, pos, nrm, mind, maxd)
            lines.append("case %s %s %d %s %s" % (
                name, " ".join(hx(v) for v in (g.fx, g.fy, g.cx, g.cy, g.bf, g.min_x, g.min_y, g.max_x, g.max_y)),
                g.nlevels, hx(g.log_scale_factor), hx(0.5)))
            lines.append("pose %s" % " ".join(hx(v) for v in np.asarray(T, f32).reshape(16)))
            lines.append("points %d" % n)
            for j in range(n):
                lines.append("%s %s %s %s %d %s %s %s %d %s" % (
                    " ".join(hx(v) for v in pos[j]), " ".join(hx(v) for v in nrm[j]), hx(mind[j]), hx(maxd[j]),
                    F.in_view[j], hx(F.proj_x[j]), hx(F.proj_y[j]), hx(F.proj_xr[j]), F.level[j], hx(F.view_cos[j])))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (os.path.join(root, "cooperative-orb-slam_amd"), os.path.join(root, "oracle"), here):
        sys.path.insert(0, p)
    with open(os.path.join(here, "golden", FIXTURE), "w") as f:
        f.write(fixture_text())

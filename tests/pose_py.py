"""Optimizer::PoseOptimization (Optimizer.cc:239-451) restated in pure Python, the yardstick of csrc/pose_optimize.c and
k_pose_optimize: the sequence include/orbslam_amd.h states ("Pose optimisation"), one scalar operation at a time on
Python floats (IEEE doubles, no contraction, no vectorised sums) with numpy.float32 for the float casts. Also the scene
builder of the pose tests, deterministic from a seed."""
import math
import struct

import numpy as np

import undistort_py as U

OK, TOO_FEW, EXCLUDED = 0, 1, 2
DBL_MAX = float.fromhex("0x1.fffffffffffffp+1023")


def f32(v):
    return float(np.float32(v))


def isfin(v):
    return (struct.unpack("<Q", struct.pack("<d", v))[0] & 0x7ff0000000000000) != 0x7ff0000000000000


# ---- so3_sincos: the constants are derived here as tools/gen_so3_sincos.py derives them, not copied ----
def _constants():
    from fractions import Fraction
    bits = 256

    def atan_inv(n):
        one = 1 << (bits + 32)
        term, total, k, sign = one // n, 0, 1, 1
        while term:
            total += sign * (term // k)
            term //= n * n
            k += 2
            sign = -sign
        return total >> 32
    pi = Fraction(4 * (4 * atan_inv(5) - atan_inv(239)), 1 << bits)
    hpi = pi / 2
    head = Fraction(int(hpi * (1 << 32)), 1 << 32)
    mid = Fraction(int((hpi - head) * (1 << 66)), 1 << 66)
    S =[float(Fraction((-1) ** i, math.factorial(2 * i + 1))) for i in range(1, 9)]
    Cc = [float(Fraction((-1) ** i, math.factorial(2 * i))) for i in range(1, 9)]
    return float(head), float(mid), float(hpi - head - mid), float(2 / pi), S, Cc


PIO2_1, PIO2_2, PIO2_3, INV_PIO2, S_COEF, C_COEF = _constants()


def so3_sincos(th):
    if not th < 1048576.0:
        return 0.0, 1.0
    k = int(th * INV_PIO2 + 0.5)
    kd = float(k)
    r = ((th - kd * PIO2_1) - kd * PIO2_2) - kd * PIO2_3
    z = r * r
    ps = z * S_COEF[7]
    for c in S_COEF[6::-1]:
        ps = z * (c + ps)
    sn = r + r * ps
    pc = z * C_COEF[7]
    for c in C_COEF[6::-1]:
        pc = z * (c + pc)
    cs = 1.0 + pc
    q = k & 3
    return ((sn, cs), (cs, -sn), (-sn, -cs), (-cs, sn))[q]


# ---- SE3 ----
def quat_normalize(q, flags=None):
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [q[0] / n, q[1] / n, q[2] / n, q[3] / n]
    if q[3] < 0.0:
        if flags is not None:
            flags["wneg"] = flags.get("wneg", 0) + 1
        q = [-q[0], -q[1], -q[2], -q[3]]
    return q


def quat_from_R(R, flags=None):
    """R: 3x3 nested list; Eigen's rule, then normalizeRotation"""
    tr = (R[0][0] + R[1][1]) + R[2][2]
    q = [0.0] * 4
    if tr > 0.0:
        s = math.sqrt(tr + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0] = (R[2][1] - R[1][2]) * s
        q[1] = (R[0][2] - R[2][0]) * s
        q[2] = (R[1][0] - R[0][1]) * s
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        if flags is not None:
            flags["branch%d" % i] = flags.get("branch%d" % i, 0) + 1
        s = math.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (R[k][j] - R[j][k]) * s
        q[j] = (R[j][i] + R[i][j]) * s
        q[k] = (R[k][i] + R[i][k]) * s
    return quat_normalize(q, flags)


def se3_from_Tcw(T, flags=None):
    T = np.asarray(T, np.float32).reshape(4, 4)
    R = [[float(T[r, c]) for c in range(3)] for r in range(3)]
    return quat_from_R(R, flags) + [float(T[r, 3]) for r in range(3)]


def quat_rot(q, X):
    u0 = q[1] * X[2] - q[2] * X[1]
    u1 = q[2] * X[0] - q[0] * X[2]
    u2 = q[0] * X[1] - q[1] * X[0]
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    return [(X[0] + q[3] * u0) + (q[1] * u2 - q[2] * u1),
            (X[1] + q[3] * u1) + (q[2] * u0 - q[0] * u2),
            (X[2] + q[3] * u2) + (q[0] * u1 - q[1] * u0)]


def se3_map(s, X):
    o = quat_rot(s, X)
    return [o[0] + s[4], o[1] + s[5], o[2] + s[6]]


def se3_to_Tcw(s):
    x, y, z, w = s[:4]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    T = np.zeros((4, 4), np.float32)
    T[0] = [1.0 - (tyy + tzz), txy - twz, txz + twy, s[4]]
    T[1] = [txy + twz, 1.0 - (txx + tzz), tyz - twx, s[5]]
    T[2] = [txz - twy, tyz + twx, 1.0 - (txx + tyy), s[6]]
    T[3, 3] = 1.0
    return T


def se3_exp_mul(d, s, flags=None):
    """returns (new state, 1 if the small-angle branch was taken)"""
    w0, w1, w2 = d[0], d[1], d[2]
    th = math.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    Om = [[0.0, -w2, w1], [w2, 0.0, -w0], [-w1, w0, 0.0]]
    O2 = [[(Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c] for c in range(3)] for r in range(3)]
    eye = lambda r, c: 1.0 if r == c else 0.0  # noqa: E731
    small = 0
    if th < 0.00001:
        small = 1
        R = [[(eye(r, c) + Om[r][c]) + O2[r][c] for c in range(3)] for r in range(3)]
        V = R
    else:
        sn, cs = so3_sincos(th)
        th2 = th * th
        a, b, c3 = sn / th, (1.0 - cs) / th2, (th - sn) / (th2 * th)
        R = [[(eye(r, c) + a * Om[r][c]) + b * O2[r][c] for c in range(3)] for r in range(3)]
        V = [[(eye(r, c) + b * Om[r][c]) + c3 * O2[r][c] for c in range(3)] for r in range(3)]
    qd = quat_from_R(R, flags)
    td = [(V[r][0] * d[3] + V[r][1] * d[4]) + V[r][2] * d[5] for r in range(3)]
    rt = quat_rot(qd, s[4:7])
    ax, ay, az, aw = qd
    bx, by, bz, bw = s[:4]
    qn = [((aw * bx + ax * bw) + ay * bz) - az * by,
          ((aw * by + ay * bw) + az * bx) - ax * bz,
          ((aw * bz + az * bw) + ax * by) - ay * bx,
          ((aw * bw - ax * bx) - ay * by) - az * bz]
    qn = quat_normalize(qn, flags)
    return qn + [td[0] + rt[0], td[1] + rt[1], td[2] + rt[2]], small


def ldlt6_solve(A, b):
    """A: 6x6 nested list (lower triangle read); returns (ok, x)"""
    L = [[0.0] * 6 for _ in range(6)]
    dg = [0.0] * 6
    ok = True
    for j in range(6):
        dj = A[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * dg[k]) * L[j][k]
        if not dj > 0.0:
            ok = False
        dg[j] = dj
        for i in range(j + 1, 6):
            sv = A[i][j]
            for k in range(j):
                sv = sv - (L[i][k] * dg[k]) * L[j][k]
            try:
                L[i][j] = sv / dj
            except ZeroDivisionError:
                L[i][j] = math.nan
    if not ok:
        return False, [0.0] * 6
    y = [0.0] * 6
    for i in range(6):
        v = b[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i] / dg[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v
    return True, x


def _div(a, b):
    """IEEE division for the cases Python raises on"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def edge_eval(cam, s, Xw, obs, stereo, w, delta, full):
    """returns (chi2, terms or None): terms = 21 H, 6 b, rho0 (full) or [rho0] (errors only); delta None = chi2 only"""
    fx, fy, cx, cy, bf = cam
    X, Y, Z = se3_map(s, Xw)
    invz = _div(1.0, Z)
    u = (X * invz) * fx + cx
    v = (Y * invz) * fy + cy
    e0, e1 = obs[0] - u, obs[1] - v
    e2 = obs[2] - (u - bf * invz) if stereo else 0.0
    we0, we1, we2 = w * e0, w * e1, w * e2
    chi2 = e0 * we0 + e1 * we1
    if stereo:
        chi2 = chi2 + e2 * we2
    if delta is None:
        return chi2, None
    rho0, rho1 = chi2, 1.0
    if delta > 0.0:
        d2 = delta * delta
        if not chi2 <= d2:
            sq = math.sqrt(chi2) if chi2 == chi2 and chi2 >= 0 else math.nan
            rho0 = (2.0 * sq) * delta - d2
            rho1 = _div(delta, sq)
    if not full:
        return chi2, [rho0]
    iz2 = invz * invz
    XY = X * Y
    J = [[(XY * iz2) * fx, (-(1.0 + (X * X) * iz2)) * fx, (Y * invz) * fx, (-invz) * fx, 0.0, (X * iz2) * fx],
         [(1.0 + (Y * Y) * iz2) * fy, ((-XY) * iz2) * fy, ((-X) * invz) * fy, 0.0, (-invz) * fy, (Y * iz2) * fy]]
    if stereo:
        J.append([J[0][0] - (bf * Y) * iz2, J[0][1] + (bf * X) * iz2, J[0][2], J[0][3], 0.0, J[0][5] - bf * iz2])
    wgt = rho1 * w
    r = [(-we0) * rho1, (-we1) * rho1, (-we2) * rho1]
    terms = []
    for a in range(6):
        for b in range(a, 6):
            h = J[0][a] * (wgt * J[0][b]) + J[1][a] * (wgt * J[1][b])
            if stereo:
                h = h + J[2][a] * (wgt * J[2][b])
            terms.append(h)
    for a in range(6):
        g = J[0][a] * r[0] + J[1][a] * r[1]
        if stereo:
            g = g + J[2][a] * r[2]
        terms.append(g)
    terms.append(rho0)
    return chi2, terms


TH_MONO, TH_STEREO = np.float32(5.991), np.float32(7.815)  # const float chi2Mono[4], chi2Stereo[4]


def edge_outlier(chi2, stereo):
    """Optimizer.cc:393-395, :422-424: the double chi2 cast to float, strictly above the float constant"""
    with np.errstate(over="ignore"):
        return int(np.float32(chi2) > (TH_STEREO if stereo else TH_MONO))


DIAG_IDX = (0, 6, 11, 15, 18, 20)


def pose_optimization(cam, inv_level_sigma2, Tcw, kps, uright, mp_index, pos, outlier=None, flags=None):
    """cam = (fx, fy, cx, cy, bf) floats (float32 values); kps: structured orbx_kp array; returns (Tcw float32 4x4,
    outlier uint8 [n], ninliers, status, diag int32 [8])"""
    cam = tuple(f32(v) for v in cam)
    n = len(kps)
    nlevels = len(inv_level_sigma2)
    Tcw = np.array(Tcw, np.float32).reshape(4, 4)
    outlier = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8)
    diag = np.zeros(8, np.int32)
    dm, ds = f32(math.sqrt(5.991)), f32(math.sqrt(7.815))
    st = OK
    if not np.isfinite(Tcw[:3]).all():
        st = EXCLUDED
    edges = []  # (i, Xw, obs, stereo, w)
    for i in range(n):
        if mp_index[i] < 0:
            continue
        X = pos[mp_index[i]]
        ur = -1.0 if uright is None else float(uright[i])
        o = int(kps["octave"][i])
        x, y = float(kps["x"][i]), float(kps["y"][i])
        if not 0 <= o < nlevels or not all(isfin(v) for v in (x, y, ur, float(X[0]), float(X[1]), float(X[2]))):
            st = EXCLUDED
            edges.append(None)
            continue
        stereo = not ur < 0
        edges.append((i, [float(X[0]), float(X[1]), float(X[2])], (x, y, ur), stereo, float(inv_level_sigma2[o])))
    ninit = len(edges)
    if st == OK and ninit < 3:
        st = TOO_FEW
    lvl = [0] * ninit
    robust = True
    nbad = 0
    est = None
    rejected = fails = small = 0

    def evaluate(s, full):
        sums = [0.0] * (28 if full else 1)
        for e, l in zip(edges, lvl):
            if l:
                continue
            _, t = edge_eval(cam, s, e[1], e[2], e[3], e[4], (ds if e[3] else dm) if robust else 0.0, full)
            for k in range(len(sums)):
                sums[k] = sums[k] + t[k]
        return sums

    for it in range(4):
        if st != OK:
            break
        est = se3_from_Tcw(Tcw, flags)
        errst = est
        nact = ninit - sum(lvl)
        for itr in range(10):
            if nact == 0:
                break
            sums = evaluate(est, True)
            errst = est
            if itr == 0 and not isfin(sums[27]):
                st = EXCLUDED
                break
            cur = sums[27]
            if itr == 0:
                md = 0.0
                for a in DIAG_IDX:
                    if abs(sums[a]) > md:
                        md = abs(sums[a])
                lam, nu = 1e-5 * md, 2.0
            rho, q = 0.0, 0
            while True:
                A = [[0.0] * 6 for _ in range(6)]
                t = 0
                for a in range(6):
                    for c in range(a, 6):
                        h = sums[t] + lam if a == c else sums[t]
                        A[a][c] = A[c][a] = h
                        t += 1
                b = sums[21:27]
                ok, x = ldlt6_solve(A, b)
                if not ok:
                    fails += 1
                saved = est
                est, sm = se3_exp_mul(x, est, flags)
                small += sm
                tmp = evaluate(est, False)[0]
                errst = est
                if not ok:
                    tmp = DBL_MAX
                scale = 0.0
                for a in range(6):
                    scale = scale + x[a] * (lam * x[a] + b[a])
                scale = scale + 1e-3
                rho = _div(cur - tmp, scale)
                if rho > 0.0 and isfin(tmp):
                    tt = 2.0 * rho - 1.0
                    alpha = 1.0 - (tt * tt) * tt
                    if 2.0 / 3.0 < alpha:
                        alpha = 2.0 / 3.0
                    lam = lam * (alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0)
                    nu = 2.0
                    cur = tmp
                else:
                    lam = lam * nu
                    nu = nu * 2.0
                    est = saved
                    rejected += 1
                q += 1
                if not (rho < 0.0 and q < 10):
                    break
            diag[1 + it] += 1
            if q == 10 or rho == 0.0:
                if flags is not None and q == 10:
                    flags["ten_rejections"] = flags.get("ten_rejections", 0) + 1
                break
        if st != OK:
            break
        diag[0] += 1
        nbad = 0
        for k, e in enumerate(edges):
            chi2, _ = edge_eval(cam, est if lvl[k] else errst, e[1], e[2], e[3], e[4], None, False)
            was = lvl[k]
            lvl[k] = edge_outlier(chi2, e[3])
            if flags is not None and was and not lvl[k]:
                flags["returned"] = flags.get("returned", 0) + 1
            nbad += lvl[k]
        if it == 2:
            robust = False
        if ninit < 10:
            break
    out = Tcw
    ninl = 0
    if st == OK:
        out = se3_to_Tcw(est)
        ninl = ninit - nbad
    if st != EXCLUDED:
        for k, e in enumerate(edges):
            outlier[e[0]] = lvl[k] if st == OK else 0
    diag[5], diag[6], diag[7] = rejected, fails, small
    return out, outlier, ninl, st, diag


# ---- scenes ----
BF = {"my": 40.0, "tum1": 40.0, "euroc": 47.90639384423901}
NLEVELS = 8


def inv_level_sigma2(nlevels=NLEVELS, scale=1.2):
    """mvInvLevelSigma2 as ORBextractor builds it: float products"""
    sf = [np.float32(1.0)]
    for _ in range(1, nlevels):
        sf.append(np.float32(sf[-1] * np.float32(scale)))
    return np.array([np.float32(1.0) / np.float32(s * s) for s in sf], np.float32)


def rot(axis, ang):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


def pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


class Scene:
    """one PoseOptimization call: cam (fx, fy, cx, cy, bf), inv (mvInvLevelSigma2), T0 (the initial mTcw), kps, uright
    (or None), mp_index, pos; T_true, planted (bool [n]) for the independent check"""

    def run_py(self, flags=None, outlier=None):
        return pose_optimization(self.cam, self.inv, self.T0, self.kps, self.uright, self.mp_index, self.pos,
                                 outlier=outlier, flags=flags)


def make_scene(camera="my", n=120, kind="stereo", noise=0.0, outliers=0.1, seed=1, stride=None, T_true=None,
               perturb=(0.03, math.radians(1.0)), unmatched=0.15, name=None):
    """n matched MapPoints at depths 1..20 m seen from T_true, an initial pose a few cm and about a degree off,
    `outliers` of them displaced by 20..60 px, octaves spread over the levels, `unmatched` extra features without a
    MapPoint interleaved; the position table holds the points in a shuffled order plus unused rows"""
    from orbamd import kp_dtype
    rng = np.random.default_rng(seed)
    cam, W, H = U.CAMERAS[camera]
    bf = BF[camera]
    s = Scene()
    s.name = name or "%s/%s/n%d/noise%g" % (camera, kind, n, noise)
    s.cam = (f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy), f32(bf))
    s.inv = inv_level_sigma2()
    if T_true is None:
        T_true = pose(rot(rng.normal(size=3), 0.3 * rng.random()), rng.normal(size=3) * 0.5)
    s.T_true = np.asarray(T_true, np.float64)
    dR = rot(rng.normal(size=3), perturb[1])
    dt = rng.normal(size=3)
    dt = dt / np.linalg.norm(dt) * perturb[0]
    s.T0 = (pose(dR, dt) @ s.T_true).astype(np.float32)
    ntot = n + int(round(n * unmatched))
    if stride is not None:
        ntot = min(ntot, stride)
    has = np.zeros(ntot, bool)
    has[rng.permutation(ntot)[:n]] = True
    u = rng.uniform(20, W - 20, ntot)
    v = rng.uniform(20, H - 20, ntot)
    z = rng.uniform(1.0, 20.0, ntot)
    Pc = np.stack([(u - cam.fx * 0 - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z], 1)
    Rt, tt = s.T_true[:3, :3], s.T_true[:3, 3]
    Pw = ((Pc - tt) @ Rt).astype(np.float32)  # R^T (Pc - t)
    # observations from the float32 positions, so the noise-free residual at T_true is rounding only
    Pc2 = Pw.astype(np.float64) @ Rt.T + tt
    s_cam = [float(c) for c in s.cam]
    u = Pc2[:, 0] / Pc2[:, 2] * s_cam[0] + s_cam[2]
    v = Pc2[:, 1] / Pc2[:, 2] * s_cam[1] + s_cam[3]
    ur = u - s_cam[4] / Pc2[:, 2]
    octave = rng.integers(0, NLEVELS, ntot)
    sig = np.array([1.2 ** o for o in octave])
    if noise:
        u = u + rng.normal(size=ntot) * noise * sig
        v = v + rng.normal(size=ntot) * noise * sig
        ur = ur + rng.normal(size=ntot) * noise * sig
    planted = np.zeros(ntot, bool)
    idx = np.flatnonzero(has)
    bad = idx[rng.permutation(len(idx))[:int(round(len(idx) * outliers))]]
    planted[bad] = True
    ang = rng.uniform(0, 2 * math.pi, len(bad))
    mag = rng.uniform(20, 60, len(bad)) * sig[bad]
    u[bad] += np.cos(ang) * mag
    v[bad] += np.sin(ang) * mag
    ur[bad] += np.cos(ang) * mag
    s.planted = planted
    s.kps = np.zeros(ntot, kp_dtype)
    s.kps["x"], s.kps["y"], s.kps["octave"] = u.astype(np.float32), v.astype(np.float32), octave
    s.kps["size"], s.kps["angle"], s.kps["response"] = 31.0, 10.0, 50.0
    if kind == "mono":
        s.uright = None
    else:
        s.uright = ur.astype(np.float32)
        if kind == "mixed":
            s.uright[rng.random(ntot) < 0.5] = -1.0
        s.uright[(s.uright < 0) & (s.uright > -1)] = -1.0
    M = ntot + 7
    rows = rng.permutation(M)[:ntot]
    s.pos = rng.normal(size=(M, 3)).astype(np.float32)
    s.pos[rows] = Pw
    s.mp_index = np.where(has, rows, -1).astype(np.int32)
    s.n = ntot
    return s


def threshold_scene():
    """chi2 exactly at the float threshold, and one float above and below it, through the whole function. With fx =
    fy = bf = 0 every projection is (cx, cy, cx) whatever the pose, so an edge's chi2 = invSigma2 ((x - cx)^2 +
    (y - cy)^2 [+ (uright - cx)^2]) is set by its observation alone, J = 0, H = 0, lambda = 0 and every solve fails:
    one round of ten rejections (N = 8 < 10), then the classification. Per kind four edges, (x, y) searched among
    neighbouring floats so that, with th = (float)5.991 or (float)7.815:
      at+    (float)chi2 == th with the double chi2 above (double)th   -> inlier (a double comparison would flag it)
      at-    (float)chi2 == th with the double chi2 below (double)th   -> inlier
      above  (float)chi2 == nextafter(th, +inf)                        -> outlier
      below  (float)chi2 == nextafter(th, -inf)                        -> inlier
    Returns (scene, want flags [8], the eight (name, chi2, its float target))."""
    from orbamd import kp_dtype
    s = Scene()
    s.name = "threshold"
    cx = cy = 0.0  # observations of a few pixels, so that a float step of x or y moves chi2 by about a float ulp
    s.cam = (0.0, 0.0, cx, cy, 0.0)
    s.inv = inv_level_sigma2()
    s.T0 = pose(rot([0.2, 1.0, -0.3], 0.1), [0.1, -0.2, 0.3]).astype(np.float32)
    s.T_true = s.T0.astype(np.float64)
    w = float(s.inv[0])
    assert w == 1.0
    rows, want, info = [], [], []
    for stereo, th in ((False, TH_MONO), (True, TH_STEREO)):
        dr = 1.25  # uright - cx, exact
        up, dn = np.nextafter(th, np.float32(np.inf)), np.nextafter(th, np.float32(-np.inf))
        for name, tgt, cond, flag in (("at+", th, lambda c, t: c > float(t), 0),
                                      ("at-", th, lambda c, t: c < float(t), 0),
                                      ("above", up, lambda c, t: c == c, 1), ("below", dn, lambda c, t: c == c, 0)):
            # a grid of neighbouring floats (x, y) around a point of the circle; the search is vectorised, the hit is
            # recomputed in scalars below
            r2 = float(tgt) - (dr * dr if stereo else 0.0)
            x0, y0 = np.float32(math.sqrt(r2 * 0.6)), np.float32(math.sqrt(r2 * 0.4))
            k = np.arange(-300, 301)
            xs = (x0.view(np.int32) + k).astype(np.int32).view(np.float32).astype(np.float64)[:, None]
            ys = (y0.view(np.int32) + k).astype(np.int32).view(np.float32).astype(np.float64)[None, :]
            c = xs * (w * xs) + ys * (w * ys)
            if stereo:
                c = c + dr * (w * dr)
            hit = np.argwhere((c.astype(np.float32) == tgt) & cond(c, tgt))
            assert len(hit), (stereo, name)
            x, y = np.float32(xs[hit[0][0], 0]), np.float32(ys[0, hit[0][1]])
            e0, e1 = float(x) - cx, float(y) - cy
            chi2 = e0 * (w * e0) + e1 * (w * e1)
            if stereo:
                chi2 = chi2 + dr * (w * dr)
            assert np.float32(chi2) == tgt and cond(chi2, tgt)
            rows.append((x, y, np.float32(cx + dr) if stereo else np.float32(-1.0)))
            want.append(flag)
            info.append((("stereo " if stereo else "mono ") + name, chi2, tgt))
    n = len(rows)
    s.kps = np.zeros(n, kp_dtype)
    s.kps["x"], s.kps["y"] = [r[0] for r in rows], [r[1] for r in rows]
    s.uright = np.array([r[2] for r in rows], np.float32)
    s.pos = np.array([[0.3 * i - 1.0, 0.2 * i - 0.5, 4.0 + i] for i in range(n)], np.float32)
    s.mp_index = np.arange(n, dtype=np.int32)
    s.planted = np.array(want, bool)
    s.n = n
    return s, np.array(want, np.uint8), info


def camera_scenes(camera, n=100):
    """{all stereo, all mono, mixed} x {noise-free, 0.5 px noise}"""
    return [make_scene(camera, n, kind, noise, seed=7 + 3 * k)
            for k, (kind, noise) in enumerate((kd, ns) for kd in ("stereo", "mono", "mixed") for ns in (0.0, 0.5))]


SIZES = (0, 1, 2, 3, 9, 10, 11, 63, 64, 65, 255, 256, 257)


def size_scene(n, seed=100, **kw):
    return make_scene("my", n, "mixed", 0.3, seed=seed + n, unmatched=0.0 if n in (0,) else 0.1, **kw)


# ---- golden vectors (tests/golden/pose_vectors.txt): recorded results of this yardstick ----
FIXTURE = "pose_vectors.txt"


def fixture_scenes():
    return [make_scene("my", 24, "mixed", 0.5, seed=41), make_scene("tum1", 12, "stereo", 0.0, seed=42),
            make_scene("euroc", 9, "mono", 0.5, seed=43), make_scene("my", 2, "stereo", 0.0, seed=44),
            make_scene("euroc", 30, "mixed", 0.5, seed=45, perturb=(0.4, math.radians(12.0))), threshold_scene()[0]]


def hexf(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]


def fixture_text():
    """per scene a header `scene n M nlevels`, the camera, inv sigma2, T0, then n feature rows (x y octave uright
    mp_index, floats as hex bits), M position rows, and the recorded result (Tcw, outlier, ninliers and status, diag)"""
    scenes = fixture_scenes()
    L = ["%d" % len(scenes)]
    for s in scenes:
        T, out, ninl, st, dg = s.run_py()
        L.append("scene %d %d %d" % (s.n, len(s.pos), len(s.inv)))
        L.append(" ".join(hexf(v) for v in s.cam))
        L.append(" ".join(hexf(v) for v in s.inv))
        L.append(" ".join(hexf(v) for v in s.T0.reshape(16)))
        for i in range(s.n):
            ur = -1.0 if s.uright is None else s.uright[i]
            L.append("%s %s %d %s %d" % (hexf(s.kps["x"][i]), hexf(s.kps["y"][i]), s.kps["octave"][i], hexf(ur),
                                         s.mp_index[i]))
        for p in s.pos:
            L.append(" ".join(hexf(v) for v in p))
        L.append(" ".join(hexf(v) for v in T.reshape(16)))
        L.append(" ".join(str(int(v)) for v in out) if len(out) else "-")
        L.append("%d %d" % (ninl, st))
        L.append(" ".join(str(int(v)) for v in dg))
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", FIXTURE), "w") as fh:
        fh.write(fixture_text())

"""Optimizer::PoseOptimization on the host (csrc/pose_optimize.c through orbamd.frame.pose_optimization) against the
pure-Python restatement tests/pose_py.py as raw bits -- pose, outlier bytes, ninliers, status, diag -- on the three
reference cameras' scenes, on every size around the kernel's lane and chunk boundaries, and on directed cases each
asserted to be reached (through diag, the yardstick's flags or a direct helper call); the independent check of the
algorithm itself (planted outliers found, the true pose recovered); so3_sincos and ldlt6_solve through their test
hooks; argument errors and malformed input. No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import orbamd
import pose_py as P
import undistort_py as U
from orbamd.frame import pose_optimization, track_geom

CAMS = sorted(U.CAMERAS)
E = -1  # ORBX_EARG
# the independent check's bound on |Tcw - T_true| (max over the 12 entries) on the noise-free scenes: 4 x the largest
# deviation the yardstick shows on them (5.47e-08, float32 output rounding of entries up to ~1); DESIGN.md 5.7
POSE_BOUND = 4 * 5.47e-08
# ldlt6_solve against numpy.linalg.solve on random SPD 6x6 (condition <= 1e4): 4 x the largest relative error seen
LDLT_BOUND = 4 * 2.04e-13


def geom_of(s, nlevels=P.NLEVELS):
    return track_geom(s.cam[0], s.cam[1], s.cam[2], s.cam[3], s.cam[4], 0.08, (0, 640, 0, 480), 0.1, 0.1,
                      [1.2 ** i for i in range(nlevels)])


def host(s, outlier=None):
    return pose_optimization(geom_of(s, len(s.inv)), s.inv, s.T0, s.kps, s.uright, s.mp_index, s.pos, outlier=outlier)


def same(ref, got):
    T, out, ninl, st, dg = ref
    return (T.tobytes() == got.Tcw.tobytes() and np.array_equal(out, got.outlier) and ninl == got.ninliers and
            st == got.status and np.array_equal(dg, got.diag))


@pytest.fixture(scope="module")
def restated():
    """per camera: [(scene, the yardstick's result, its flags)], computed once"""
    out = {}
    for name in CAMS:
        runs = []
        for s in P.camera_scenes(name):
            fl = {}
            runs.append((s, s.run_py(fl), fl))
        out[name] = runs
    return out


@pytest.mark.parametrize("name", CAMS)
def test_host_equals_restatement_bitwise(restated, name):
    runs = restated[name]
    assert len(runs) == 6  # {stereo, mono, mixed} x {noise-free, 0.5 px}
    for s, ref, _ in runs:
        assert same(ref, host(s)), s.name
        assert ref[3] == P.OK and ref[4][0] == 4


@pytest.mark.parametrize("name", CAMS)
def test_planted_outliers_and_true_pose(restated, name):
    """the gate for the algorithm itself, on the yardstick and on the host unit: on the noise-free scenes every planted
    outlier is flagged and no inlier is, and the pose is the true one within POSE_BOUND"""
    worst = 0.0
    for s, ref, _ in restated[name]:
        if "noise0.5" in s.name:
            continue
        has = s.mp_index >= 0
        for T, out in ((ref[0], ref[1]), (lambda r: (r.Tcw, r.outlier))(host(s))):
            assert np.array_equal(out[has].astype(bool), s.planted[has]), s.name
            dev = np.abs(T.astype(np.float64) - s.T_true).max()
            worst = max(worst, dev)
            assert dev <= POSE_BOUND, (s.name, dev)
        assert ref[2] == has.sum() - s.planted[has].sum()
    print("largest deviation from the true pose: %.3g (bound %.3g)" % (worst, POSE_BOUND))


@pytest.mark.parametrize("n", P.SIZES)
def test_sizes(n):
    s = P.size_scene(n)
    ref = s.run_py()
    got = host(s)
    assert same(ref, got), n
    assert ref[3] == (P.TOO_FEW if n < 3 else P.OK)
    assert ref[4][0] == (0 if n < 3 else 1 if n < 10 else 4)  # N = 9: one round only
    if n < 3:
        assert ref[2] == 0 and ref[0].tobytes() == s.T0.tobytes()


def test_thousand_of_stride_1024():
    s = P.make_scene("euroc", 1000, "mixed", 0.5, seed=5, unmatched=0.024, stride=1024)
    assert s.n == 1024
    assert same(s.run_py(), host(s))


def test_features_without_mappoint_keep_their_byte():
    s = P.make_scene("my", 40, "mixed", 0.5, seed=3, unmatched=0.5)
    inc = np.where(s.mp_index < 0, 0xA5, 0x5A).astype(np.uint8)
    ref = s.run_py(outlier=inc)
    got = host(s, outlier=inc)
    assert same(ref, got)
    assert (got.outlier[s.mp_index < 0] == 0xA5).all() and (got.outlier[s.mp_index >= 0] <= 1).all()


# ------------------------------------------------------------------------------------------------ directed cases
def test_start_at_the_optimum_takes_the_small_angle_branch():
    s = P.make_scene("my", 50, "stereo", 0.0, outliers=0.0, seed=21, perturb=(0.0, 0.0))
    ref = s.run_py()
    assert ref[4][7] > 0 and same(ref, host(s))  # diag[7]: exp calls with theta < 1e-5


def test_far_start_rejects_trials_and_an_outlier_returns():
    s = P.make_scene("my", 60, "mixed", 0.5, seed=13, perturb=(0.3, math.radians(8.0)))
    fl = {}
    ref = s.run_py(fl)
    assert ref[4][5] >= 1 and fl.get("returned", 0) >= 1  # rejected trials; an outlier that is an inlier again later
    assert same(ref, host(s))


def test_round_ending_on_ten_rejections(restated):
    """the stale-error rule: after ten rejected trials the inliers' chi2 is the one computed at the rejected estimate"""
    hit = [(s, ref) for runs in restated.values() for s, ref, fl in runs if fl.get("ten_rejections")]
    assert hit
    for s, ref in hit:
        assert same(ref, host(s))


def test_solver_failure():
    """a non-positive pivot: zero information on every edge gives H = 0 and lambda = 0 (ten failed solves per round).
    Every point on one ray gives a rank-deficient H, but that does not reach the failure: Levenberg adds lambda =
    1e-5 max|H_aa| > 0 to the diagonal before every solve, so the matrix handed to the LDL^T is positive definite
    with pivots of the order of lambda, 1e11 times the rounding of the elimination; asserted below as zero failed
    solves (diag[6]), and the scene is kept for host == yardstick on an ill-conditioned system. The pivot test itself
    is reached by the zero-information scene, by the threshold scene and by the direct calls at the end."""
    s = P.make_scene("my", 12, "stereo", 0.0, seed=8)
    s.inv = np.zeros(8, np.float32)
    ref = s.run_py()
    assert ref[4][6] >= 10 and ref[3] == P.OK
    assert same(ref, host(s))
    r = P.make_scene("my", 12, "mono", 0.0, outliers=0.0, seed=9, unmatched=0.0)
    ray = np.array([0.1, -0.05, 1.0])
    r.pos[r.mp_index] = (np.linspace(2, 9, 12)[:, None] * ray).astype(np.float32)
    r.T0 = np.eye(4, dtype=np.float32)
    r.kps["x"], r.kps["y"] = r.cam[2] + r.cam[0] * 0.1 + 0.5, r.cam[3] - r.cam[1] * 0.05
    ref = r.run_py()
    assert ref[4][6] == 0 and ref[4][5] > 0 and same(ref, host(r))
    lib = orbamd.load()
    A = np.diag([1.0, 2.0, 0.0, 1.0, 1.0, 1.0])
    b, x = np.ones(6), np.full(6, 7.0)
    assert lib.orbx_test_ldlt6_solve(A.ctypes.data, b.ctypes.data, x.ctypes.data) == 0 and not x.any()
    assert P.ldlt6_solve(A.tolist(), b.tolist()) == (False, [0.0] * 6)


def se3_hook(op, T, delta=None):
    lib = orbamd.load()
    T = np.ascontiguousarray(T, np.float32).reshape(16)
    st, out = np.zeros(7), np.zeros(16, np.float32)
    d = None if delta is None else np.ascontiguousarray(delta, np.float64)
    rc = lib.orbx_test_se3(op, T.ctypes.data, None if d is None else d.ctypes.data, st.ctypes.data, out.ctypes.data)
    return rc, st, out.reshape(4, 4)


@pytest.mark.parametrize("axis", range(3))
def test_matrix_to_quaternion_trace_branches(axis):
    """rotations near 180 degrees about x, y, z: the three trace <= 0 branches, reached per the yardstick's flags"""
    ax = np.eye(3)[axis] + 0.01
    for ang in (math.radians(179.0), math.radians(181.0), math.pi):
        T = P.pose(P.rot(ax, ang), [0.1, -0.2, 0.3]).astype(np.float32)
        fl = {}
        ref = P.se3_from_Tcw(T, fl)
        assert fl.get("branch%d" % axis) == 1
        rc, st, out = se3_hook(0, T)
        assert rc == 0 and st.tobytes() == np.array(ref).tobytes()
        assert out.tobytes() == P.se3_to_Tcw(ref).tobytes()
    s = P.make_scene("tum1", 40, "mixed", 0.5, seed=30 + axis,
                     T_true=P.pose(P.rot(ax, math.radians(179.5)), [0, 0, 0.5]))
    fl = {}
    ref = s.run_py(fl)
    assert fl.get("branch%d" % axis, 0) >= 4 and same(ref, host(s))


def test_negative_w_after_the_product():
    """a state just short of 180 degrees times a step that passes it: w < 0 after the Hamilton product, all negated"""
    T = P.pose(P.rot([0, 0, 1], math.radians(179.9)), [0.3, 0.2, 0.1]).astype(np.float32)
    delta = [0.0, 0.0, math.radians(0.5), 0.01, -0.02, 0.03]
    f0, f1 = {}, {}
    s0 = P.se3_from_Tcw(T, f0)
    ref, small = P.se3_exp_mul(delta, s0, f1)
    assert f0.get("wneg", 0) == 0 and f1.get("wneg", 0) == 1 and ref[3] >= 0
    rc, st, out = se3_hook(1, T, delta)
    assert rc == small == 0 and st.tobytes() == np.array(ref).tobytes()
    assert out.tobytes() == P.se3_to_Tcw(ref).tobytes()
    rc, st, _ = se3_hook(1, T, [1e-7, -2e-7, 3e-7, 0.01, 0.0, 0.0])  # the small-angle branch through the hook
    ref, small = P.se3_exp_mul([1e-7, -2e-7, 3e-7, 0.01, 0.0, 0.0], s0)
    assert rc == small == 1 and st.tobytes() == np.array(ref).tobytes()


def test_chi2_exactly_at_the_float_threshold():
    """P.threshold_scene: with a zero focal length chi2 is set by the observation alone, so the eight edges sit
    exactly on (float)5.991 / (float)7.815 (from either side in double), one float above and one float below. Pins
    that the comparison is strict and is made on the float cast against the float constant: both constants lie above
    their double literals, and the `at+` edges' double chi2 lies above both, so `>=`, a comparison in double, or one
    against the double literal would each flag an edge that must stay an inlier."""
    s, want, info = P.threshold_scene()
    assert float(P.TH_MONO) > 5.991 and float(P.TH_STEREO) > 7.815
    for (name, chi2, tgt), flag in zip(info, want):
        th = P.TH_STEREO if name.startswith("stereo") else P.TH_MONO
        assert np.float32(chi2) == tgt
        if name.endswith("at+"):
            assert tgt == th and chi2 > float(th) > (7.815 if name.startswith("stereo") else 5.991) and flag == 0
        elif name.endswith("at-"):
            assert tgt == th and chi2 < float(th) and flag == 0
        elif name.endswith("above"):
            assert tgt == np.nextafter(th, np.float32(np.inf)) and flag == 1
        else:
            assert tgt == np.nextafter(th, np.float32(-np.inf)) and flag == 0
    ref = s.run_py()
    got = host(s)
    assert list(want) == [0, 0, 1, 0, 0, 0, 1, 0]
    assert np.array_equal(ref[1], want) and np.array_equal(got.outlier, want)  # the flags, explicitly, on both
    assert ref[2] == got.ninliers == 6 and ref[3] == got.status == P.OK
    assert ref[4].tolist() == [1, 1, 0, 0, 0, 10, 10, 10]  # one round, one iteration of ten failed, rejected trials
    assert same(ref, got)
    # the twin of the rule alone, at the constants themselves
    for th, st in ((P.TH_MONO, False), (P.TH_STEREO, True)):
        assert P.edge_outlier(float(th), st) == 0
        assert P.edge_outlier(float(np.nextafter(th, np.float32(np.inf))), st) == 1
        assert P.edge_outlier(np.nextafter(float(th), np.inf), st) == 0  # one double above: still the same float


# ------------------------------------------------------------------------------------------------ helpers
def directed_angles():
    v = [1e-5, np.nextafter(1e-5, 1), 0.5, 1.0, 1048575.9, 1048576.0, 2e6, float("inf"), float("nan")]
    for k in range(1, 12):
        for base in (k * math.pi / 4, k * math.pi / 2):
            v += [base, np.nextafter(base, 0), np.nextafter(base, 100)]
    return v


def test_so3_sincos_hook_equals_restatement():
    rng = np.random.default_rng(2)
    th = np.concatenate([rng.uniform(1e-5, math.pi, 1 << 15), 10 ** rng.uniform(-5, 5.5, 1 << 15), directed_angles()])
    sn, cs = np.zeros_like(th), np.zeros_like(th)
    assert orbamd.load().orbx_test_so3_sincos(th.ctypes.data, sn.ctypes.data, cs.ctypes.data, len(th)) == 0
    ref = np.array([P.so3_sincos(float(t)) for t in th])
    assert ref[:, 0].tobytes() == sn.tobytes() and ref[:, 1].tobytes() == cs.tobytes()
    small = th < 100
    assert np.abs(sn[small] - np.sin(th[small])).max() < 1e-15 and np.abs(cs[small] - np.cos(th[small])).max() < 1e-15


def test_ldlt6_solve_against_numpy():
    rng = np.random.default_rng(4)
    lib = orbamd.load()
    worst = 0.0
    for _ in range(200):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        A = Q @ np.diag(10 ** rng.uniform(0, 4, 6)) @ Q.T
        A = np.ascontiguousarray((A + A.T) / 2)
        b = rng.normal(size=6)
        x = np.zeros(6)
        assert lib.orbx_test_ldlt6_solve(A.ctypes.data, b.ctypes.data, x.ctypes.data) == 1
        ok, xp = P.ldlt6_solve(A.tolist(), b.tolist())
        assert ok and np.array(xp).tobytes() == x.tobytes()
        ref = np.linalg.solve(A, b)
        worst = max(worst, np.abs(x - ref).max() / np.abs(ref).max())
    print("ldlt6_solve: largest relative error against numpy %.3g (bound %.3g)" % (worst, LDLT_BOUND))
    assert worst <= LDLT_BOUND


# ------------------------------------------------------------------------------------------------ bad input
def test_contract_excluded_inputs():
    base = P.make_scene("my", 30, "mixed", 0.5, seed=12)
    inc = np.full(base.n, 0x33, np.uint8)
    edge = int(np.flatnonzero(base.mp_index >= 0)[5])

    def variant(f):
        s = P.make_scene("my", 30, "mixed", 0.5, seed=12)
        f(s)
        return s
    cases = [variant(lambda s: s.T0.__setitem__((1, 2), np.nan)),
             variant(lambda s: s.kps["octave"].__setitem__(edge, 8)),
             variant(lambda s: s.kps["octave"].__setitem__(edge, -1)),
             variant(lambda s: s.kps["x"].__setitem__(edge, np.inf)),
             variant(lambda s: s.uright.__setitem__(edge, np.nan)),
             variant(lambda s: s.pos.__setitem__((s.mp_index[edge], 1), np.inf))]
    z = variant(lambda s: None)  # a point on the camera's plane z = 0: a non-finite chi2 at the first evaluation
    z.T0 = np.eye(4, dtype=np.float32)
    z.pos[z.mp_index[edge]] = (0.5, 0.5, 0.0)
    cases.append(z)
    for s in cases:
        ref = s.run_py(outlier=inc)
        got = host(s, outlier=inc)
        assert ref[3] == P.EXCLUDED and ref[2] == 0 and same(ref, got)
        assert (got.outlier == 0x33).all() and got.Tcw.tobytes() == s.T0.tobytes()
    # the same defects on a feature without a MapPoint are not read
    s = variant(lambda s: s.kps["octave"].__setitem__(int(np.flatnonzero(s.mp_index < 0)[0]), 99))
    assert s.run_py()[3] == P.OK and same(s.run_py(), host(s))


def test_argument_errors():
    lib = orbamd.load()
    s = P.make_scene("my", 12, "stereo", 0.0, seed=1)
    g = geom_of(s)
    inv = np.zeros(16, np.float32)
    inv[:8] = s.inv
    T = s.T0.copy().reshape(16)
    out = np.full(s.n, 9, np.uint8)
    ninl, st = C.c_int(-7), C.c_int(-7)
    kps = np.ascontiguousarray(s.kps)
    a = dict(g=C.byref(g), inv=inv.ctypes.data, nl=8, T=T.ctypes.data, n=s.n, kps=kps.ctypes.data,
             ur=s.uright.ctypes.data, mp=s.mp_index.ctypes.data, pos=s.pos.ctypes.data, out=out.ctypes.data,
             ninl=C.byref(ninl), st=C.byref(st), diag=None)
    order = ("g", "inv", "nl", "T", "n", "kps", "ur", "mp", "pos", "out", "ninl", "st", "diag")

    def call(**kw):
        return lib.orbx_pose_optimization(*[dict(a, **kw)[k] for k in order])
    for k in ("g", "inv", "T", "kps", "mp", "pos", "out", "ninl", "st"):
        assert call(**{k: None}) == E, k
    assert call(n=-1) == E and call(n=65537) == E and call(nl=0) == E and call(nl=17) == E
    assert T.tobytes() == s.T0.tobytes() and (out == 9).all() and ninl.value == st.value == -7
    assert call(n=0, kps=None, mp=None, pos=None, out=None) == 0 and st.value == P.TOO_FEW
    # the device entry's checks return before any device is touched
    dev = lib.orbm_pose_optimization_batch_device
    p = 0x1000
    good = [p, 1, p, 1, p, p, 64, p, C.byref(g), inv.ctypes.data, p, p, 10, p, p, p, None, None, p, None, p, None]
    for idx, bad in ((0, None), (1, -1), (3, 0), (6, 0), (6, 65537), (8, None), (9, None), (12, -1)):
        args = list(good)
        args[idx] = bad
        assert dev(*args) == E, idx
    for idx in (2, 4, 5, 10, 11, 13, 14, 15, 18, 20):
        args = list(good)
        args[idx] = None
        assert dev(*args) == E, idx
    args = list(good)
    args[4] = p + 4  # d_kps_un not 8-byte aligned
    assert dev(*args) == E

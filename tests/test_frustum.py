"""Frame::isInFrustum on the host (csrc/frustum.c through orbamd.frame) against the pure-Python restatement
tests/frustum_py.py, bit for bit; its directed boundary rows; the argument checks of the host unit and of the two device
entry points, which return before any device is touched; the host unit as a stand-alone C program under ASan + UBSan;
and tools/check_logf.c on a stride of the float range. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frustum_py as FP
import orbamd
import undistort_py as U
from orbamd.frame import is_in_frustum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
FIXTURE = os.path.join(ROOT, "tests", "golden", FP.FIXTURE)
CAMS = sorted(U.CAMERAS)
E = -1  # ORBX_EARG
f32 = np.float32


@pytest.fixture(scope="module")
def restated():
    """per camera: (geometry, [(pose, cloud, restated fields)]), computed once"""
    out = {}
    for ci, name in enumerate(CAMS):
        g = FP.camera_geom(name)
        per_pose = []
        for pi, T in enumerate(FP.poses()):
            cloud = FP.cloud(g, T, 300, 100 * ci + pi)
            per_pose.append((T, cloud, FP.is_in_frustum(g, T, 0.5, *cloud)))
        out[name] = (g, per_pose)
    return out


@pytest.mark.parametrize("name", CAMS)
def test_host_equals_restatement_bitwise(restated, name):
    g, per_pose = restated[name]
    assert len(per_pose) == 3
    for T, cloud, ref in per_pose:
        got = is_in_frustum(g.cstruct(), g.log_scale_factor, T, *cloud)
        assert ref.same_as(*got)
        # the cloud reaches every outcome and every level: the comparison sees every branch
        why = np.bincount(ref.why, minlength=7)
        assert why[FP.IN_VIEW] >= 75 and all(why[r] >= 10 for r in FP.REJECTIONS) and why[FP.EXCLUDED] == 0
        assert sorted(set(ref.level[ref.in_view == 1])) == list(range(8))
        rej = ref.in_view == 0
        assert not (got[1][rej].any() or got[2][rej].any() or got[3][rej].any() or got[4][rej].any() or got[5][rej].any())
    assert not np.array_equal(per_pose[0][2].proj_x, per_pose[1][2].proj_x)


def test_restatement_fixed_numbers():
    """a hand-computed point: fx = fy = 2, cx = cy = 1, bf = 8, a quarter turn about z and a translation.
    Pc = R P + t = (-4 + 1, 3 + 2, 1 + 3) = (-3, 5, 4); invz = 0.25; u = 2 * -3 * 0.25 + 1 = -0.5, v = 2 * 5 * 0.25 + 1
    = 3.5; Ow = -R^T t = (-2, 1, -3); PO = (5, 3, 4), dist = sqrt(50); Pn = (0.6, 0, 0.8): viewCos = 6.2 / sqrt(50);
    ratio = 4 sqrt(50) / sqrt(50) = 4 -> level = ceil(log 4 / log 1.2) = ceil(7.6) = 8 -> 7 of 8; xr = -0.5 - 8 * 0.25"""
    g = FP.Geom(2.0, 2.0, 1.0, 1.0, 8.0, (-4.0, 4.0, -4.0, 4.0))
    T = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], f32)
    Ow = FP.camera_center(T)
    assert [float(v) for v in Ow] == [-2.0, 1.0, -3.0]
    d50 = f32(np.sqrt(50.0))
    P, Pn = (3.0, 4.0, 1.0), (f32(0.6), 0.0, f32(0.8))
    why, u, v, xr, level, vc = FP.frustum_one(g, T, Ow, 0.5, P, Pn, 1.0, f32(4.0) * d50)
    assert (why, float(u), float(v), float(xr), level) == (FP.IN_VIEW, -0.5, 3.5, -2.5, 7)
    assert abs(float(vc) - 6.2 / np.sqrt(50.0)) < 1e-7
    g16 = FP.Geom(2.0, 2.0, 1.0, 1.0, 8.0, (-4.0, 4.0, -4.0, 4.0), nlevels=16)
    assert FP.frustum_one(g16, T, Ow, 0.5, P, Pn, 1.0, f32(4.0) * d50)[4] == 8
    # each test in turn: behind the camera, left of the image, below it, too near, too far, seen from behind
    assert FP.frustum_one(g, T, Ow, 0.5, (3.0, 4.0, -4.0), Pn, 1.0, 100.0)[0] == FP.DEPTH
    assert FP.frustum_one(g, T, Ow, 0.5, (3.0, 14.0, 1.0), Pn, 1.0, 100.0)[0] == FP.BOUNDS_U
    assert FP.frustum_one(g, T, Ow, 0.5, (13.0, 4.0, 1.0), Pn, 1.0, 100.0)[0] == FP.BOUNDS_V
    assert FP.frustum_one(g, T, Ow, 0.5, P, Pn, 10.0, 100.0)[0] == FP.DISTANCE
    assert FP.frustum_one(g, T, Ow, 0.5, P, Pn, 1.0, 5.0)[0] == FP.DISTANCE
    assert FP.frustum_one(g, T, Ow, 0.5, P, (0.0, 0.0, -1.0), 1.0, 100.0)[0] == FP.VIEW_COS
    got = is_in_frustum(g.cstruct(), g.log_scale_factor, T, [P], [Pn], [1.0], [f32(4.0) * d50])
    assert (got[0][0], got[1][0], got[2][0], got[3][0], got[4][0], got[5][0]) == (1, u, v, xr, 7, vc)


def test_directed_boundary_rows():
    """every row of frustum_py.directed_rows: the restatement gives the stated outcome, the host unit gives the
    restatement's bits, and the boundaries lie where the rows say (equality is in view, one ulp outside is not)"""
    g = FP.EXACT
    rows = FP.directed_rows()
    labels = [r[0] for r in rows]
    assert len(set(labels)) == len(labels) == 96
    levels = {}
    with np.errstate(all="ignore"):
        for label, T, P, Pn, mind, maxd, why in rows:
            assert mind is not None and maxd is not None, label  # factor_for found the threshold
            ref = FP.frustum_one(g, T, FP.camera_center(T), 0.5, P, Pn, mind, maxd)
            if why is not None:
                assert ref[0] == why, (label, ref)
            got = is_in_frustum(g.cstruct(), g.log_scale_factor, T, [P], [Pn], [mind], [maxd])
            want = FP.is_in_frustum(g, T, 0.5, [P], [Pn], [mind], [maxd])
            assert want.why[0] == ref[0] and want.same_as(*got), (label, ref, got)
            if label.startswith("ratio=") and ref[0] == FP.IN_VIEW:
                levels[label[6:]] = ref[4]
    # u = 512 X: the boundary rows hit the bounds exactly
    for label, T, P, Pn, mind, maxd, why in rows:
        if label in ("u=min_x", "u=max_x", "v=min_y", "v=max_y"):
            r = FP.frustum_one(g, T, FP.camera_center(T), 0.5, P, Pn, mind, maxd)
            assert (r[1] if label[0] == "u" else r[2]) == getattr(g, label[2:]), label
    r = {lab: FP.frustum_one(g, T, FP.camera_center(T), 0.5, P, Pn, mi, ma) for lab, T, P, Pn, mi, ma, _ in rows
         if lab.startswith("cos=")}
    assert r["cos=limit"][5] == f32(0.5) and r["cos=limit+1ulp"][5] == FP.up(0.5)
    # PredictScale: logf's early return, every level, the steps one ulp above a power of 1.2f, both clamps
    assert levels["1"] == 0 and levels["1+1ulp"] == 1 and levels["1-1ulp"] == 0
    assert [levels["1.2^%d" % k] for k in range(-1, 10)] == [0, 0, 1, 2, 3, 4, 5, 6, 7, 7, 7]
    assert [levels["1.2^%d+1ulp" % k] for k in range(0, 7)] == [1, 2, 3, 4, 5, 6, 7]
    assert "1.2^-2" not in levels  # beyond 1.2f * max_dist: the distance test takes it first


def _args(n=4):
    g = FP.EXACT.cstruct()
    T = np.eye(4, dtype=f32)
    pos = np.tile(np.array([0, 0, 2], f32), (n, 1))
    nrm = np.tile(np.array([0, 0, 1], f32), (n, 1))
    mind, maxd = np.full(n, 0.01, f32), np.full(n, 100, f32)
    outs = [np.full(n, 7, np.uint8)] + [np.full(n, 7, f32) for _ in range(3)] + [np.full(n, 7, np.int32),
                                                                                np.full(n, 7, f32)]
    keep = [T, pos, nrm, mind, maxd] + outs
    a = [C.byref(g), float(FP.EXACT.log_scale_factor), T.ctypes.data, 0.5, n, pos.ctypes.data, nrm.ctypes.data,
         mind.ctypes.data, maxd.ctypes.data] + [o.ctypes.data for o in outs]
    return g, a, outs, keep


def test_bad_arguments_write_nothing():
    lib = orbamd.load()
    g, a, outs, keep = _args()
    assert lib.orbx_is_in_frustum(*a) == 0 and (outs[0] == 1).all() and (outs[4] == 7).all()
    for o in outs:
        o[:] = 7
    for i in (0, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14):
        b = list(a)
        b[i] = None
        assert lib.orbx_is_in_frustum(*b) == E, i
    for i, v in ((4, -1), (1, 0.0), (1, -0.2), (1, float("nan")), (1, float("inf")), (3, float("nan"))):
        b = list(a)
        b[i] = v
        assert lib.orbx_is_in_frustum(*b) == E, (i, v)
    for nl in (0, -1, 17):
        bad = FP.EXACT.cstruct()
        bad.nlevels = nl
        assert lib.orbx_is_in_frustum(C.byref(bad), *a[1:]) == E, nl
    assert all((o == 7).all() for o in outs)
    assert lib.orbx_is_in_frustum(a[0], a[1], a[2], a[3], 0, *([None] * 10)) == 0


def test_frustum_batch_bad_arguments_need_no_device():
    lib = orbamd.load()
    fn = lib.orbx_is_in_frustum_batch_device
    g = FP.EXACT.cstruct()
    P = 0x1000  # never dereferenced: every call returns at its argument check
    good = [P, C.byref(g), 0.18, 0.5, 5, P, P, P, P, 3, P, P, P, P, P, P, P, None]
    for i in (0, 1, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16):
        b = list(good)
        b[i] = None
        assert fn(*b) == E, i
    for i, v in ((4, -1), (9, -1), (9, 65536), (2, 0.0), (2, float("nan")), (3, float("inf"))):
        b = list(good)
        b[i] = v
        assert fn(*b) == E, (i, v)
    for nl in (0, 17):
        bad = FP.EXACT.cstruct()
        bad.nlevels = nl
        b = list(good)
        b[1] = C.byref(bad)
        assert fn(*b) == E, nl


def test_local_points_batch_bad_arguments_need_no_device():
    lib = orbamd.load()
    fn = lib.orbm_search_local_points_batch_device
    g = FP.EXACT.cstruct()
    P = 0x1000
    #       ctx nf kps desc cnt  S   ur   Tcw geom         lsf  M  pos nrm min max mpd fl rng  fmp th   nn   cos  m  nm ntm inv st
    good = [P, 3, P, P, P, 128, None, P, C.byref(g), 0.18, 9, P, P, P, P, P, P, None, P, 1.0, 0.8, 0.5, P, P, P, None, None]
    for i in (0, 2, 3, 4, 7, 8, 11, 12, 13, 14, 15, 16, 18, 22, 23, 24):
        b = list(good)
        b[i] = None
        assert fn(*b) == E, i
    for i, v in ((1, -1), (5, 0), (5, 65537), (10, -1), (2, P + 4), (3, P + 8), (15, P + 8), (9, 0.0),
                 (9, float("nan")), (21, float("nan"))):
        b = list(good)
        b[i] = v
        assert fn(*b) == E, (i, v)
    for nl in (0, -1, 17):
        bad = FP.EXACT.cstruct()
        bad.nlevels = nl
        b = list(good)
        b[8] = C.byref(bad)
        assert fn(*b) == E, nl


# ------------------------------------------------------------------------------------------------ the C programs
@pytest.fixture(scope="module")
def built():
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp", "build_frustum.sh")])
    return BUILD


def run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-4000:])
    return r


def test_fixture_is_the_restatement():
    """the committed vectors are what tests/frustum_py.py computes (python tests/frustum_py.py rewrites them)"""
    assert open(FIXTURE).read() == FP.fixture_text()


def test_host_unit_over_the_fixture(built):
    r = run(os.path.join(built, "test_frustum"), FIXTURE)
    assert r.returncode == 0 and "ALL PASS" in r.stdout


def test_host_unit_under_asan_ubsan(built):
    r = run(os.path.join(built, "test_frustum_asan"), FIXTURE)
    assert r.returncode == 0 and "ALL PASS" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr


def test_logf_restatement_on_a_stride_of_the_float_range(built):
    """tools/check_logf.c, the C statement of the device logf, against this machine's libm on every 997th positive
    normal float, in both evaluation orders; the full range (stride 1) is the manual check"""
    r = run(os.path.join(built, "check_logf"), "997")
    assert r.returncode == 0
    lines = r.stdout.strip().splitlines()
    n = (0x7f800000 - 0x00800000 + 996) // 997
    assert len(lines) == 2 and all(ln.endswith("%d floats, logf mismatches 0" % n) for ln in lines)

"""The per-match loop of LocalMapping::CreateNewMapPoints on the host (csrc/triangulate.c through orbamd.frame) against
the pure-Python restatement tests/triangulate_py.py, bit for bit, on every pair of the three reference cameras' scenes;
the outcomes the scenes reach; a hand-computed case and directed rows at every boundary; the float Jacobi's null vector
against numpy's SVD; the baseline skip; the argument checks of the host and device entries, which return before any
device is touched; the order of the compacted table; tools/check_atan2f.c on a stride of the float range. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orbamd
import triangulate_py as TP
import undistort_py as U
from orbamd.frame import triangulate_matches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
CAMS = sorted(U.CAMERAS)
E = -1  # ORBX_EARG
f32, f64 = np.float32, np.float64


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


@pytest.fixture(scope="module")
def restated():
    """per camera: (geometry, [(pair, the yardstick's result)], stats), computed once"""
    out = {}
    for name in CAMS:
        g, pairs = TP.camera_scene(name)
        st = {}
        out[name] = (g, [(p, p.run(TP.triangulate_matches, stats=st)) for p in pairs], st)
    return out


def host(p):
    return triangulate_matches(p.g.cstruct(), p.monocular, p.median_depth2, p.T1, p.T2, p.kps1, p.ur1, p.d1, p.desc1,
                               p.kps2, p.ur2, p.d2, p.match12)


@pytest.mark.parametrize("name", CAMS)
def test_host_equals_restatement_bitwise(restated, name):
    g, runs, _ = restated[name]
    generated = [p for p, _ in runs if p.name.split("/")[0] in ("lateral", "forward", "rot+trans")]
    assert len(generated) == 9 and all(len(p.kps1) == 300 for p in generated)  # 3 poses x stereo, mono, mixed
    for p, ref in runs:
        got = host(p)
        assert ref.same_as(got), p.name
        made = np.isin(ref.status, TP.CREATED)
        assert not got.pos3[~made].any() and got.nnew == made.sum()


@pytest.mark.parametrize("name", CAMS)
def test_scene_reaches_every_outcome(restated, name):
    """asserted on the yardstick's output, not on the code under test: every outcome code at least 10 times per
    camera, the three creation branches included; the Jacobi converges within 5 sweeps of its 30"""
    _, runs, st = restated[name]
    tot = np.zeros(14, int)
    for _, ref in runs:
        tot += np.bincount(ref.status, minlength=14)
    assert (tot >= 10).all(), dict(zip(TP.NAMES, tot.tolist()))
    assert 2 <= st["sweeps"] <= 6


def test_compaction_keeps_idx1_order(restated):
    """table row k is the k-th created idx1, with its idx2, its position and the current keyframe's descriptor"""
    _, runs, _ = restated["my"]
    for p, ref in runs[:3]:
        got = host(p)
        made = np.flatnonzero(np.isin(got.status, TP.CREATED))
        assert len(made) == got.nnew > 100
        assert np.array_equal(got.feat1, made) and np.array_equal(got.feat2, p.match12[made])
        assert np.array_equal(got.tab_pos, got.pos3[made]) and np.array_equal(got.tab_desc, p.desc1[made])
        assert (got.tab_flags == 9).all()


# ------------------------------------------------------------------------------------------------ exact cases
EXACT = TP.TriGeom(512.0, 512.0, 0.0, 0.0, 64.0, b=0.125)
GZ = TP.TriGeom(512.0, 512.0, 256.0, 0.0, 64.0, b=0.125)  # cx = 256: room for mvuRight >= 0
I4 = np.eye(4, dtype=f32)


def shifted(tx, ty=0.0, tz=0.0):
    T = np.eye(4, dtype=f32)
    T[:3, 3] = (tx, ty, tz)
    return T


def one(g, T1, T2, kp1, kp2, ur1=-1.0, d1=-1.0, ur2=-1.0, d2=-1.0, monocular=0, med=1.0):
    """one match through the yardstick and the host unit: they agree; returns the yardstick's result"""
    k1, k2 = np.zeros(1, TP.KP), np.zeros(1, TP.KP)
    k1["x"], k1["y"], k1["octave"] = kp1
    k2["x"], k2["y"], k2["octave"] = kp2
    a = (g, monocular, med, T1, T2, k1, np.array([ur1], f32), np.array([d1], f32), np.zeros((1, 32), np.uint8), k2,
         np.array([ur2], f32), np.array([d2], f32), np.array([0], np.int32))
    ref = TP.triangulate_matches(*a)
    got = triangulate_matches(g.cstruct(), *a[1:])
    assert ref.same_as(got), (kp1, kp2, ref.status, got.status)
    return ref


def test_hand_computed_point():
    """fx = fy = 512, cx = cy = 0. KF1 at the origin, KF2 one unit to its right (Tcw2 = [I | (-1, 0, 0)], Ow2 =
    (1, 0, 0)). The point (1, 0.5, 4) projects to (128, 64) in KF1 and to (0, 64) in KF2; xn1 = (0.25, 0.125), xn2 =
    (0, 0.125). The system's rows are (-1, 0, 0.25, 0), (0, -1, 0.125, 0), (-1, 0, 0, 1), (0, -1, 0.125, 0): its null
    vector is (1, 0.5, 4, 1) / sqrt(18.25) exactly, so the triangulation is exact up to the Jacobi's float rotations.
    z1 = z2 = 4, both reprojections exact, dist1 = sqrt(17.25), dist2 = sqrt(16.25); normal = (n1 / |n1| + n2 / |n2|) / 2;
    octave 2: max = dist1 * 1.2^2, min = max / 1.2^7."""
    T2 = shifted(-1.0)
    r = one(EXACT, I4, T2, (128.0, 64.0, 2), (0.0, 64.0, 2))
    assert r.status[0] == TP.TRIANGULATED and r.nnew == 1
    assert np.allclose(r.tab_pos[0], (1.0, 0.5, 4.0), rtol=0, atol=4e-6)
    n1, n2 = np.array([1, 0.5, 4.0]), np.array([0, 0.5, 4.0])
    nrm = (n1 / np.linalg.norm(n1) + n2 / np.linalg.norm(n2)) / 2
    assert np.allclose(r.tab_normal[0], nrm, rtol=0, atol=1e-6)
    sf = EXACT.scale_factors
    assert abs(float(r.tab_max[0]) - np.sqrt(17.25) * float(sf[2])) < 1e-5
    assert r.tab_min[0] == f32(r.tab_max[0] / sf[7]) and r.feat1[0] == 0 and r.feat2[0] == 0
    # the same point from KF1's stereo when the neighbour has less parallax than the rig: x3D = (u / fx z, v / fy z, z)
    T2 = shifted(0.0, 0.0, -0.25)  # a quarter unit ahead: baseline 0.25 >= mb
    X = np.array([0.0625, 0.03125, 4.0])
    k2 = (256.0 + 512 * 0.0625 / 3.75, 512 * 0.03125 / 3.75, 0)
    r = one(GZ, I4, T2, (264.0, 4.0, 0), k2, ur1=264.0 - 64.0 / 4.0 + 16.0, d1=4.0)
    assert r.status[0] == TP.REPROJ1  # mvuRight 16 px off
    r = one(GZ, I4, T2, (264.0, 4.0, 0), k2, ur1=264.0 - 64.0 / 4.0, d1=4.0)
    assert r.status[0] == TP.STEREO1 and [float(v) for v in r.tab_pos[0]] == X.tolist()


def test_directed_boundary_rows():
    """rows at the boundary of each test, found by stepping an input one ulp at a time until the yardstick's
    intermediate crosses it; host and yardstick agree on every row (inside `one`), and the outcome flips exactly
    where the reference's comparison says"""
    g = EXACT
    with np.errstate(all="ignore"):
        # cosParallaxRays against 0.9998 (monocular, strict <): rays (x, 0, 1) and (0, 0, 1), cos = 1 / sqrt(1 + x^2)
        T2 = shifted(-1.0)
        seen = {}
        x0 = 512.0 * np.sqrt(1.0 / 0.9998 ** 2 - 1.0)
        for k in range(-80, 80):  # a float ulp of the cosine is about 1600 ulps of u: step u by 2^-13
            u = f32(x0 + k * 2.0 ** -13)
            xn = f32(u * (f32(1.0) / g.fx))
            c = f32(f64(1.0) / (np.sqrt(f64(xn) * f64(xn) + f64(1.0)) * np.sqrt(f64(1.0))))
            r = one(g, I4, T2, (u, 0.0, 0), (0.0, 0.0, 0))
            low = not f64(c) < f64(0.9998)
            assert (r.status[0] == TP.LOW_PARALLAX) == low, (u, c)
            seen[float(c)] = low
        # the float nearest 0.9998 lies above the double: a cosine of exactly 0.9998f is low parallax, one ulp below it
        # is enough
        assert f64(f32(0.9998)) > f64(0.9998)
        assert seen[float(f32(0.9998))] is True and seen[float(down(0.9998))] is False and len(seen) >= 6
        # cosParallaxRays exactly 0 (perpendicular rays) fails `> 0`: KF2 turned a quarter about y
        Tq = np.array([[0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, -1], [0, 0, 0, 1]], f32)
        assert one(g, I4, Tq, (0.0, 0.0, 0), (0.0, 0.0, 0)).status[0] == TP.LOW_PARALLAX
        # w == 0 and dist == 0: the degenerate pairs of the scenes, also under this geometry
        for pair, code in ((TP.w_zero_pair(GZ), TP.W_ZERO), (TP.dist_zero_pair(GZ), TP.DIST_ZERO)):
            ref = pair.run(TP.triangulate_matches)
            assert (ref.status == code).all() and ref.same_as(host(pair)), pair.name
        # z == 0 exactly: KF1's stereo point at depth 1 seen from a neighbour exactly one unit ahead (z2 = 1 - 1);
        # z1 <= 0 cannot follow a stereo point (depth > 0), nor a triangulation with positive parallax; one ulp nearer
        # the point is in front
        gz = GZ
        Tz = shifted(0.0, 0.0, -1.0)
        r = one(gz, I4, Tz, (256.0, 0.0, 0), (256.0, 0.0, 0), ur1=256.0 - 64.0, d1=1.0)
        assert r.status[0] == TP.Z2
        r = one(gz, I4, shifted(0.0, 0.0, down(-1.0)), (256.0, 0.0, 0), (256.0, 0.0, 0), ur1=256.0 - 64.0, d1=1.0)
        assert r.status[0] == TP.Z2
        r = one(gz, I4, shifted(0.0, 0.0, up(-1.0)), (256.0, 0.0, 0), (256.0, 0.0, 0), ur1=256.0 - 64.0, d1=1.0)
        assert r.status[0] != TP.Z2
        # reprojection error equal to the threshold passes (strict >): a stereo point at depth 4 whose second view is
        # off by e pixels in v only; 5.991 * sigma2 is no float square, so walk e across it
        T2 = shifted(0.0, 0.0, -0.25)
        e = f32(np.sqrt(5.991))
        flips = set()
        for _ in range(8):
            e = down(e)
        for _ in range(16):
            r = one(gz, I4, T2, (256.0, 0.0, 0), (256.0, e, 0), ur1=256.0 - 16.0, d1=4.0)
            e2 = f32(f32(0.0) + f32(e * e))
            want = TP.REPROJ2 if f64(e2) > f64(5.991) * f64(1.0) else TP.STEREO1
            assert r.status[0] == want, (e, e2)
            flips.add(int(r.status[0]))
            e = up(e)
        assert flips == {TP.REPROJ2, TP.STEREO1}
        # ratioDist * ratioFactor == ratioOctave passes (strict <): dist1 = 4, dist2 = 3.75... use exact distances:
        # KF1 at the origin, the stereo point at (0, 0, 4); KF2 at (0, 0, -d): dist2 = 4 + d. Octaves (0, o2) give
        # ratioOctave = 1 / sf[o2]; equality needs (4 + d) / 4 * 1.8f == 1 / sf[o2], impossible with dist2 > dist1, so
        # test the other side: ratioDist > ratioOctave * ratioFactor with ratioDist = 2 (d = 4) against octaves whose
        # product brackets 2
        rf = f32(f32(1.5) * g.scale_factors[1])
        hits = set()
        for o1 in range(8):
            for o2 in range(8):
                ro = f32(g.scale_factors[o1] / g.scale_factors[o2])
                r = one(gz, I4, shifted(0.0, 0.0, 4.0), (256.0, 0.0, o1), (256.0, 0.0, o2), ur1=256.0 - 16.0, d1=4.0)
                want_reject = f32(f32(2.0) * rf) < ro or f32(2.0) > f32(ro * rf)
                if r.status[0] in (TP.SCALE_RATIO, TP.STEREO1):
                    assert (r.status[0] == TP.SCALE_RATIO) == bool(want_reject), (o1, o2)
                    hits.add(int(r.status[0]))
        assert hits == {TP.SCALE_RATIO, TP.STEREO1}
    # exact equality on both sides of :430, from the restatement's own arithmetic: a power-of-two scale factor
    g2 = TP.TriGeom(512.0, 512.0, 256.0, 0.0, 64.0, b=0.125, scale_factor=2.0)  # ratioFactor = 3
    # dist1 = 4, dist2 = 12 (KF2 8 behind): ratioDist = 3 = ratioOctave (1) * 3: not above, kept
    r = one(g2, I4, shifted(0.0, 0.0, 8.0), (256.0, 0.0, 0), (256.0, 0.0, 0), ur1=256.0 - 16.0, d1=4.0)
    assert r.status[0] == TP.STEREO1
    r = one(g2, I4, shifted(0.0, 0.0, up(8.0)), (256.0, 0.0, 0), (256.0, 0.0, 0), ur1=256.0 - 16.0, d1=4.0)
    assert r.status[0] == TP.SCALE_RATIO
    # dist1 = 12, dist2 = 4 (KF2 8 ahead), octaves (2, 0): ratioOctave = 4 against ratioDist * 3 = 1: rejected; octaves
    # (0, 0): ratioDist * ratioFactor = 1 == ratioOctave: kept
    r = one(g2, I4, shifted(0.0, 0.0, -8.0), (256.0, 0.0, 0), (256.0, 0.0, 0), ur1=256.0 - 64.0 / 12.0, d1=12.0)
    assert r.status[0] == TP.STEREO1
    r = one(g2, I4, shifted(0.0, 0.0, -8.0), (256.0, 0.0, 2), (256.0, 0.0, 0), ur1=256.0 - 64.0 / 12.0, d1=12.0)
    assert r.status[0] == TP.SCALE_RATIO


def test_svd_null_vector_against_numpy(restated):
    """the float Jacobi's vt.row(3) against numpy.linalg.svd in double on the systems of the scenes' triangulated
    rows (540 of them), as the angle between the two null directions. The yardstick's own worst deviation measured on
    these scenes is 2.56e-7 rad (well-conditioned two-view systems, float rotations of unit-scale rows); the bound is 4
    times that for the float rotations, 1.03e-6 rad."""
    worst = 0.0
    n = 0
    for name in CAMS:
        g, runs, _ = restated[name]
        for p, ref in runs[:9:4]:
            invfx, invfy = f32(1.0) / g.fx, f32(1.0) / g.fy
            for i in np.flatnonzero(ref.status == TP.TRIANGULATED)[:60]:
                j = p.match12[i]
                xn1 = [f32(f32(p.kps1["x"][i] - g.cx) * invfx), f32(f32(p.kps1["y"][i] - g.cy) * invfy)]
                xn2 = [f32(f32(p.kps2["x"][j] - g.cx) * invfx), f32(f32(p.kps2["y"][j] - g.cy) * invfy)]
                A = TP.system_matrix(np.asarray(p.T1, f32), np.asarray(p.T2, f32), xn1, xn2)
                x = np.array(TP.svd4_null(A), f64)
                v = np.linalg.svd(np.array(A, f64))[2][3]
                c = abs(float(x @ v)) / (np.linalg.norm(x) * np.linalg.norm(v))
                worst = max(worst, float(np.arccos(min(c, 1.0))))
                n += 1
    print("worst angle", worst, "over", n)
    assert n > 300 and worst < 1.03e-6


def test_baseline_skip_in_both_modes():
    g = TP.camera_geom("my")
    T1 = TP.relative_poses()[0][1]
    for mono in (0, 1):
        p = TP.short_baseline_pair(g, T1, mono)
        ref = p.run(TP.triangulate_matches)
        assert ref.same_as(host(p)) and ref.nnew == 0
        assert (ref.status[p.match12 >= 0] == TP.BASELINE).all() and (ref.status[p.match12 < 0] == TP.NO_MATCH).all()
    # stereo: baseline == mb is kept (strict <); monocular: the ratio against 0.01 in double
    gb = TP.TriGeom(512.0, 512.0, 0.0, 0.0, 64.0, b=0.125)
    kept = one(gb, I4, shifted(-0.125), (128.0, 64.0, 0), (112.0, 64.0, 0))
    assert kept.status[0] != TP.BASELINE
    assert one(gb, I4, shifted(down(-0.125) + f32(2 ** -26)), (128.0, 64.0, 0), (112.0, 64.0, 0)).status[0] != TP.BASELINE
    assert one(gb, I4, shifted(-0.1249), (128.0, 64.0, 0), (112.0, 64.0, 0)).status[0] == TP.BASELINE
    assert f64(f32(0.01)) < 0.01  # the float quotient 0.01f is below the double 0.01: skipped
    assert one(gb, I4, shifted(-1.0), (128.0, 64.0, 0), (0.0, 64.0, 0), monocular=1, med=100.0).status[0] == TP.BASELINE
    assert one(gb, I4, shifted(-1.0), (128.0, 64.0, 0), (0.0, 64.0, 0), monocular=1, med=99.0).status[0] != TP.BASELINE


# ------------------------------------------------------------------------------------------------ argument checks
def test_host_bad_arguments_write_nothing():
    lib = orbamd.load()
    g = EXACT.cstruct()
    n = 3
    k = np.zeros(n, TP.KP)
    T = np.eye(4, dtype=f32)
    m = np.full(n, -1, np.int32)
    desc = np.zeros((n, 32), np.uint8)
    outs = [np.full(n, 7, np.int8), np.full(3 * n, 7, f32), np.full(3 * n, 7, f32), np.full(3 * n, 7, f32),
            np.full(n, 7, f32), np.full(n, 7, f32), np.full(32 * n, 7, np.uint8), np.full(n, 7, np.uint8),
            np.full(n, 7, np.int32), np.full(n, 7, np.int32)]
    nn = C.c_int(7)
    good = [C.byref(g), 0, 1.0, T.ctypes.data, T.ctypes.data, n, k.ctypes.data, None, None, desc.ctypes.data, n,
            k.ctypes.data, None, None, m.ctypes.data] + [o.ctypes.data for o in outs] + [C.byref(nn)]
    fn = lib.orbx_triangulate_matches
    for i in (0, 3, 4, 6, 9, 11, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25):
        b = list(good)
        b[i] = None
        assert fn(*b) == E, i
    for i, v in ((5, -1), (10, -1)):
        b = list(good)
        b[i] = v
        assert fn(*b) == E, (i, v)
    for field, v in (("nlevels", 0), ("nlevels", 17), ("fx", 0.0), ("fy", 0.0)):
        bad = EXACT.cstruct()
        setattr(bad, field, v)
        assert fn(C.byref(bad), *good[1:]) == E, field
    assert all((o == 7).all() for o in outs) and nn.value == 7
    assert fn(*good) == 0 and nn.value == 0 and (outs[0] == 0).all() and not outs[1].any()
    assert fn(good[0], 0, 1.0, good[3], good[4], 0, *([None] * 4), 0, *([None] * 14), C.byref(nn)) == 0


def test_device_entry_bad_arguments_need_no_device():
    lib = orbamd.load()
    fn = lib.orbm_create_new_map_points_batch_device
    g = EXACT.cstruct()
    P = 0x1000  # never dereferenced: every call returns at its argument check
    #       ctx np q1 q2 nf kps cnt S   ur d  desc Tcw m  geom        mono med st pos3 ... range nnew stream
    good = [P, 2, P, P, 3, P, P, 128, P, P, P, P, P, C.byref(g), 0, None] + [P] * 12 + [None]
    for i in (0, 2, 3, 5, 6, 10, 11, 12, 13) + tuple(range(16, 28)):
        b = list(good)
        b[i] = None
        assert fn(*b) == E, i
    for i, v in ((1, -1), (4, 0), (4, -1), (7, 0), (7, 65537), (5, P + 4), (10, P + 8), (22, P + 8), (8, None),
                 (9, None), (14, 1)):
        b = list(good)
        b[i] = v
        assert fn(*b) == E, (i, v)
    for field, v in (("nlevels", 0), ("nlevels", -1), ("nlevels", 17), ("fx", 0.0), ("fy", 0.0)):
        bad = EXACT.cstruct()
        setattr(bad, field, v)
        b = list(good)
        b[13] = C.byref(bad)
        assert fn(*b) == E, (field, v)
    b = list(good)
    b[1], b[7] = 65536, 65536  # npairs * kp_stride beyond the int32 rows of d_new_range
    assert fn(*b) == E


# ------------------------------------------------------------------------------------------------ the C program
@pytest.fixture(scope="module")
def built():
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp", "build_triangulate.sh")])
    return BUILD


def test_atan2f_restatement_on_a_stride_of_the_float_range(built):
    """tools/check_atan2f.c, the C statement of the device atanf / atan2f, against this machine's libm on every 997th
    positive finite float and on first-quadrant pairs; stride 3 is the manual check"""
    r = subprocess.run([os.path.join(built, "check_atan2f"), "997"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    lines = r.stdout.strip().splitlines()
    n = (0x7f800000 - 1 + 996) // 997
    assert len(lines) == 2 and lines[0] == "atanf: %d floats, mismatches 0" % n
    assert lines[1].startswith("atan2f: ") and lines[1].endswith(" pairs, mismatches 0")

"""The epipolar tile cull of the BF SearchForTriangulation scan (csrc/orb_tri_cull.h), on the CPU: the ordering, the
tile records and tri_tile_dead are the kernel's own lines, built into a host library (tests/cpp/tri_cull_host.cpp).

The exact predicate is restated here in numpy float32, one rounding per operation as epi_line / epi_ok_f
(orb_match_dev.h, match_kernels.hip) state it. For every geometry: no (query, candidate) pair the exact predicate
accepts lies in a (query, tile) the cull calls dead -- zero misses. On the C2 fixture a wave of 32 ordered queries
keeps at most 20 % of the candidate tiles (measured when the cull was proposed: 14.5 %), so an ordering regression
cannot quietly give the speed back."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from match_cases import KP, scale_table

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("c2_640x480_1000", "c3_752x480_1200", "c4_1241x376_2000")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp", "build_tri_cull.sh")])
    so = C.CDLL(os.path.join(ROOT, "tests", "cpp", "build", "libtricull.so"))
    so.tricull_plan.restype = C.c_int
    so.tricull_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]
    return so


def thf_table(sigma2):
    """MatchGeom::th384f: 3.84 * (double)sigma2 rounded up to a float"""
    t = 3.84 * sigma2.astype(np.float64)
    f = t.astype(f32)
    return np.where(f.astype(np.float64) < t, np.nextafter(f, f32(np.inf)), f).astype(f32)


def lines(F, xy1):
    """epi_line: a = fl(fl(fl(x1 F0) + fl(y1 F3)) + F6), ..."""
    F = F.reshape(9).astype(f32)
    x, y = xy1[:, 0], xy1[:, 1]
    return [(x * F[k] + y * F[3 + k]) + F[6 + k] for k in range(3)]


def accepted(F, xy1, xy2, thf2):
    """[n1, n2] bool: epi_ok_f of every pair, in float32 with the kernel's roundings"""
    with np.errstate(all="ignore"):
        a, b, c = (v[:, None] for v in lines(F, xy1))
        num = (a * xy2[None, :, 0] + b * xy2[None, :, 1]) + c
        den = a * a + b * b
        dsqr = (num * num) / den
        return (den != 0) & (dsqr < thf2[None, :])


def plan(lib, F, xy1, xy2, thf2):
    n1, n2 = len(xy1), len(xy2)
    F = np.ascontiguousarray(F, f32).reshape(9)
    xy1, xy2, thf2 = (np.ascontiguousarray(v, f32) for v in (xy1, xy2, thf2))
    ntiles = (n2 + 31) // 32
    permQ, permC = np.zeros(n1, np.uint16), np.zeros(n2, np.uint16)
    tiles, dead = np.zeros((max(ntiles, 1), 8), f32), np.zeros(n1 * ntiles + 1, np.uint8)
    rc = lib.tricull_plan(F.ctypes.data, n1, xy1.ctypes.data, n2, xy2.ctypes.data, thf2.ctypes.data,
                          permQ.ctypes.data, permC.ctypes.data, tiles.ctypes.data, dead.ctypes.data)
    assert rc == ntiles
    return permQ, permC, dead[:n1 * ntiles].reshape(n1, ntiles).astype(bool)


def check(lib, F, xy1, xy2, thf2):
    """zero misses; returns (kept-tile share per wave of 32 queries, number of accepted pairs)"""
    xy1, xy2, thf2 = (np.asarray(v, f32) for v in (xy1, xy2, thf2))
    permQ, permC, dead = plan(lib, F, xy1, xy2, thf2)
    n1, n2 = len(xy1), len(xy2)
    assert sorted(permQ.tolist()) == list(range(n1)) and sorted(permC.tolist()) == list(range(n2))
    for t in range(0, n2, 32):  # rows of a tile ascend in the original index (the tie rule needs it)
        assert (np.diff(permC[t:t + 32].astype(int)) > 0).all()
    if n1 == 0 or n2 == 0:
        return 0.0, 0
    tile_of = np.empty(n2, int)
    tile_of[permC] = np.arange(n2) // 32
    acc = accepted(F, xy1, xy2, thf2)[permQ]  # rows in query order
    qi, cj = np.nonzero(acc)
    misses = int(dead[qi, tile_of[cj]].sum())
    assert misses == 0, "%d accepted pairs lie in a culled (query, tile)" % misses
    kept = [(~dead[w:w + 32]).any(axis=0).mean() for w in range(0, n1, 32)]
    return float(np.mean(kept)), len(qi)


def fixture(name, swap):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    k1, k2 = (d[k].copy().view(np.dtype(KP)).reshape(-1) for k in (("kps0", "kps1") if swap else ("kps1", "kps0")))
    thf = thf_table((scale_table() ** 2).astype(f32))
    F = d["F12"].astype(f32)
    F = np.ascontiguousarray(F.T) if swap else F
    ex, ey = f32(d["ex"]), f32(d["ey"])
    xy = lambda k: np.stack([k["x"], k["y"]], 1).astype(f32)  # noqa: E731
    th2 = thf[k2["octave"]].copy()
    if not swap:  # the mono form's near-epipole candidates take no part (threshold -1)
        dx, dy = ex - k2["x"], ey - k2["y"]
        th2[(dx * dx + dy * dy) < (100 * scale_table())[k2["octave"]]] = -1
    return F, xy(k1), xy(k2), th2


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_no_accepted_pair_is_culled(lib, name, swap):
    share, nacc = check(lib, *fixture(name, swap))
    print("%s swap=%d: kept-tile share per wave %.3f, %d accepted pairs" % (name, swap, share, nacc))
    assert nacc > 0


def test_c2_wave_keeps_at_most_a_fifth_of_the_tiles(lib):
    share, _ = check(lib, *fixture(FIXTURES[0], False))
    print("C2 kept-tile share per wave: %.4f" % share)
    assert share <= 0.20


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def random_geometry(rng, kind):
    """F12 of a random relative pose under a 640 x 480 pinhole camera; kind: where the epipole falls"""
    K = np.array([[500 + 300 * rng.random(), 0, 320], [0, 500 + 300 * rng.random(), 240], [0, 0, 1]])
    w = rng.normal(size=3) * {"far": 0.02, "inside": 0.05, "rotated": 0.6, "sideways": 0.0}[kind]
    th = np.linalg.norm(w)
    Kx = skew(w / th) if th > 0 else np.zeros((3, 3))
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = {"far": np.array([1, 0.1 * rng.normal(), 0.2 * rng.normal()]),
         "inside": np.array([0.1 * rng.normal(), 0.1 * rng.normal(), 1.0]),
         "rotated": rng.normal(size=3),
         "sideways": np.array([1.0, 0.0, 0.0])}[kind]
    Ki = np.linalg.inv(K)
    F = Ki.T @ skew(t) @ R @ Ki
    return (F * 10.0 ** rng.integers(-6, 3)).astype(f32)  # any scale: the predicate is homogeneous in F


@pytest.mark.parametrize("kind", ["far", "inside", "rotated", "sideways"])
def test_random_geometries(lib, kind):
    rng = np.random.default_rng([3840, sum(map(ord, kind))])
    thf = thf_table((scale_table() ** 2).astype(f32))
    total = 0
    for _ in range(6):
        F = random_geometry(rng, kind)
        n1, n2 = int(rng.integers(1, 700)), int(rng.integers(1, 700))
        xy1 = (rng.random((n1, 2)) * [640, 480]).astype(f32)
        xy2 = (rng.random((n2, 2)) * [640, 480]).astype(f32)
        th2 = thf[rng.integers(0, 8, n2)]
        th2[rng.random(n2) < 0.05] = -1
        share, nacc = check(lib, F, xy1, xy2, th2)
        total += nacc
        print(kind, "n1 %d n2 %d: kept share %.3f, %d accepted pairs" % (n1, n2, share, nacc))
    assert total > 0


def test_degenerate_inputs(lib):
    """F = 0 (no pair passes, every tile dead), every keypoint at one point, near-degenerate lines (a query at the
    epipole of the first image: a = b = c ~ 0), NaN / inf coordinates: always a permutation, never a miss"""
    rng = np.random.default_rng(77)
    thf = thf_table((scale_table() ** 2).astype(f32))
    n = 200
    xy = (rng.random((n, 2)) * [640, 480]).astype(f32)
    th2 = thf[rng.integers(0, 8, n)]
    Fz = np.zeros((3, 3), f32)
    permQ, permC, dead = plan(lib, Fz, xy, xy, th2)
    assert dead.all() and check(lib, Fz, xy, xy, th2)[1] == 0
    one = np.tile(np.array([[123.25, 77.5]], f32), (n, 1))
    F = random_geometry(rng, "inside")
    check(lib, F, one, one, th2)
    # queries at and around the first image's epipole e1 (F12^T ... a = b = c = 0 for x1 = e1: F12^T e1 = 0)
    _, _, vt = np.linalg.svd(F.astype(np.float64).T)
    e1 = vt[-1] / vt[-1][2]
    near = (e1[:2] + rng.normal(size=(n, 2)) * np.array([1e-3, 1e-3])).astype(f32)
    near[0] = e1[:2].astype(f32)
    check(lib, F, near, xy, th2)
    bad = xy.copy()
    bad[::7, 0] = np.nan
    bad[3::11, 1] = np.inf
    bad[5::13, 0] = -np.inf
    check(lib, F, bad, bad, th2)
    check(lib, (F * f32(1e30)).astype(f32), xy, xy, th2)  # den overflows
    check(lib, (F * f32(1e-30)).astype(f32), xy, xy, th2)  # den underflows


def test_candidates_a_few_ulps_either_side_of_the_threshold(lib):
    """candidates walked ulp by ulp across dsqr == thf, at box corners and alone in their tile: the ones the exact
    predicate accepts are never in a culled tile"""
    rng = np.random.default_rng(384)
    thf = thf_table((scale_table() ** 2).astype(f32))
    total = 0
    for kind in ("far", "inside", "sideways"):
        F = random_geometry(rng, kind)
        xy1 = (rng.random((64, 2)) * [640, 480]).astype(f32)
        a, b, c = (v.astype(np.float64) for v in lines(F, xy1))
        cands, ths = [], []
        for i in range(len(xy1)):
            o = int(rng.integers(0, 8))
            nrm = np.hypot(a[i], b[i])
            if not nrm > 0:
                continue
            # a point of the line, moved along the normal to the edge of the band, then +-4 ulps in x and in y
            x0 = rng.random() * 640
            y0 = -(a[i] * x0 + c[i]) / b[i] if abs(b[i]) > abs(a[i]) else rng.random() * 480
            if abs(b[i]) <= abs(a[i]):
                x0 = -(b[i] * y0 + c[i]) / a[i]
            for sgn in (-1, 1):
                d = sgn * np.sqrt(float(thf[o]))
                px, py = f32(x0 + d * a[i] / nrm), f32(y0 + d * b[i] / nrm)
                for k in range(-4, 5):
                    qx, qy = px, py
                    for _ in range(abs(k)):
                        qx = np.nextafter(qx, f32(np.inf if k > 0 else -np.inf))
                        qy = np.nextafter(qy, f32(np.inf if k > 0 else -np.inf))
                    cands += [(qx, py), (px, qy)]
                    ths += [thf[o], thf[o]]
        xy2, th2 = np.array(cands, f32), np.array(ths, f32)
        acc = accepted(F, xy1, xy2, th2)
        own = acc[np.repeat(np.arange(len(xy1)), len(xy2) // len(xy1))[:len(xy2)], np.arange(len(xy2))]
        assert 0 < own.sum() < len(own)  # the walk straddles the threshold
        total += check(lib, F, xy1, xy2, th2)[1]
        # and one candidate per tile (a degenerate box: the corner values are the candidate's own num)
        for j in rng.integers(0, len(xy2), 40):
            check(lib, F, xy1, xy2[j:j + 1], th2[j:j + 1])
    assert total > 0

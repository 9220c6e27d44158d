"""Frame::UnprojectStereo on the host (csrc/unproject.c through orbamd.frame) against the pure-Python restatement
tests/unproject_py.py, bit for bit, and the argument checks of the three tracking entry points, which return before
any device is touched. No GPU."""
import ctypes as C

import numpy as np
import pytest

import orbamd
import undistort_py as U
import unproject_py as UP
from orbamd._lib import OrbmTrackGeom
from orbamd.frame import make_camera, track_geom, unproject_stereo

CAMS = sorted(U.CAMERAS)
E = -1  # ORBX_EARG


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def restated():
    """per camera: (camera, keypoints, depths, [(pose, restated pos, restated valid)]), computed once"""
    out = {}
    for name, (cam, cols, rows) in U.CAMERAS.items():
        kps, d = UP.test_inputs(cols, rows, cam, 120)
        out[name] = (cam, kps, d, [(T,) + UP.unproject_stereo(cam, T, kps, d) for T in UP.poses()])
    return out


@pytest.mark.parametrize("name", CAMS)
def test_host_equals_restatement_bitwise(restated, name):
    cam, kps, d, per_pose = restated[name]
    for z in (-1.0, 0.0, float(UP.DENORMAL), 1e6):  # the edge depths are among the inputs
        assert (d == np.float32(z)).any()
    assert len(per_pose) == 3 and np.array_equal(per_pose[0][0], np.eye(4, dtype=np.float32))
    for T, ref, rvalid in per_pose:
        pos, valid = unproject_stereo(cam.astuple(), T, kps, d)
        assert np.array_equal(bits(pos), bits(ref)) and np.array_equal(valid, rvalid)
        assert np.array_equal(valid != 0, d > 0) and (pos[valid == 0] == 0).all()
        assert 20 < int(valid.sum()) < len(kps)
    # the poses change the result: the comparison sees the pose arithmetic
    assert not np.array_equal(per_pose[0][1], per_pose[1][1]) and not np.array_equal(per_pose[1][1], per_pose[2][1])


@pytest.mark.parametrize("name", CAMS)
def test_identity_pose_is_the_camera_point(restated, name):
    """mRwc = I, mOw = 0: pos = ((u - cx) z invfx, (v - cy) z invfy, z) exactly"""
    cam, kps, d, _ = restated[name]
    pos, valid = unproject_stereo(cam.astuple(), np.eye(4), kps, d)
    f32 = np.float32
    with np.errstate(all="ignore"):
        x = (kps["x"] - f32(cam.cx)) * d * (f32(1) / f32(cam.fx))
        y = (kps["y"] - f32(cam.cy)) * d * (f32(1) / f32(cam.fy))
    ok = valid != 0
    assert ok.sum() > 20
    assert np.array_equal(pos[ok, 0], x[ok]) and np.array_equal(pos[ok, 1], y[ok]) and np.array_equal(pos[ok, 2], d[ok])
    assert pos[ok, 2].min() == UP.DENORMAL and pos[ok, 2].max() == f32(1e6)


def test_restatement_fixed_numbers():
    """a hand-computed point: fx = fy = 2, cx = cy = 1, a quarter turn about z and a translation"""
    class Cam:
        fx, fy, cx, cy = 2.0, 2.0, 1.0, 1.0
    T = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], np.float32)
    # Ow = -R^T t = (-2, 1, -3); x3Dc = ((5 - 1) * 4 / 2, (3 - 1) * 4 / 2, 4) = (8, 4, 4); Rwc x3Dc = (4, -8, 4)
    assert [float(v) for v in UP.camera_center(T)] == [-2.0, 1.0, -3.0]
    p = UP.unproject_one(Cam.fx, Cam.fy, Cam.cx, Cam.cy, T, UP.camera_center(T), 5.0, 3.0, 4.0)
    assert [float(v) for v in p] == [2.0, -7.0, 1.0]
    assert UP.unproject_one(Cam.fx, Cam.fy, Cam.cx, Cam.cy, T, UP.camera_center(T), 5.0, 3.0, 0.0) is None
    assert UP.unproject_one(Cam.fx, Cam.fy, Cam.cx, Cam.cy, T, UP.camera_center(T), 5.0, 3.0, np.nan) is None


def test_empty_and_optional_arguments():
    lib = orbamd.load()
    cam = make_camera(U.MY_YAML[0].astuple())
    T = np.eye(4, dtype=np.float32)
    assert lib.orbx_unproject_stereo(C.byref(cam), T.ctypes.data, 0, None, None, None, None) == 0
    pos, valid = unproject_stereo(cam, T, np.zeros(0, orbamd.kp_dtype), np.zeros(0, np.float32))
    assert pos.shape == (0, 3) and valid.shape == (0,)
    kps = np.zeros(3, orbamd.kp_dtype)
    d = np.ones(3, np.float32)
    pos = np.full((3, 3), 7, np.float32)
    assert lib.orbx_unproject_stereo(C.byref(cam), T.ctypes.data, 3, kps.ctypes.data, d.ctypes.data, pos.ctypes.data,
                                     None) == 0
    assert (pos[:, 2] == 1).all()


def test_unproject_bad_arguments_write_nothing():
    lib = orbamd.load()
    cam = make_camera(U.MY_YAML[0].astuple())
    T = np.eye(4, dtype=np.float32)
    kps = np.zeros(4, orbamd.kp_dtype)
    d = np.ones(4, np.float32)
    pos = np.full((4, 3), 7, np.float32)
    valid = np.full(4, 7, np.uint8)
    a = [C.byref(cam), T.ctypes.data, 4, kps.ctypes.data, d.ctypes.data, pos.ctypes.data, valid.ctypes.data]
    assert lib.orbx_unproject_stereo(*a) == 0
    pos[:], valid[:] = 7, 7
    for i in (0, 1, 3, 4, 5):
        b = list(a)
        b[i] = None
        assert lib.orbx_unproject_stereo(*b) == E, i
    b = list(a)
    b[2] = -1
    assert lib.orbx_unproject_stereo(*b) == E
    for k in ("fx", "fy"):
        bad = make_camera(U.MY_YAML[0].astuple())
        setattr(bad, k, 0.0)
        assert lib.orbx_unproject_stereo(C.byref(bad), *a[1:]) == E
    assert (pos == 7).all() and (valid == 7).all()


def test_unproject_batch_bad_arguments_need_no_device():
    lib = orbamd.load()
    cam = make_camera(U.MY_YAML[0].astuple())
    P = 0x1000  # never dereferenced: every call returns at its argument check
    good = [P, C.byref(cam), 2, P, P, P, 128, P, P, None, 9, None]
    fn = lib.orbx_unproject_stereo_batch_device
    for i in (0, 1, 3, 4, 5, 7, 8):
        b = list(good)
        b[i] = None
        assert fn(*b) == E, i
    for i, v in ((2, -1), (2, 65536), (6, 0), (3, P + 4)):
        b = list(good)
        b[i] = v
        assert fn(*b) == E, (i, v)
    for k in ("fx", "fy"):
        bad = make_camera(U.MY_YAML[0].astuple())
        setattr(bad, k, 0.0)
        b = list(good)
        b[1] = C.byref(bad)
        assert fn(*b) == E


def _geom(nlevels=8):
    s = np.float32(1.2) ** np.arange(nlevels, dtype=np.float32)
    return track_geom(700, 700, 320, 240, 40, 40 / 700, (0, 640, 0, 480), 0.1, 0.1, s)


def test_track_batch_bad_arguments_need_no_device():
    lib = orbamd.load()
    fn = lib.orbm_search_by_projection_last_frame_batch_device
    g = _geom()
    P = 0x1000
    good = [P, 3, P, P, 4, P, P, P, 128, None, None, P, P, P, C.byref(g), 7.0, 0, 1, P, P, None]
    for i in (0, 2, 3, 5, 6, 7, 11, 12, 13, 14, 18, 19):
        b = list(good)
        b[i] = None
        assert fn(*b) == E, i
    for i, v in ((1, -1), (4, 0), (8, 0), (8, 65537), (5, P + 4), (6, P + 8)):
        b = list(good)
        b[i] = v
        assert fn(*b) == E, (i, v)
    for nl in (0, -1, 17):
        bad = _geom()
        bad.nlevels = nl
        b = list(good)
        b[14] = C.byref(bad)
        assert fn(*b) == E, nl


def test_track_geom_fields():
    g = _geom(16)
    assert isinstance(g, OrbmTrackGeom) and C.sizeof(g) == 4 * (12 + 1 + 16)
    assert (g.min_x, g.max_x, g.min_y, g.max_y, g.nlevels) == (0.0, 640.0, 0.0, 480.0, 16)
    assert g.scale_factors[1] == np.float32(1.2)
    with pytest.raises(ValueError):
        track_geom(1, 1, 0, 0, 0, 0, (0, 1, 0, 1), 1, 1, np.ones(17))

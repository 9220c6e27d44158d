"""Frame::UndistortKeyPoints / ComputeImageBounds on the host (csrc/undistort.c through orbamd.frame) against the
pure-Python restatement tests/undistort_py.py, bit for bit, and the restatement against fixed numbers, the closed-form
forward model and its own iteration count. No GPU."""
import ctypes as C

import numpy as np
import pytest

import orbamd
import undistort_py as U
from orbamd._lib import OrbxCamera
from orbamd.frame import image_bounds, make_camera, undistort_keypoints, undistort_points

CAMS = sorted(U.CAMERAS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def restated():
    """per camera: (camera, cols, rows, test points, their restated undistortion), computed once"""
    out = {}
    for name, (cam, cols, rows) in U.CAMERAS.items():
        xy = U.test_points(cols, rows, cam)
        out[name] = (cam, cols, rows, xy, U.undistort_points(cam, xy))
    return out


@pytest.mark.parametrize("name", CAMS)
def test_host_points_equal_restatement_bitwise(restated, name):
    cam, cols, rows, xy, ref = restated[name]
    got = undistort_points(cam.astuple(), xy)
    assert len(xy) >= 504 and np.array_equal(bits(got), bits(ref))
    # in place
    buf = xy.copy()
    c = make_camera(cam.astuple())
    assert orbamd.load().orbx_undistort_points(C.byref(c), len(buf), buf.ctypes.data, buf.ctypes.data) == 0
    assert np.array_equal(bits(buf), bits(ref))


@pytest.mark.parametrize("name", CAMS)
def test_host_keypoints_equal_restatement_bitwise(restated, name):
    cam, cols, rows, xy, ref = restated[name]
    kps = U.test_keypoints(cols, rows, cam)
    got = undistort_keypoints(cam.astuple(), kps)
    want = U.undistort_keypoints(cam, kps)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(bits(np.stack([got["x"], got["y"]], 1)), bits(ref))
    for f in ("size", "angle", "response", "octave"):  # carried bit for bit
        assert got[f].tobytes() == kps[f].tobytes(), f
    assert not np.array_equal(got["x"], kps["x"])


@pytest.mark.parametrize("name", CAMS)
def test_host_bounds_equal_restatement_bitwise(name):
    cam, cols, rows = U.CAMERAS[name]
    b, gw, gh = image_bounds(cam.astuple(), cols, rows)
    rb, rgw, rgh = U.image_bounds(cam, cols, rows)
    assert np.array_equal(bits(b), bits(rb))
    assert bits(gw) == bits(rgw) and bits(gh) == bits(rgh)
    assert b[0] != 0 and b[1] != cols  # a distorted camera moves the bounds


def test_restatement_fixed_numbers():
    """the my.yaml corners and the principal point"""
    cam, cols, rows = U.MY_YAML
    want = [(-0.39748213, 0.19233076), (630.6768799, 4.67265034), (2.13527989, 475.63656616),
            (629.08099365, 472.30780029)]
    for (px, py), (wx, wy) in zip(((0, 0), (cols, 0), (0, rows), (cols, rows)), want):
        x, y = U.cv_undistort_point(cam, px, py)
        assert (x, y) == (np.float32(wx), np.float32(wy)), (px, py, x, y)
    for name, (cam, cols, rows) in U.CAMERAS.items():
        x, y = U.cv_undistort_point(cam, cam.cx, cam.cy)
        assert (x, y) == (np.float32(cam.cx), np.float32(cam.cy)), name
    b, gw, gh = U.image_bounds(*U.MY_YAML)
    assert np.array_equal(b, np.array([-0.39748213, 630.6768799, 0.19233076, 475.63656616], np.float32))


# the forward model takes the restated result back to the input: converged for my.yaml; TUM1 and EuRoC have not
# converged after five fixed iterations at the image corners, which is the reference's behaviour
ROUNDTRIP_PX = {"my": 1e-3, "tum1": 0.5, "euroc": 0.5}


@pytest.mark.parametrize("name", CAMS)
def test_restatement_inverts_forward_model(restated, name):
    """independent of the iteration: the closed-form distortion of the restated normalised point returns to the
    input pixel, over the corners, the principal point and the random points inside the image"""
    cam, cols, rows, xy, _ = restated[name]
    worst = 0.0
    for px, py in xy:
        if not (0 <= px <= cols and 0 <= py <= rows):
            continue
        x, y = U.normalized(cam, px, py)
        bx, by = U.distort_normalized(cam, x, y)
        worst = max(worst, abs(bx - float(px)), abs(by - float(py)))
    print("%s: forward-model round trip, worst %.3g px" % (name, worst))
    assert worst < ROUNDTRIP_PX[name]


@pytest.mark.parametrize("name", CAMS)
def test_iteration_count_is_observable(restated, name):
    """4 and 6 iterations each change the float output of at least one test point: the bit-exact comparisons above
    pin the count of five"""
    cam, cols, rows, xy, ref = restated[name]
    for iters in (4, 6):
        other = U.undistort_points(cam, xy, iters)
        changed = int((bits(other) != bits(ref)).any(axis=1).sum())
        print("%s: %d iterations change %d of %d points" % (name, iters, changed, len(xy)))
        assert changed >= 1


def test_k1_zero_copies_whatever_the_other_coefficients():
    cam, cols, rows = U.K1_ZERO
    assert cam.k2 != 0 and cam.p1 != 0 and cam.p2 != 0 and cam.k3 != 0
    kps = U.test_keypoints(cols, rows, cam)
    assert undistort_keypoints(cam.astuple(), kps).tobytes() == kps.tobytes()
    xy = U.test_points(cols, rows, cam)
    assert np.array_equal(bits(undistort_points(cam.astuple(), xy)), bits(xy))
    assert np.array_equal(bits(U.undistort_points(cam, xy)), bits(xy))
    b, gw, gh = image_bounds(cam.astuple(), cols, rows)
    assert b.tolist() == [0.0, float(cols), 0.0, float(rows)]
    assert gw == np.float32(64.0) / np.float32(cols) and gh == np.float32(48.0) / np.float32(rows)
    rb, rgw, rgh = U.image_bounds(cam, cols, rows)
    assert np.array_equal(bits(b), bits(rb)) and gw == rgw and gh == rgh


def test_bad_arguments():
    lib = orbamd.load()
    cam = make_camera(U.MY_YAML[0].astuple())
    xy = np.zeros((4, 2), np.float32)
    kps = np.zeros(4, orbamd.kp_dtype)
    b = np.zeros(4, np.float32)
    g = C.c_float()
    E = -1  # ORBX_EARG
    assert lib.orbx_undistort_points(None, 4, xy.ctypes.data, xy.ctypes.data) == E
    assert lib.orbx_undistort_points(C.byref(cam), -1, xy.ctypes.data, xy.ctypes.data) == E
    assert lib.orbx_undistort_points(C.byref(cam), 4, None, xy.ctypes.data) == E
    assert lib.orbx_undistort_points(C.byref(cam), 4, xy.ctypes.data, None) == E
    assert lib.orbx_undistort_keypoints(None, 4, kps.ctypes.data, kps.ctypes.data) == E
    assert lib.orbx_undistort_keypoints(C.byref(cam), -1, kps.ctypes.data, kps.ctypes.data) == E
    assert lib.orbx_undistort_keypoints(C.byref(cam), 4, None, kps.ctypes.data) == E
    assert lib.orbx_undistort_keypoints(C.byref(cam), 4, kps.ctypes.data, None) == E
    assert lib.orbx_image_bounds(None, 640, 480, b.ctypes.data, C.byref(g), C.byref(g)) == E
    assert lib.orbx_image_bounds(C.byref(cam), 640, 480, None, C.byref(g), C.byref(g)) == E
    for k in ("fx", "fy"):
        bad = make_camera(U.MY_YAML[0].astuple())
        setattr(bad, k, 0.0)
        assert lib.orbx_undistort_points(C.byref(bad), 4, xy.ctypes.data, xy.ctypes.data) == E
        assert lib.orbx_undistort_keypoints(C.byref(bad), 4, kps.ctypes.data, kps.ctypes.data) == E
        assert lib.orbx_image_bounds(C.byref(bad), 640, 480, b.ctypes.data, C.byref(g), C.byref(g)) == E
        assert lib.orbx_undistort_batch_device(None, C.byref(bad), 1, None, None, 1, None, None, None) == E
    # n == 0 needs no arrays; the grid inverses are optional
    assert lib.orbx_undistort_points(C.byref(cam), 0, None, None) == 0
    assert lib.orbx_undistort_keypoints(C.byref(cam), 0, None, None) == 0
    assert lib.orbx_image_bounds(C.byref(cam), 640, 480, b.ctypes.data, None, None) == 0
    assert isinstance(cam, OrbxCamera)

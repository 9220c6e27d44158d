"""The C++ drop-in Frame::UndistortKeyPoints / ComputeImageBounds (host/Frame_undistort_amd.{h,cc},
ORBextractor::SetCamera) builds with g++ against the C ABI and the test stand-in for OpenCV, and equals the vectors the
Python restatement wrote into tests/golden/undistort_vectors.txt: on the host, through the extractor overload's
device-less fallback, stand-alone under ASan + UBSan, and (GPU) through the extractor's own call."""
import os
import subprocess

import pytest

import undistort_py as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
FIXTURE = os.path.join(ROOT, "tests", "golden", U.FIXTURE)


@pytest.fixture(scope="module")
def built():
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp", "build_undistort.sh")])
    return BUILD


def run(exe, *args, env=None):
    r = subprocess.run([exe, FIXTURE, *args], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    return r


def test_fixture_is_the_restatement():
    """the committed vectors are what tests/undistort_py.py computes (python tests/undistort_py.py rewrites them)"""
    assert open(FIXTURE).read() == U.fixture_text()


def test_dropin_host_functions_and_deviceless_fallback(built):
    """ORBAMD_DEVICE=99 is out of range on any box: no handle, so the extractor overload runs on the host"""
    r = run(os.path.join(built, "test_undistort"), env=dict(os.environ, ORBAMD_DEVICE="99"))
    assert r.returncode == 0 and "ALL PASS" in r.stdout


def test_host_unit_under_asan_ubsan(built):
    r = run(os.path.join(built, "test_undistort_asan"))
    assert r.returncode == 0 and "ALL PASS" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr


@pytest.mark.gpu
def test_dropin_extractor_overload_on_gpu(built):
    env = dict(os.environ)
    env.pop("ORBAMD_DEVICE", None)
    r = run(os.path.join(built, "test_undistort"), "gpu", env=env)
    assert r.returncode == 0 and "ALL PASS" in r.stdout

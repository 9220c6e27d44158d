"""The C++ KeyFrameDatabase drop-in (host/KeyFrameDatabase.h, KeyFrameDatabase_amd.cc) builds with g++ against the
C ABI and its own mock KeyFrame / Frame (tests/cpp/kfdb/), and (GPU) returns the candidate vectors and writes the
mLoopScore / mRelocScore / word-count fields of the C++ restatement of KeyFrameDatabase.cc:40-309 embedded in
tests/cpp/kfdb/test_kfdb.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_kfdb")


def _build():
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp", "kfdb", "build_kfdb.sh")])


def test_kfdb_dropin_builds():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_kfdb_dropin_equals_restatement_on_gpu():
    _build()
    env = dict(os.environ)
    env.pop("ORBAMD_DEVICE", None)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASS" in r.stdout


def test_kfdb_dropin_does_not_throw_without_device():
    """ORBAMD_DEVICE=99 is out of range on any box: add stores nothing, both Detect* return no candidates, the
    status is logged to stderr, the process exits 0"""
    _build()
    env = dict(os.environ, ORBAMD_DEVICE="99")
    r = subprocess.run([BIN, "nodevice"], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASS" in r.stdout
    assert "orbslam_amd: orbdb_add failed (status -2, device)" in r.stderr

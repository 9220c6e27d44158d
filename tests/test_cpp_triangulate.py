"""The host unit of CreateNewMapPoints' per-match loop (csrc/triangulate.c) as a stand-alone C program over the vectors
the Python restatement wrote into tests/golden/triangulate_vectors.txt: built normally and under ASan + UBSan, run
directly. No GPU, no library."""
import os
import subprocess

import pytest

import triangulate_py as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
FIXTURE = os.path.join(ROOT, "tests", "golden", TP.FIXTURE)


@pytest.fixture(scope="module")
def built():
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp", "build_triangulate.sh")])
    return BUILD


def run(exe):
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-4000:])
    return r


def test_fixture_is_the_restatement():
    """the committed vectors are what tests/triangulate_py.py computes (python tests/triangulate_py.py rewrites
    them)"""
    assert open(FIXTURE).read() == TP.fixture_text()


def test_host_unit_over_the_fixture(built):
    r = run(os.path.join(built, "test_triangulate"))
    assert r.returncode == 0 and "ALL PASS" in r.stdout


def test_host_unit_under_asan_ubsan(built):
    r = run(os.path.join(built, "test_triangulate_asan"))
    assert r.returncode == 0 and "ALL PASS" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr

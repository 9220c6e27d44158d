"""The host unit of Optimizer::PoseOptimization (csrc/pose_optimize.c) as a stand-alone C program over the vectors the
Python restatement wrote into tests/golden/pose_vectors.txt: built normally and under ASan + UBSan, run directly; and
tools/check_so3_sincos.c on a reduced sample. No GPU, no library."""
import os
import re
import subprocess
import sys

import pytest

import pose_py as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
FIXTURE = os.path.join(ROOT, "tests", "golden", P.FIXTURE)


@pytest.fixture(scope="module")
def built():
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp", "build_pose_optimize.sh")])
    return BUILD


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-4000:])
    return r


def test_fixture_is_the_restatement():
    """the committed vectors are what tests/pose_py.py computes (python tests/pose_py.py rewrites them)"""
    assert open(FIXTURE).read() == P.fixture_text()


def test_host_unit_over_the_fixture(built):
    r = run(os.path.join(built, "test_pose_optimize"), FIXTURE)
    assert r.returncode == 0 and "ALL PASS" in r.stdout


def test_host_unit_under_asan_ubsan(built):
    r = run(os.path.join(built, "test_pose_optimize_asan"), FIXTURE)
    assert r.returncode == 0 and "ALL PASS" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr


def test_check_so3_sincos_runs(built):
    """the measuring tool builds, runs on a reduced sample and prints its figure; the figure is a record (DESIGN.md
    quotes the full run), not a gate"""
    r = run(os.path.join(built, "check_so3_sincos"), "200000")
    assert r.returncode == 0
    assert re.search(r"max ulp over the dense sample: ([0-9.]+)", r.stdout)


def test_generated_constants_are_the_headers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_so3_sincos.py"), "--check"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "pose_math.h: equal" in r.stdout, r.stdout

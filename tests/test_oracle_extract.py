"""The whole extractor restated in Python (tests/extract_py.py) vs the CPU oracle, stage by stage (no GPU).

For every directed case of tests/extract_cases.py, every size of the cell-geometry sweep and two synthetic frames:
pyramid levels, vToDistributeKeys, DistributeOctTree's output, every keypoint field as raw bits and every descriptor
byte agree; and every case takes the exit its name claims, read from the restatement's stats, so the GPU tests that run
the same images (tests/test_gpu_extract_cases.py) cannot pass on an image that misses its branch."""
import types

import numpy as np
import pytest

import extract_cases as X
import oracle_py
import orbamd
from extract_py import extract_py

CASES = X.all_cases()
_results = {}


def restated(case):
    """extract_py of a case, computed once and shared"""
    if case.name not in _results:
        k, d, st, stats = extract_py(case.image, *case.params)
        _results[case.name] = types.SimpleNamespace(kps=k, desc=d, stages=st, stats=stats)
    return _results[case.name]


def compare_with_oracle(r, image, params, what):
    orc = oracle_py.OracleExtractor(*params)
    ko, do = orc(image)
    for l in range(params[2]):
        assert orc.level_size(l) == r.stats["levels"][l]["size"], "%s: level %d size" % (what, l)
        np.testing.assert_array_equal(r.stages[l]["pyramid"], orc.pyramid(l), err_msg="%s: pyramid %d" % (what, l))
        for stage, got in (("candidates", orc.candidates(l)), ("octree", orc.octree(l))):
            exp = r.stages[l][stage]
            assert exp.shape == got.shape and np.array_equal(exp.view(np.uint32), got.view(np.uint32)), \
                "%s: level %d %s" % (what, l, stage)
    assert len(ko) == len(r.kps), "%s: %d keypoints vs oracle %d" % (what, len(r.kps), len(ko))
    for f in ("octave", "x", "y", "response", "size", "angle"):
        assert np.array_equal(r.kps[f].view(np.uint32), ko[f].view(np.uint32)), "%s: field %s" % (what, f)
    assert np.array_equal(r.desc, do), "%s: descriptors" % what
    return orc


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_restatement_equals_oracle_and_takes_its_exit(case):
    r = restated(case)
    case.expect(r)
    compare_with_oracle(r, case.image, case.params, case.name)


def test_fast_groups_with_the_oracle_scalar_and_vector_fast():
    """the FAST, fallback and NMS groups through both forms of the oracle's cv::FAST"""
    n = 0
    try:
        for simd in (False, True):
            oracle_py.set_fast_simd(simd)
            for case in CASES:
                if case.name.startswith(X.FAST_GROUP_PREFIXES):
                    compare_with_oracle(restated(case), case.image, case.params, "%s simd=%d" % (case.name, simd))
                    n += 1
    finally:
        oracle_py.set_fast_simd(True)
    assert n >= 150


@pytest.fixture(scope="module")
def sweep():
    out = {}
    for w, h in X.sweep_sizes():
        img = X.sweep_image(w, h)
        k, d, st, stats = extract_py(img, *X.SWEEP_PARAMS)
        out[(w, h)] = (img, types.SimpleNamespace(kps=k, desc=d, stages=st, stats=stats))
    return out


def test_sweep_restatement_equals_oracle(sweep):
    for (w, h), (img, r) in sweep.items():
        compare_with_oracle(r, img, X.SWEEP_PARAMS, "sweep %dx%d" % (w, h))
        assert len(r.kps) >= 4


def test_sweep_covers_the_cell_geometry(sweep):
    """what the sweep is for, from the stats: every residue of the cell width mod 4, clamped last cells, 1 to 4 octree
    roots, and all three height classes at every width. No size up to 140 px has a cell dropped by the
    iniX >= maxBorderX - 6 rule (:803) or a cell under 7 px: those need 26 cell columns or rows and have cases of their
    own (geo/dropped_last_column, geo/dropped_last_row, geo/zero_capacity_row)."""
    residues, clamped, dropped, nini = set(), 0, 0, set()
    for (w, h), (_, r) in sweep.items():
        lv = r.stats["levels"][0]
        nini.add(lv["nIni"])
        for c in lv["cells"]:
            if c["skipped"]:
                dropped += 1
            elif c["skipped"] is None:
                residues.add((c["rect"][2] - c["rect"][0]) % 4)
                clamped += c["clamped_x"] or c["clamped_y"]
                assert c["rect"][2] - c["rect"][0] >= 7 and c["rect"][3] - c["rect"][1] >= 7  # no zero-capacity cell
    assert residues == {0, 1, 2, 3} and clamped > 0 and dropped == 0 and nini == {1, 2, 3, 4}
    assert len(sweep) == 3 * 79 - 1  # 62 x 62 is both the smallest and the square


@pytest.mark.parametrize("agent,t", [(0, 0), (3, 11)])
def test_synthetic_frame_restatement_equals_oracle(agent, t):
    img = orbamd.synth_frames(agent, t, 1, 320, 240)[0]
    params = (500, 1.2, 5, 20, 7)
    k, d, st, stats = extract_py(img, *params)
    r = types.SimpleNamespace(kps=k, desc=d, stages=st, stats=stats)
    compare_with_oracle(r, img, params, "synthetic %d/%d" % (agent, t))
    assert len(k) > 400 and any(v["stop_at_n"] for v in stats["levels"])


def test_rejected_inputs_are_what_their_names_claim():
    """the shapes tests/test_gpu_extract_cases.py expects ORBX_EARG for, from the restated geometry (the oracle is not
    called: it divides by zero on the portrait shape)"""
    from extract_py import constructor_tables, level_sizes
    got = {}
    for name, w, h, params in X.REJECTED:
        sizes = level_sizes(w, h, constructor_tables(params[0], params[1], params[2])["inv_scale"])
        small = any(min(s) < 62 for s in sizes)
        roots = [int(np.floor(np.float32(s[0] - 32) / np.float32(s[1] - 32) + np.float32(0.5)))
                 for s in sizes if min(s) > 32]
        twice = any(a[0] == 2 * b[0] and a[1] == 2 * b[1] for a, b in zip(sizes, sizes[1:]))
        got[name] = (small, min(roots) == 0, twice)
    assert got == {"level_under_62": (True, False, False), "level1_under_62": (True, False, False),
                   "zero_roots_62x93": (False, True, False), "scale_exactly_2": (False, False, True)}

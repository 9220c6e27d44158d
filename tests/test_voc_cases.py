"""The hand-made vocabulary cases (voc_cases.py) on the CPU: the oracle (oracle/orb_oracle_voc.c) and the Python
restatement (voc_py.py) agree bit for bit on every case, every case reaches the edge it is built for (asserted from
the restatement's trace), four small cases are checked against literals derived by hand, and the module as a whole
reaches every trace flag."""
import struct

import numpy as np
import pytest

import oracle_py
import voc_cases as vc
import voc_py
from voc_py import L1_NORM, L2_NORM

_RESULTS = {}
_ORACLES = {}


def restated(case):
    if case.name not in _RESULTS:
        _RESULTS[case.name] = voc_py.transform_trace(*case.args(), case.feats, case.levelsup)
    return _RESULTS[case.name]


def oracle_of(case):
    key = case.launch_key()[:3]
    if key not in _ORACLES:
        _ORACLES[key] = oracle_py.OracleVocabulary(*case.args())
    return _ORACLES[key]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("case", vc.CASES, ids=lambda c: c.name)
def test_oracle_equals_restatement(case):
    r = restated(case)
    ov = oracle_of(case)
    (bw, bv), fv = ov.transform(case.feats, case.levelsup)
    np.testing.assert_array_equal(bw, r.bow[0])
    np.testing.assert_array_equal(bits(bv), bits(r.bow[1]))
    assert fv == r.fv
    word, weight, nid = ov.descend(case.feats, case.levelsup)
    np.testing.assert_array_equal(word, r.word)
    np.testing.assert_array_equal(bits(weight), bits(r.weight))
    np.testing.assert_array_equal(nid, r.nid)


@pytest.mark.parametrize("case", vc.CASES, ids=lambda c: c.name)
def test_case_reaches_its_edge(case):
    s = restated(case).summary()
    assert case.expect, "a case without an expectation proves nothing"
    for key, want in case.expect.items():
        if key == "flags":
            assert want <= s["flags"], (want, s["flags"])
        elif key == "order":
            continue  # test_order_cases_depend_on_order
        else:
            assert s[key] == want, (key, s[key], want)


def _seq(xs):
    t = 0.0
    for x in xs:
        t += x
    return t


def _pairs(xs):
    """adjacent pairs added first, then accumulated"""
    t = 0.0
    for i in range(0, len(xs) - 1, 2):
        t += xs[i] + xs[i + 1]
    if len(xs) % 2:
        t += xs[-1]
    return t


@pytest.mark.parametrize("case", [c for c in vc.CASES if "order" in c.expect], ids=lambda c: c.name)
def test_order_cases_depend_on_order(case):
    """the sum the case pins changes bits when run in reverse and when run pairwise: another order would show"""
    r = restated(case)
    if case.expect["order"] == "word":
        xs = max(r.word_addends.values(), key=len)
        assert _seq(xs) / r.nwords == r.bow[1][0]
    else:
        xs = [abs(v) for v in r.norm_addends]
        assert _seq(xs) == r.norm
    fwd, rev, pw = _seq(xs), _seq(xs[::-1]), _pairs(xs)
    assert min(xs) <= 1e-8 * 1.0001 and max(xs) >= 1e8
    assert bits([fwd])[0] != bits([rev])[0]
    assert bits([fwd])[0] != bits([pw])[0]


def test_big_sums_depend_on_order():
    """the 4096-word norm and the 4096-feature word (the kernel's longest chains) also change bits pairwise"""
    r = restated(vc.BY_NAME["own_word_4096_features"])
    xs = [abs(v) for v in r.norm_addends]
    assert bits([_seq(xs)])[0] != bits([_pairs(xs)])[0]
    r = restated(vc.BY_NAME["one_word_4096_features"])
    xs = r.word_addends[0]
    assert len(xs) == 4096 and bits([_seq(xs)])[0] != bits([_pairs(xs)])[0]


def test_every_trace_flag_is_reached():
    reached = set()
    for c in vc.CASES:
        reached |= restated(c).flags()
    assert reached == set(voc_py.FLAGS), set(voc_py.FLAGS) - reached


def test_listed_shapes_are_all_present():
    names = set(vc.BY_NAME)
    for nw in vc.WORD_COUNTS:
        for sc in (L1_NORM, L2_NORM):
            assert restated(vc.BY_NAME["word_count_%d_scoring_%d" % (nw, sc)]).nwords == nw
    for m in vc.KEPT_COUNTS:
        assert restated(vc.BY_NAME["kept_%d_interleaved_stopped" % m]).kept == m
    assert len([n for n in names if n.startswith("scoring_")]) == 24
    assert len([n for n in names if n.startswith("levelsup_")]) == 6
    nc = {x for row in restated(vc.BY_NAME["child_counts_1_to_33"]).summary()["nc"] for x in row[1:]}
    assert nc == set(vc.CHILD_COUNTS)
    groups = vc.launches()
    assert sorted(c.name for g in groups for c in g) == sorted(names)


# ---- literals derived by hand: these rest on no implementation at all
def _run_all(case):
    """[(bow words, bow value bits, fv)] of the restatement and the oracle"""
    r = restated(case)
    (bw, bv), fv = oracle_of(case).transform(case.feats, case.levelsup)
    return [(r.bow[0].tolist(), bits(r.bow[1]).tolist(), r.fv), (bw.tolist(), bits(bv).tolist(), fv)]


def _rows(case):
    """[(per-feature words, weight bits, node ids)] of the restatement and the oracle"""
    r = restated(case)
    word, weight, nid = oracle_of(case).descend(case.feats, case.levelsup)
    return [(r.word.tolist(), bits(r.weight).tolist(), r.nid.tolist()),
            (word.tolist(), bits(weight).tolist(), nid.tolist())]


def _b(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_literal_duplicate_children():
    # L = 1, children 0 and 1 of the root identical (nodes 1 and 2, words 0 and 1, weights 1.0 and 2.0), child 2
    # random. The `d < best_d` scan keeps the first of the two: node 1, word 0, weight 1.0. TF_IDF: v[0] = 1.0;
    # L1 norm = 1.0; 1.0 / 1.0 = 1.0. levelsup 0: the FeatureVector key is the node at level 1 - 0 = 1: node 1.
    for words, vals, fv in _run_all(vc.BY_NAME["dup_children_0_1"]):
        assert words == [0] and vals == [_b(1.0)] and fv == {1: [0]}
    for word, weight, nid in _rows(vc.BY_NAME["dup_children_0_1"]):
        assert word == [0] and weight == [_b(1.0)] and nid == [1]


def test_literal_stopped_word():
    # L = 1, words 0..4 with weights 1.5, 0.0, -0.0, -2.0, NaN; queries at words 0, 1, 2, 3, 4, 0, 4. `w > 0` holds
    # for word 0 alone: features 0 and 5. TF_IDF: v[0] = 1.5 + 1.5 = 3.0; L1 norm 3.0; 3.0 / 3.0 = 1.0. levelsup 0:
    # key = node 1 (word 0's node). Stopped features enter neither vector.
    for words, vals, fv in _run_all(vc.BY_NAME["stopped_by_zero_negzero_negative_nan"]):
        assert words == [0] and vals == [_b(1.0)] and fv == {1: [0, 5]}
    nan = float("nan")
    for word, weight, nid in _rows(vc.BY_NAME["stopped_by_zero_negzero_negative_nan"]):  # words 0..4 are nodes 1..5
        assert word == [0, 1, 2, 3, 4, 0, 4] and nid == [1, 2, 3, 4, 5, 1, 5]
        assert weight == [_b(x) for x in (1.5, 0.0, -0.0, -2.0, nan, 1.5, nan)]


def test_literal_l2_underflow():
    # L = 1, words 0..2 with weights 1e-200, 2e-200, 3e-200; queries at words 0, 1, 0, 2. TF_IDF: v = (1e-200 +
    # 1e-200, 2e-200, 3e-200) = (2e-200, 2e-200, 3e-200) (a doubling is exact). L2: every square is below 1e-399,
    # far under the smallest subnormal 4.9e-324, so each rounds to 0, the sum is 0, sqrt(0) = 0, and `norm > 0.0`
    # is false: the values stay as they are. levelsup 0: keys = nodes 1, 2, 3.
    for words, vals, fv in _run_all(vc.BY_NAME["l2_weights_1e-200"]):
        assert words == [0, 1, 2] and vals == [_b(2e-200), _b(2e-200), _b(3e-200)]
        assert fv == {1: [0, 2], 2: [1], 3: [3]}
    for word, weight, nid in _rows(vc.BY_NAME["l2_weights_1e-200"]):
        assert word == [0, 1, 0, 2] and nid == [1, 2, 1, 3]
        assert weight == [_b(x) for x in (1e-200, 2e-200, 1e-200, 3e-200)]


def test_literal_dot_tf_division():
    # L = 1, words 0..2 with weights 0.5, 0.25, 3.0; queries at words 0, 0, 1. TF: v = (0.5 + 0.5, 0.25) = (1.0,
    # 0.25); DOT_PRODUCT does not normalise, so each value is divided by the number of words in the vector, 2 (not
    # by the 3 features): (0.5, 0.125), all exact in binary. levelsup 0: keys = nodes 1 and 2.
    for words, vals, fv in _run_all(vc.BY_NAME["dot_product_tf"]):
        assert words == [0, 1] and vals == [_b(0.5), _b(0.125)] and fv == {1: [0, 1], 2: [2]}
    for word, weight, nid in _rows(vc.BY_NAME["dot_product_tf"]):
        assert word == [0, 0, 1] and weight == [_b(0.5), _b(0.5), _b(0.25)] and nid == [1, 1, 2]
    # IDF: addIfNotExist keeps the first weight and nothing is divided: (0.5, 0.25)
    for words, vals, fv in _run_all(vc.BY_NAME["dot_product_idf"]):
        assert words == [0, 1] and vals == [_b(0.5), _b(0.25)] and fv == {1: [0, 1], 2: [2]}

"""The hand-made vocabulary cases (voc_cases.py) on the GPU: k_voc_descend + k_voc_bow behind orbv_transform (host
API) and orbv_transform_batch_device (the cases of one vocabulary as frames of one launch) against the oracle, every
comparison on raw bits; a sentinel guard that a frame's outputs stay inside its own rows; batch shapes, buffer re-use,
the count clamp and the text loader. Whether each case reaches its edge is asserted on the CPU (test_voc_cases.py)."""
import numpy as np
import pytest

import oracle_py
import orbamd
import voc_cases as vc
from orbamd.vocabulary import to_text
from voc_py import L1_NORM, TF_IDF

pytestmark = pytest.mark.gpu

SENT32 = 0x5A5A5A5A
SENT64 = 0x7FF85A5A5A5A5A5A  # a NaN no sum produces
_HANDLES, _ORACLES = {}, {}


def handles(case):
    """(device vocabulary, oracle vocabulary) of the case, one pair per (vocabulary, scoring, weighting)"""
    key = case.launch_key()[:3]
    if key not in _HANDLES:
        _HANDLES[key] = orbamd.ORBVocabulary.from_arrays(*case.args())
        _ORACLES[key] = oracle_py.OracleVocabulary(*case.args())
    return _HANDLES[key], _ORACLES[key]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_transform_equal(got, want, msg=""):
    (bw, bv), fv = got
    (bw2, bv2), fv2 = want
    np.testing.assert_array_equal(bw, bw2, err_msg=msg)
    np.testing.assert_array_equal(bits(bv), bits(bv2), err_msg=msg)
    assert fv == fv2, msg


class Buffers:
    """the output tensors of one batch launch, pre-filled with sentinels"""

    def __init__(self, B, S):
        import torch
        self.torch, self.B, self.S = torch, B, S
        self.dev = torch.device("cuda", 0)
        i32 = lambda *s: torch.full(s, SENT32, dtype=torch.int32, device=self.dev)  # noqa: E731
        i64 = lambda *s: torch.full(s, SENT64, dtype=torch.int64, device=self.dev)  # noqa: E731
        self.word, self.weight, self.nid = i32(B, S), i64(B, S), i32(B, S)
        self.bw, self.bv, self.nb = i32(B, S), i64(B, S), i32(B)
        self.fn, self.fo, self.ff, self.nf = i32(B, S), i32(B, S + 1), i32(B, S), i32(B)

    def launch(self, gv, frames, counts, levelsup):
        """frames[f]: the descriptor rows of frame f (at most S); counts[f]: what d_counts holds for it"""
        torch, B, S = self.torch, self.B, self.S
        assert len(frames) == len(counts) == B
        host = np.zeros((B, S, 32), np.uint8)
        for f, d in enumerate(frames):
            assert len(d) <= S
            host[f, :len(d)] = d
        dd = torch.from_numpy(host).to(self.dev)
        dc = torch.from_numpy(np.array(counts, np.int32)).to(self.dev)
        st = torch.cuda.current_stream(self.dev).cuda_stream
        rc = orbamd.load().orbv_transform_batch_device(
            gv._h, B, dd.data_ptr(), dc.data_ptr(), S, levelsup, self.word.data_ptr(), self.weight.data_ptr(),
            self.nid.data_ptr(), self.bw.data_ptr(), self.bv.data_ptr(), self.nb.data_ptr(), self.fn.data_ptr(),
            self.fo.data_ptr(), self.ff.data_ptr(), self.nf.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("word", "weight", "nid", "bw", "bv", "nb", "fn", "fo", "ff",
                                                             "nf")}


def check_frame(out, f, desc, ov, levelsup, sentinels=True, msg=""):
    """frame f of a launch's outputs against the oracle on `desc`: every row holds its result, then untouched sentinel"""
    msg = "%s frame %d" % (msg, f)
    c = len(desc)
    (bw, bv), fv = ov.transform(desc, levelsup)
    word, weight, nid = ov.descend(desc, levelsup)
    np.testing.assert_array_equal(out["word"][f, :c], word, err_msg=msg)
    np.testing.assert_array_equal(out["weight"][f, :c].view(np.uint64), bits(weight), err_msg=msg)
    np.testing.assert_array_equal(out["nid"][f, :c], nid, err_msg=msg)
    nb, nf = int(out["nb"][f]), int(out["nf"][f])
    assert nb == len(bw) and nf == len(fv), (msg, nb, len(bw), nf, len(fv))
    np.testing.assert_array_equal(out["bw"][f, :nb].view(np.uint32), bw, err_msg=msg)
    np.testing.assert_array_equal(out["bv"][f, :nb].view(np.uint64), bits(bv), err_msg=msg)
    nodes = sorted(fv)
    offs = np.cumsum([0] + [len(fv[k]) for k in nodes])
    feats = [i for k in nodes for i in fv[k]]
    np.testing.assert_array_equal(out["fn"][f, :nf].view(np.uint32), np.array(nodes, np.uint32), err_msg=msg)
    np.testing.assert_array_equal(out["fo"][f, :nf + 1], offs, err_msg=msg)  # fv_off of frame f at f * (stride + 1)
    np.testing.assert_array_equal(out["ff"][f, :len(feats)], feats, err_msg=msg)
    if sentinels:
        for k, used in (("word", c), ("nid", c), ("bw", nb), ("fn", nf), ("fo", nf + 1), ("ff", len(feats))):
            assert (out[k][f, used:] == SENT32).all(), (msg, k, "written past its %d entries" % used)
        for k, used in (("weight", c), ("bv", nb)):
            assert (out[k][f, used:] == SENT64).all(), (msg, k, "written past its %d entries" % used)


# ---------------------------------------------------------------------------------------------------------- host API
@pytest.mark.parametrize("case", vc.CASES, ids=lambda c: c.name)
def test_host_transform_equals_oracle(case):
    gv, ov = handles(case)
    assert_transform_equal(gv.transform(case.feats, case.levelsup), ov.transform(case.feats, case.levelsup), case.name)


# ------------------------------------------------------------------------------------------------------- batch entry
@pytest.mark.parametrize("group", vc.launches(), ids=lambda g: g[0].name)
def test_batch_cases_equal_oracle_inside_their_rows(group):
    pytest.importorskip("torch")
    gv, ov = handles(group[0])
    S = max(max(c.n for c in group), 1)
    out = Buffers(len(group), S).launch(gv, [c.feats for c in group], [c.n for c in group], group[0].levelsup)
    for f, c in enumerate(group):
        check_frame(out, f, c.feats, ov, c.levelsup, msg=c.name)


def _stop_voc():
    case = vc.BY_NAME["kept_129_interleaved_stopped"]
    gv, ov = handles(case)
    return case, gv, ov, np.array(vc._stopv()[1], np.uint8)


def _queries(leaves, n, seed):
    """n queries: leaves with up to 3 flipped bits, repeats among them"""
    g = np.random.default_rng([400407, seed])
    idx = g.integers(0, max(min(len(leaves), 2 * n // 3), 1), n)
    return np.array([vc.flipn(g, leaves[i], int(g.integers(0, 4))) for i in idx], np.uint8).reshape(n, 32)


def test_batch_stride_100_small_counts():
    pytest.importorskip("torch")
    case, gv, ov, leaves = _stop_voc()
    counts = [0, 100, 1, 15, 16, 17, 37]
    frames = [_queries(leaves, n, 10 + f) for f, n in enumerate(counts)]
    out = Buffers(len(counts), 100).launch(gv, frames, counts, 1)
    for f, d in enumerate(frames):
        check_frame(out, f, d, ov, 1)


def test_batch_stride_4096_full_frame_beside_small_ones():
    pytest.importorskip("torch")
    case = vc.BY_NAME["own_word_4096_features"]
    gv, ov = handles(case)
    leaves = vc._big()[1]
    counts = [4096, 3, 0, 129]
    frames = [_queries(leaves, n, 20 + f) for f, n in enumerate(counts)]
    out = Buffers(len(counts), 4096).launch(gv, frames, counts, 1)
    for f, d in enumerate(frames):
        check_frame(out, f, d, ov, 1)


def test_empty_vocabulary_on_both_entries():
    """a root without children: TemplatedVocabulary::empty(), both vectors empty; the per-feature rows hold the root's
    Node() defaults (word 0, weight 0.0, node 0)"""
    pytest.importorskip("torch")
    none = (np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros((0, 32), np.uint8), np.zeros(0, np.float64))
    gv = orbamd.ORBVocabulary.from_arrays(10, 6, L1_NORM, TF_IDF, *none)
    ov = oracle_py.OracleVocabulary(10, 6, L1_NORM, TF_IDF, *none)
    assert gv.info()["nodes"] == 1 and gv.info()["words"] == 0
    d = _queries(vc._big()[1], 37, 30)
    (bw, bv), fv = gv.transform(d, 4)
    assert len(bw) == 0 and len(bv) == 0 and fv == {}
    assert_transform_equal(gv.transform(d, 4), ov.transform(d, 4))
    counts = [37, 0, 5]
    frames = [d, d[:0], d[:5]]
    out = Buffers(3, 40).launch(gv, frames, counts, 4)
    for f, x in enumerate(frames):
        check_frame(out, f, x, ov, 4)
        assert out["nb"][f] == 0 and out["nf"][f] == 0 and out["fo"][f, 0] == 0
        assert (out["word"][f, :len(x)] == 0).all() and (out["nid"][f, :len(x)] == 0).all()
        assert (out["weight"][f, :len(x)].view(np.uint64) == 0).all()


def test_batch_buffers_reused_with_smaller_counts():
    pytest.importorskip("torch")
    case, gv, ov, leaves = _stop_voc()
    first, second = [100, 64, 37, 17], [5, 0, 36, 3]
    frames = [_queries(leaves, n, 40 + f) for f, n in enumerate(first)]
    buf = Buffers(4, 100)
    out = buf.launch(gv, frames, first, 1)
    for f, d in enumerate(frames):
        check_frame(out, f, d, ov, 1)
    frames2 = [_queries(leaves, n, 50 + f) for f, n in enumerate(second)]
    again = buf.launch(gv, frames2, second, 1)
    fresh = Buffers(4, 100).launch(gv, frames2, second, 1)
    for f, d in enumerate(frames2):
        check_frame(again, f, d, ov, 1, sentinels=False)
        check_frame(fresh, f, d, ov, 1)
        c, nb, nf = len(d), int(fresh["nb"][f]), int(fresh["nf"][f])
        assert again["nb"][f] == nb and again["nf"][f] == nf
        for k, used in (("word", c), ("weight", c), ("nid", c), ("bw", nb), ("bv", nb), ("fn", nf), ("fo", nf + 1),
                        ("ff", int(fresh["fo"][f, nf]))):
            assert again[k][f, :used].tobytes() == fresh[k][f, :used].tobytes(), (f, k)


def test_batch_count_is_clamped_to_the_stride():
    """d_counts[f] is read as min(max(count, 0), stride): 69 at stride 64 transforms the frame's 64 rows and touches
    nothing of the next frame, -3 is an empty frame. (The over-count frame is not the last and 69 <= 128, the sort's
    block: code without the clamp would stay inside the launch's buffers as well.)"""
    pytest.importorskip("torch")
    case, gv, ov, leaves = _stop_voc()
    counts = [10, 69, -3, 64, 5]
    rows = [10, 64, 64, 64, 5]
    frames = [_queries(leaves, n, 60 + f) for f, n in enumerate(rows)]
    out = Buffers(len(counts), 64).launch(gv, frames, counts, 1)
    check_frame(out, 0, frames[0], ov, 1, msg="neighbour")
    check_frame(out, 1, frames[1], ov, 1, msg="count 69 at stride 64")
    check_frame(out, 2, frames[2][:0], ov, 1, msg="count -3")
    assert out["nb"][2] == 0 and out["nf"][2] == 0 and out["fo"][2, 0] == 0
    check_frame(out, 3, frames[3], ov, 1, msg="neighbour")
    check_frame(out, 4, frames[4], ov, 1, msg="neighbour")


# ------------------------------------------------------------------------------------------------------------ loader
def _write_text(path, k, L, scoring, weighting, parent, leaf, desc, weight, eol="\n", fmt=repr, blank_every=0,
                trailing=0):
    with open(path, "w", newline="") as f:
        f.write("%d %d %d %d%s" % (k, L, scoring, weighting, eol))
        for i, (p, lf, d, w) in enumerate(zip(parent, leaf, desc, weight)):
            if blank_every and i % blank_every == 0:
                f.write((" \t" if i % 2 else "") + eol)
            f.write("%d %d %s %s%s" % (p, lf, " ".join(str(int(x)) for x in d), fmt(float(w)), eol))
        f.write(eol * trailing)


TEXT_FORMS = {
    "crlf": dict(eol="\r\n"),
    "blank_lines": dict(blank_every=7, trailing=3),
    "crlf_blank_lines": dict(eol="\r\n", blank_every=5, trailing=2),
    "17_digits": dict(fmt=lambda w: "%.17g" % w),
    "exponent": dict(fmt=lambda w: "%.16e" % w),
    "exponent_upper_crlf": dict(fmt=lambda w: "%.16E" % w, eol="\r\n", trailing=1),
}


@pytest.mark.parametrize("form", sorted(TEXT_FORMS))
def test_loader_text_forms_equal_arrays(form, tmp_path):
    case, gv, ov, leaves = _stop_voc()
    args = case.args()
    for w in args[7]:
        assert float("%.17g" % w) == w and float("%.16e" % w) == w
    path = tmp_path / "voc.txt"
    _write_text(path, *args, **TEXT_FORMS[form])
    tv = orbamd.ORBVocabulary(path)
    assert tv.info() == gv.info()
    d = _queries(leaves, 200, 70)
    want = ov.transform(d, 1)
    assert_transform_equal(gv.transform(d, 1), want, "arrays")
    assert_transform_equal(tv.transform(d, 1), want, form)


def test_loader_written_by_to_text_equals_arrays(tmp_path):
    case, gv, ov, leaves = _stop_voc()
    k, L, sc, wt, parent, leaf, desc, weight = case.args()
    path = tmp_path / "voc.txt"
    to_text(path, k, L, parent, leaf, desc, weight, scoring=sc, weighting=wt)
    d = _queries(leaves, 200, 71)
    assert_transform_equal(orbamd.ORBVocabulary(path).transform(d, 1), ov.transform(d, 1))


def _node_line(parent, nfields=35):
    return " ".join(([str(parent), "1"] + ["7"] * 32 + ["1.5"])[:nfields])


BAD_TEXTS = {
    "too_few_fields": "3 2 0 0\n" + _node_line(0) + "\n" + _node_line(0, 34) + "\n",
    "no_descriptor": "3 2 0 0\n0 1\n",
    "parent_equals_own_id": "3 2 0 0\n" + _node_line(0) + "\n" + _node_line(2) + "\n",
    "parent_above_own_id": "3 2 0 0\n" + _node_line(5) + "\n",
    "parent_negative": "3 2 0 0\n" + _node_line(-1) + "\n",
    "k_21": "21 2 0 0\n" + _node_line(0) + "\n",
    "k_negative": "-1 2 0 0\n" + _node_line(0) + "\n",
    "L_0": "3 0 0 0\n" + _node_line(0) + "\n",
    "L_11": "3 11 0 0\n" + _node_line(0) + "\n",
    "scoring_6": "3 2 6 0\n" + _node_line(0) + "\n",
    "weighting_4": "3 2 0 4\n" + _node_line(0) + "\n",
    "header_short": "3 2 0\n" + _node_line(0) + "\n",
}


@pytest.mark.parametrize("name", sorted(BAD_TEXTS))
def test_loader_rejects_bad_text(name, tmp_path):
    import ctypes as C
    from orbamd._lib import ORBX_EARG
    lib = orbamd.load()
    good = tmp_path / "good.txt"
    good.write_text("3 2 0 0\n" + _node_line(0) + "\n" + _node_line(1) + "\n")
    h = C.c_void_p()
    assert lib.orbv_load_text(str(good).encode(), 0, C.byref(h)) == 0  # the lines the bad files are made of load
    lib.orbv_destroy(h)
    path = tmp_path / "bad.txt"
    path.write_text(BAD_TEXTS[name])
    h = C.c_void_p()
    assert lib.orbv_load_text(str(path).encode(), 0, C.byref(h)) == ORBX_EARG
    assert not h.value

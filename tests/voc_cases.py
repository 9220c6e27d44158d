"""Hand-made vocabularies and queries for the DBoW2 transform (TemplatedVocabulary<FORB>::transform): one case per
exit of the algorithm and per layout edge of the kernels that run it.

A vocabulary is arrays of node lines in file order (parent, isLeaf, descriptor, weight; node ids = line order, root
= 0). A descriptor at Hamming distance h from another is that one with h chosen bits flipped. A Case holds the
vocabulary, (scoring, weighting, levelsup), the query descriptors and `expect`: values the restatement's trace
(voc_py.Result.summary()) must show for the edge the case is built to reach -- asserted on the CPU from the restatement
only (test_voc_cases.py), never from the code under test. Cases sharing one Voc object and one (scoring, weighting,
levelsup) are frames of one batch launch in test_gpu_voc_cases.py.

Everything is inside the domain: finite weights, or NaN only as a stopped word; no infinite weight; n <= 4096.
"""
import zlib

import numpy as np

from voc_py import (L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT, TF_IDF, TF, IDF, BINARY, _POP)

SCORINGS = (L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT)
WEIGHTINGS = (TF_IDF, TF, IDF, BINARY)
WORD_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025)
KEPT_COUNTS = (0, 1, 127, 128, 129)
CHILD_COUNTS = (1, 2, 15, 16, 17, 20, 33)
LEVELSUPS = (-1, 0, 1, 9, 10, 13)  # on the L = 10 tree: -1, 0, 1, L - 1, L, L + 3


def _rng(name):
    return np.random.default_rng([400407, zlib.crc32(name.encode())])


def rdesc(g):
    return g.integers(0, 256, 32).astype(np.uint8)


def flip(d, bits):
    d = np.array(d, np.uint8)
    for p in bits:
        d[p >> 3] ^= np.uint8(1 << (p & 7))
    return d


def flipn(g, d, h):
    return flip(d, g.permutation(256)[:h])


def ham(a, b):
    return int(_POP[np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)].sum())


def near(g, d, h=2):
    """a query at distance h from d, the flips inside bits 240..255 (which kid() never touches)"""
    return flip(d, 240 + g.permutation(16)[:h])


def kid(d, depth, c, width=12, per_level=48):
    """child c of a node at `depth` (root = 0): the parent's descriptor with `width` bits of the level's own range
    flipped, so a node is at distance width * (levels apart) from its ancestors and 2 * width from a sibling"""
    lo = depth * per_level + c * width
    assert lo + width <= 240 and (c + 1) * width <= per_level
    return flip(d, range(lo, lo + width))


class Voc:
    def __init__(self, k, L):
        self.k, self.L = k, L
        self.parent, self.leaf, self.desc, self.weight = [], [], [], []
        self._arr = None

    def add(self, parent, d, w=1.0, leaf=0):
        assert self._arr is None and 0 <= parent <= len(self.parent)
        self.parent.append(int(parent))
        self.leaf.append(int(leaf))
        self.desc.append(np.asarray(d, np.uint8))
        self.weight.append(float(w))
        return len(self.parent)  # node id

    def arrays(self):
        if self._arr is None:
            n = len(self.parent)
            self._arr = (np.array(self.parent, np.int32), np.array(self.leaf, np.uint8),
                         np.array(self.desc, np.uint8).reshape(n, 32), np.array(self.weight, np.float64))
        return self._arr


class Case:
    def __init__(self, name, group, voc, feats, expect, scoring=L1_NORM, weighting=TF_IDF, levelsup=0):
        self.name, self.group, self.voc, self.expect = name, group, voc, expect
        self.scoring, self.weighting, self.levelsup = scoring, weighting, levelsup
        self.feats = np.array(feats, np.uint8).reshape(-1, 32)
        assert len(self.feats) <= 4096
        w = np.array(voc.weight, np.float64)
        assert not np.isinf(w).any()

    @property
    def n(self):
        return len(self.feats)

    def args(self):
        """(k, L, scoring, weighting, parent, is_leaf, desc, weight): the arguments of the three implementations"""
        return (self.voc.k, self.voc.L, self.scoring, self.weighting) + self.voc.arrays()

    def launch_key(self):
        return (id(self.voc), self.scoring, self.weighting, self.levelsup)

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------- descent
def _dup(a, b):
    """children a and b identical (distance 10 from the query), every other child random: the first in file order"""
    name = "dup_children_%d_%d" % (a, b)
    g = _rng(name)
    q = rdesc(g)
    twin = flipn(g, q, 10)
    v = Voc(20, 1)
    for j in range(max(b + 1, 3)):
        d = twin if j in (a, b) else rdesc(g)
        assert j in (a, b) or ham(d, q) > 10
        v.add(0, d, w=1.0 + j, leaf=1)
    flags = set()
    if b >= 16:
        flags.add("trip2")
    if a % 16 == b % 16:
        flags.add("tie_congruent")
    if a % 16 > b % 16:
        flags.add("tie_cross")
    return Case(name, "descent", v, [q], {"winner": [[a]], "nties": [[2]], "word": [a], "nid": [a + 1], "depth": [1],
                                          "flags": flags})


def _all_256():
    g = _rng("all_256")
    q = rdesc(g)
    v = Voc(20, 1)
    for j in range(17):
        v.add(0, ~q, w=0.5 + j, leaf=1)
    return Case("all_children_at_256", "descent", v, [q],
                {"winner": [[0]], "nties": [[17]], "word": [0], "flags": {"trip2", "tie_congruent"}})


def _dist_0():
    g = _rng("dist_0")
    q = rdesc(g)
    v = Voc(4, 1)
    for j in range(4):
        v.add(0, q if j == 2 else flipn(g, q, 1 + j), w=1.0 + j, leaf=1)
    return Case("child_at_distance_0", "descent", v, [q], {"winner": [[2]], "nties": [[1]], "word": [2]})


def _fanout():
    """interior nodes of 1, 2, 15, 16, 17, 20 and 33 children under a declared k of 20; a query at the first and at
    the last child of each"""
    g = _rng("fanout")
    v = Voc(20, 2)
    tops = [rdesc(g) for _ in CHILD_COUNTS]
    for d in tops:
        v.add(0, d)
    feats, winner, word, nc = [], [], [], []
    w0 = 0
    for i, cnt in enumerate(CHILD_COUNTS):
        leaves = [flipn(g, tops[i], 40) for _ in range(cnt)]
        for d in leaves:
            v.add(i + 1, d, w=float(g.uniform(0.1, 8.0)), leaf=1)
        for j in sorted({0, cnt - 1}):
            feats.append(flipn(g, leaves[j], 3))
            winner.append([i, j])
            word.append(w0 + j)
            nc.append([len(CHILD_COUNTS), cnt])
        w0 += cnt
    return Case("child_counts_1_to_33", "descent", v, feats,
                {"winner": winner, "word": word, "nc": nc, "nties": [[1, 1]] * len(feats),
                 "flags": {"trip2", "trip3"}}, levelsup=1)


def _l1():
    g = _rng("L1")
    v = Voc(3, 1)
    leaves = [rdesc(g) for _ in range(3)]
    for j, d in enumerate(leaves):
        v.add(0, d, w=0.5 * (j + 1), leaf=1)
    return Case("L1_words_under_root", "descent", v, [near(g, leaves[j]) for j in (2, 0, 1)],
                {"word": [2, 0, 1], "depth": [1, 1, 1], "nid": [0, 0, 0]}, levelsup=4)


_DEEP = None
DEEP_PATHS = (0, 1023, 0b1010101010, 0b0101010101, 1, 512)


def _deep():
    """the full binary tree of depth 10 in breadth-first file order: node of depth d and path p (d bits) has id
    2^d - 1 + p, leaf p is word p"""
    global _DEEP
    if _DEEP is None:
        g = _rng("deep")
        v = Voc(2, 10)
        level = [(0, rdesc(g))]
        for depth in range(10):
            nxt = []
            for pid, pd in level:
                for c in range(2):
                    d = kid(pd, depth, c, width=12, per_level=24)
                    nxt.append((0, d, pid))
            ids = []
            for p, (_, d, pid) in enumerate(nxt):
                nid = v.add(pid, d, w=0.5 + 0.001 * p if depth == 9 else 1.0, leaf=int(depth == 9))
                assert nid == 2 ** (depth + 1) - 1 + p
                ids.append((nid, d))
            level = ids
        _DEEP = (v, [d for _, d in level], g)
    return _DEEP


def _deep_case(name, levelsup):
    v, leaves, _ = _deep()
    g = _rng(name)
    lvl = 10 - levelsup
    nid = [2 ** lvl - 1 + (p >> (10 - lvl)) if 1 <= lvl <= 10 else 0 for p in DEEP_PATHS]
    return Case(name, "descent", v, [near(g, leaves[p], 3) for p in DEEP_PATHS],
                {"word": list(DEEP_PATHS), "depth": [10] * len(DEEP_PATHS), "nid": nid}, levelsup=levelsup)


def _chain():
    g = _rng("chain")
    v = Voc(1, 4)
    d = rdesc(g)
    for depth in range(4):
        d = flipn(g, d, 8)
        v.add(depth, d, w=0.75, leaf=int(depth == 3))
    return Case("single_child_chain", "descent", v, [rdesc(g), rdesc(g)],
                {"depth": [4, 4], "word": [0, 0], "nid": [2, 2], "nties": [[1] * 4] * 2, "nc": [[1] * 4] * 2},
                levelsup=2)


def _childless_unflagged():
    """B has no children and is not flagged as a word: Node() leaves its word id 0, and its weight adds into word 0"""
    g = _rng("childless")
    r = rdesc(g)
    v = Voc(2, 2)
    da, db = kid(r, 0, 0), kid(r, 0, 1)
    a = v.add(0, da)
    v.add(0, db, w=2.5)
    d0, d1 = kid(da, 1, 0), kid(da, 1, 1)
    v.add(a, d0, w=1.5, leaf=1)
    v.add(a, d1, w=0.25, leaf=1)
    return Case("childless_unflagged_node", "descent", v, [near(g, x) for x in (db, d0, d1, db)],
                {"word": [0, 0, 1, 0], "depth": [1, 2, 2, 1], "nid": [0, 3, 4, 0], "nwords": 2, "tf_div": True},
                scoring=DOT_PRODUCT, weighting=TF_IDF, levelsup=0)


def _flagged_with_children():
    """A is flagged (it takes word id 0) and has children: the descent goes on (isLeaf = no children)"""
    g = _rng("flagged")
    r = rdesc(g)
    v = Voc(2, 2)
    da, db = kid(r, 0, 0), kid(r, 0, 1)
    a = v.add(0, da, w=9.0, leaf=1)
    d0, d1 = kid(da, 1, 0), kid(da, 1, 1)
    v.add(a, d0, w=1.0, leaf=1)
    v.add(a, d1, w=2.0, leaf=1)
    v.add(0, db, w=4.0, leaf=1)
    return Case("flagged_node_with_children", "descent", v, [near(g, x) for x in (d0, d1, db)],
                {"word": [1, 2, 3], "depth": [2, 2, 1], "nid": [1, 1, 4]}, levelsup=1)


def _shallow():
    """L = 4, levelsup = 1: the FeatureVector key is the node at level 3; a branch that ends above it reports 0"""
    g = _rng("shallow")
    r = rdesc(g)
    v = Voc(2, 4)
    ds, dt = kid(r, 0, 0), kid(r, 0, 1)
    s = v.add(0, ds)                              # 1
    ds0, ds1 = kid(ds, 1, 0), kid(ds, 1, 1)
    v.add(s, ds0, w=1.25, leaf=1)                 # 2: word 0, depth 2
    s1 = v.add(s, ds1)                            # 3
    ds10 = kid(ds1, 2, 0)
    s10 = v.add(s1, ds10)                         # 4: depth 3
    d100, d101 = kid(ds10, 3, 0), kid(ds10, 3, 1)
    v.add(s10, d100, w=0.5, leaf=1)               # 5: word 1
    v.add(s10, d101, w=0.75, leaf=1)              # 6: word 2
    v.add(0, dt, w=3.0, leaf=1)                   # 7: word 3, depth 1
    return Case("branch_shallower_than_nid_level", "descent", v, [near(g, x) for x in (ds0, d100, dt, d101)],
                {"word": [0, 1, 3, 2], "depth": [2, 4, 1, 4], "nid": [0, 4, 0, 4]}, levelsup=1)


MIXED_DEPTHS = (10, 1, 6, 3, 3, 6, 1, 10, 1, 1, 1, 1, 10, 10, 10, 10, 3)


def _mixed_depths():
    """chains of depth 1, 3, 6 and 10 under the root; the first four queries (one 64-lane wave of 16 lanes per
    descriptor) stop at all four depths"""
    g = _rng("mixed")
    v = Voc(4, 10)
    heads = {t: rdesc(g) for t in (1, 3, 6, 10)}
    ids = {}
    for t in (1, 3, 6, 10):
        ids[t] = [v.add(0, heads[t], w=0.25 * t, leaf=int(t == 1))]
    for t in (3, 6, 10):
        d = heads[t]
        for depth in range(2, t + 1):
            d = flipn(g, d, 8)
            ids[t].append(v.add(ids[t][-1], d, w=0.25 * t, leaf=int(depth == t)))
    assert set(MIXED_DEPTHS[:4]) == {1, 3, 6, 10}
    word = {1: 0, 3: 1, 6: 2, 10: 3}
    nid = {1: 0, 3: 0, 6: ids[6][5], 10: ids[10][5]}
    return Case("depths_1_3_6_10_in_one_wave", "descent", v, [flipn(g, heads[t], 5) for t in MIXED_DEPTHS],
                {"depth": list(MIXED_DEPTHS), "word": [word[t] for t in MIXED_DEPTHS],
                 "nid": [nid[t] for t in MIXED_DEPTHS]}, levelsup=4)


# -------------------------------------------------------------------------------------------------------------- bow
_BIG = None


def _big():
    """k = 16, L = 3: 4096 words, leaf (a, b, c) is word 256 a + 16 b + c and descends to itself"""
    global _BIG
    if _BIG is None:
        g = _rng("big")
        v = Voc(16, 3)
        tops = [rdesc(g) for _ in range(16)]
        assert min(ham(tops[i], tops[j]) for i in range(16) for j in range(i)) > 80
        for d in tops:
            v.add(0, d)
        mids = []
        for a in range(16):
            for b in range(16):
                d = flip(tops[a], range(16 * b, 16 * b + 16))
                v.add(1 + a, d)
                mids.append(d)
        leaves = []
        for ab in range(256):
            for c in range(16):
                d = flip(mids[ab], range(16 * c, 16 * c + 8))
                v.add(17 + ab, d, w=float(g.uniform(0.1, 8.0)), leaf=1)
                leaves.append(d)
        _BIG = (v, np.array(leaves, np.uint8))
    return _BIG


def _one_word_4096():
    g = _rng("one_word")
    v = Voc(2, 1)
    d0 = rdesc(g)
    v.add(0, d0, w=0.1, leaf=1)
    v.add(0, ~d0, w=0.7, leaf=1)
    feats = [flip(d0, [i % 256]) for i in range(4096)]
    return Case("one_word_4096_features", "bow", v, feats,
                {"kept": 4096, "nwords": 1, "max_per_word": 4096, "tf_div": True},
                scoring=DOT_PRODUCT, weighting=TF, levelsup=0)


def _own_word_4096():
    v, leaves = _big()
    perm = _rng("own_word").permutation(4096)
    return Case("own_word_4096_features", "bow", v, leaves[perm],
                {"kept": 4096, "nwords": 4096, "max_per_word": 1, "word": perm.tolist(), "norm_side": "pos"},
                levelsup=1)


def _word_count(nw, scoring):
    v, leaves = _big()
    sel = _rng("word_count_%d" % nw).permutation(4096)
    idx = np.concatenate([sel[:nw], sel[:nw // 2]]).astype(np.int64)
    return Case("word_count_%d_scoring_%d" % (nw, scoring), "bow", v, leaves[idx],
                {"nwords": nw, "kept": nw + nw // 2, "max_per_word": 0 if nw == 0 else 1 if nw == 1 else 2,
                 "word": idx.tolist()}, scoring=scoring, levelsup=1)


_STOPV = None


def _stopv():
    """k = 16, L = 2: 256 words, the odd ones stopped (weight 0.0)"""
    global _STOPV
    if _STOPV is None:
        g = _rng("stopv")
        v = Voc(16, 2)
        tops = [rdesc(g) for _ in range(16)]
        assert min(ham(tops[i], tops[j]) for i in range(16) for j in range(i)) > 80
        for d in tops:
            v.add(0, d)
        leaves = []
        for a in range(16):
            for b in range(16):
                d = flip(tops[a], range(16 * b, 16 * b + 16))
                v.add(1 + a, d, w=0.0 if (16 * a + b) % 2 else float(g.uniform(0.1, 8.0)), leaf=1)
                leaves.append(d)
        _STOPV = (v, leaves)
    return _STOPV


def _kept(m):
    v, leaves = _stopv()
    words = []
    for i in range(m):
        words += [2 * (i % 128), 2 * ((7 * i) % 128) + 1]
    words += [1, 255, 3] if m == 0 else [255]
    return Case("kept_%d_interleaved_stopped" % m, "bow", v, [leaves[w] for w in words],
                {"kept": m, "nwords": min(m, 128), "word": words,
                 "stopped": ["zero" if w % 2 else None for w in words]}, levelsup=1)


_STOPR = None
STOP_WEIGHTS = (1.5, 0.0, -0.0, -2.0, float("nan"))
STOP_NAMES = (None, "zero", "negzero", "negative", "nan")


def _stop_reasons(name, targets):
    global _STOPR
    if _STOPR is None:
        g = _rng("stopr")
        v = Voc(5, 1)
        leaves = [rdesc(g) for _ in STOP_WEIGHTS]
        for d, w in zip(leaves, STOP_WEIGHTS):
            v.add(0, d, w=w, leaf=1)
        _STOPR = (v, leaves)
    v, leaves = _STOPR
    g = _rng(name)
    kept = sum(1 for t in targets if t == 0)
    return Case(name, "bow", v, [near(g, leaves[t]) for t in targets],
                {"word": list(targets), "stopped": [STOP_NAMES[t] for t in targets], "kept": kept,
                 "nwords": int(kept > 0), "flags": {"stop_" + STOP_NAMES[t] for t in targets if t}}, levelsup=0)


def _word0_feeders():
    g = _rng("feeders")
    v = Voc(5, 1)
    spec = [(0.3, 0), (1.1, 1), (7.0, 0), (0.6, 1), (1e-3, 0)]  # (weight, flagged): words 0 and 1 are nodes 2 and 4
    ds = [rdesc(g) for _ in spec]
    for d, (w, lf) in zip(ds, spec):
        v.add(0, d, w=w, leaf=lf)
    targets = [0, 1, 2, 3, 4, 0, 1]
    return Case("unflagged_nodes_feed_word_0", "bow", v, [near(g, ds[t]) for t in targets],
                {"word": [0, 0, 0, 1, 0, 0, 0], "nwords": 2, "max_per_word": 6, "kept": 7, "tf_div": True},
                scoring=DOT_PRODUCT, weighting=TF_IDF, levelsup=0)


_SMALL = None


def _scoring_weighting(scoring, weighting):
    global _SMALL
    if _SMALL is None:
        g = _rng("small")
        v = Voc(3, 2)
        r = rdesc(g)
        tops = [kid(r, 0, c) for c in range(3)]
        for d in tops:
            v.add(0, d)
        leaves = []
        for a in range(3):
            for c in range(3):
                d = kid(tops[a], 1, c)
                v.add(1 + a, d, w=0.0 if 3 * a + c == 5 else float(g.uniform(0.1, 8.0)), leaf=1)
                leaves.append(d)
        _SMALL = (v, leaves)
    v, leaves = _SMALL
    g = _rng("small_q")
    targets = [0, 4, 8, 4, 4, 2, 7, 0, 8, 8, 1, 3, 5, 6]
    return Case("scoring_%d_weighting_%d" % (scoring, weighting), "bow", v, [near(g, leaves[t]) for t in targets],
                {"word": targets, "kept": 13, "nwords": 8, "max_per_word": 3,
                 "tf_div": scoring == DOT_PRODUCT and weighting in (TF_IDF, TF),
                 "norm_side": None if scoring == DOT_PRODUCT else "pos"},
                scoring=scoring, weighting=weighting, levelsup=1)


def _l2_extreme(name, x, side):
    g = _rng(name)
    v = Voc(3, 1)
    ds = [rdesc(g) for _ in range(3)]
    for j, d in enumerate(ds):
        v.add(0, d, w=x * (j + 1), leaf=1)
    return Case(name, "bow", v, [near(g, ds[t]) for t in (0, 1, 0, 2)],
                {"word": [0, 1, 0, 2], "norm_side": side, "nwords": 3, "kept": 4}, scoring=L2_NORM, levelsup=0)


_DOTV = None


def _dot(name, weighting):
    global _DOTV
    if _DOTV is None:
        g = _rng("dotv")
        v = Voc(3, 1)
        ds = [rdesc(g) for _ in range(3)]
        for d, w in zip(ds, (0.5, 0.25, 3.0)):
            v.add(0, d, w=w, leaf=1)
        _DOTV = (v, ds)
    v, ds = _DOTV
    g = _rng(name)
    return Case(name, "bow", v, [near(g, ds[t]) for t in (0, 0, 1)],
                {"word": [0, 0, 1], "nwords": 2, "kept": 3, "tf_div": weighting == TF, "norm_side": None},
                scoring=DOT_PRODUCT, weighting=weighting, levelsup=0)


# ------------------------------------------------------------------------------------------------------------ order
def _order_in_word():
    """unflagged childless nodes of weights 1e-8 .. 1e8 all add into word 0, in feature order"""
    g = _rng("order_word")
    ws = [1e8, 1.0, 1e-8, 3e7, 1e-8, 0.1, 1e-8, 7e-3, 1e-8]
    v = Voc(9, 1)
    ds = [rdesc(g) for _ in ws]
    for j, (d, w) in enumerate(zip(ds, ws)):
        v.add(0, d, w=w, leaf=int(j == len(ws) - 1))
    targets = list(range(len(ws))) + [2, 5, 0, 7]
    return Case("order_inside_one_word", "order", v, [near(g, ds[t]) for t in targets],
                {"nwords": 1, "max_per_word": len(targets), "order": "word", "tf_div": True},
                scoring=DOT_PRODUCT, weighting=TF_IDF, levelsup=0)


def _order_across_words():
    """24 words of weights 1e-8 .. 1e8: the L1 norm adds them in word order"""
    g = _rng("order_norm")
    v = Voc(20, 1)
    ds = [rdesc(g) for _ in range(24)]
    for j, d in enumerate(ds):
        v.add(0, d, w=10.0 ** ((7 * j) % 17 - 8) * (1.0 + j / 7.0), leaf=1)
    targets = g.permutation(24).tolist()
    return Case("order_across_words", "order", v, [near(g, ds[t]) for t in targets],
                {"nwords": 24, "word": targets, "order": "norm", "norm_side": "pos", "flags": {"trip2"}}, levelsup=0)


def _build():
    cs = [_dup(0, 1), _dup(0, 16), _dup(3, 19), _dup(5, 18), _all_256(), _dist_0(), _fanout(), _l1(),
          _deep_case("L10_k2", 4)]
    cs += [_deep_case("levelsup_%d" % s, s) for s in LEVELSUPS]
    cs += [_chain(), _childless_unflagged(), _flagged_with_children(), _shallow(), _mixed_depths()]
    cs += [_one_word_4096(), _own_word_4096()]
    cs += [_word_count(nw, sc) for sc in (L1_NORM, L2_NORM) for nw in WORD_COUNTS]
    cs += [_kept(m) for m in KEPT_COUNTS]
    cs += [_stop_reasons("stopped_by_zero_negzero_negative_nan", (0, 1, 2, 3, 4, 0, 4)),
           _stop_reasons("all_features_stopped", (1, 2, 3, 4)), _word0_feeders()]
    cs += [_scoring_weighting(sc, wt) for sc in SCORINGS for wt in WEIGHTINGS]
    cs += [_l2_extreme("l2_weights_1e-200", 1e-200, "zero"), _l2_extreme("l2_weights_5e-324", 5e-324, "zero"),
           _l2_extreme("l2_weights_1e200", 1e200, "pos"), _dot("dot_product_tf", TF), _dot("dot_product_idf", IDF)]
    cs += [_order_in_word(), _order_across_words()]
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


def launches():
    """the cases grouped into batch launches: one vocabulary handle, one levelsup; every case is in exactly one"""
    groups = {}
    for c in CASES:
        groups.setdefault(c.launch_key(), []).append(c)
    return list(groups.values())

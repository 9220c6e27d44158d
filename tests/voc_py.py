"""Pure-Python restatement of the DBoW2 vocabulary transform (TemplatedVocabulary<FORB>::transform(features, BowVector&,
FeatureVector&, levelsup) of the ORB-SLAM2 fork), with a trace of the exits it takes.

Plain Python and numpy in float64, the std::map iteration order (ascending word / node id), the sums in the order the
map code runs them: a word's weights in feature order, the norm in word order. The trace is taken from this restatement
only; voc_cases.py's expectations are asserted against it (test_voc_cases.py), never against the code under test.
"""
import math

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
TF_IDF, TF, IDF, BINARY = range(4)

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)

FLAGS = ("trip2", "trip3", "tie_congruent", "tie_cross", "norm_pos", "norm_zero", "stop_zero", "stop_negzero",
         "stop_negative", "stop_nan", "tf_div")


def stop_reason(w):
    """why `w > 0` is false (None when it is true)"""
    if w > 0:
        return None
    if w != w:
        return "nan"
    if w < 0:
        return "negative"
    return "negzero" if math.copysign(1.0, w) < 0 else "zero"


class Level:
    """one level of one feature's descent"""
    __slots__ = ("nc", "nties", "winner", "trips", "tie_congruent", "tie_cross")

    def __init__(self, dist):
        self.nc = len(dist)
        dmin = dist.min()
        tied = np.flatnonzero(dist == dmin)
        self.nties = len(tied)
        self.winner = int(tied[0])  # first strict minimum of the `d < best_d` scan
        self.trips = (self.nc + 15) // 16  # trips of a 16-wide loop over the children
        lanes = tied % 16
        self.tie_congruent = len(set(lanes.tolist())) < len(lanes)
        # a tied pair a < b with a mod 16 > b mod 16: the lower position sits in the higher lane
        self.tie_cross = any(int(lanes[i]) > int(lanes[j]) for i in range(len(tied)) for j in range(i + 1, len(tied)))


class Result:
    """bow = (word ids uint32, values float64), fv = {node: [features]}, word / weight / nid per feature, and the trace:
    levels[i] (one Level per level of feature i), depth[i], stopped[i] (None or the reason), kept, nwords,
    max_per_word, word_addends {word: weights in the order they are added}, norm_addends (values in word order, before
    the norm), norm (None when the scoring does not normalise), norm_side ('pos' / 'zero' / None), tf_div"""

    def flags(self):
        s = set()
        for lv in self.levels:
            for x in lv:
                if x.trips >= 2:
                    s.add("trip2")
                if x.trips >= 3:
                    s.add("trip3")
                if x.tie_congruent:
                    s.add("tie_congruent")
                if x.tie_cross:
                    s.add("tie_cross")
        for r in self.stopped:
            if r:
                s.add("stop_" + r)
        if self.norm_side:
            s.add("norm_" + self.norm_side)
        if self.tf_div:
            s.add("tf_div")
        return s

    def summary(self):
        return {"word": [int(x) for x in self.word], "nid": [int(x) for x in self.nid], "depth": list(self.depth),
                "stopped": list(self.stopped), "winner": [[x.winner for x in lv] for lv in self.levels],
                "nties": [[x.nties for x in lv] for lv in self.levels],
                "nc": [[x.nc for x in lv] for lv in self.levels], "kept": self.kept, "nwords": self.nwords,
                "max_per_word": self.max_per_word, "norm_side": self.norm_side, "tf_div": self.tf_div,
                "flags": self.flags()}


def transform_trace(k, L, scoring, weighting, parent, is_leaf, desc, weight, feats, levelsup):
    n = len(parent) + 1
    children = [[] for _ in range(n)]
    word = [0] * n  # Node() default 0 for nodes not flagged as words
    nw = 0
    for i in range(1, n):
        children[parent[i - 1]].append(i)
        if is_leaf[i - 1] > 0:
            word[i] = nw
            nw += 1
    children = [np.array(c, np.int64) for c in children]
    D = np.concatenate([np.zeros((1, 32), np.uint8), np.asarray(desc, np.uint8).reshape(-1, 32)])
    W = np.concatenate([[0.0], np.asarray(weight, np.float64)])
    feats = np.asarray(feats, np.uint8).reshape(-1, 32)
    r = Result()
    nf = len(feats)
    r.word, r.weight, r.nid = np.zeros(nf, np.int32), np.zeros(nf, np.float64), np.zeros(nf, np.int32)
    r.levels, r.depth, r.stopped = [], [], []
    bow, fv, addends = {}, {}, {}
    must = scoring != DOT_PRODUCT
    empty = len(children[0]) == 0  # TemplatedVocabulary::empty()
    nid_level = L - levelsup
    for i, f in enumerate(feats):
        nid = 0
        node, level = 0, 0
        lv = []
        while len(children[node]):
            level += 1
            ch = children[node]
            x = Level(_POP[D[ch] ^ f].sum(axis=1))
            lv.append(x)
            node = int(ch[x.winner])
            if level == nid_level:
                nid = node
        w = float(W[node])
        r.word[i], r.weight[i], r.nid[i] = word[node], w, nid
        r.levels.append(lv)
        r.depth.append(level)
        r.stopped.append(stop_reason(w))
        if empty:
            continue
        if w > 0:
            wid = word[node]
            if weighting in (TF_IDF, TF):  # BowVector::addWeight
                bow[wid] = bow[wid] + w if wid in bow else w
                addends.setdefault(wid, []).append(w)
            elif wid not in bow:  # BowVector::addIfNotExist
                bow[wid] = w
                addends[wid] = [w]
            fv.setdefault(nid, []).append(i)
    keys = sorted(bow)
    vals = [bow[kk] for kk in keys]
    r.kept = sum(len(v) for v in fv.values())
    r.nwords = len(keys)
    per_word = {}
    for i in range(nf):
        if not empty and r.weight[i] > 0:
            per_word[int(r.word[i])] = per_word.get(int(r.word[i]), 0) + 1
    r.max_per_word = max(per_word.values()) if per_word else 0
    r.word_addends = addends
    r.tf_div = bool(weighting in (TF_IDF, TF) and vals and not must)
    if r.tf_div:
        vals = [v / float(len(vals)) for v in vals]
    r.norm, r.norm_side, r.norm_addends = None, None, list(vals)
    if must and not empty:
        norm = 0.0
        if scoring == L2_NORM:
            with np.errstate(over="ignore", under="ignore"):
                for v in vals:
                    norm += float(np.float64(v) * np.float64(v))
            norm = math.sqrt(norm)
        else:
            for v in vals:
                norm += abs(v)
        r.norm = norm
        r.norm_side = "pos" if norm > 0 else "zero"
        if norm > 0:
            vals = [v / norm for v in vals]
    r.bow = (np.array(keys, np.uint32), np.array(vals, np.float64))
    r.fv = fv
    return r


def transform_py(k, L, scoring, weighting, parent, is_leaf, desc, weight, feats, levelsup):
    """Pure-Python TemplatedVocabulary::transform (features, BowVector, FeatureVector, levelsup)."""
    r = transform_trace(k, L, scoring, weighting, parent, is_leaf, desc, weight, feats, levelsup)
    return r.bow, r.fv

"""Keyframe database, host half (no GPU): orbdb_select_candidates against the literal restatement of
KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates (tests/kfdb_ref.py,
KeyFrameDatabase.cc:76-309), fed restatement-computed counts, scores and first common words; the argument
checks of orbdb_create / orbdb_add."""
import ctypes as C

import numpy as np
import pytest

import kfdb_ref as R
import orbamd
from orbamd.database import MODE_LOOP, MODE_RELOC, KeyFrameDatabase, select_candidates


def bow(words, rng=None, values=None):
    """An L1-normalised BowVector over ascending `words`."""
    w = np.array(sorted(words), np.uint32)
    v = np.asarray(values, np.float64) if values is not None else rng.uniform(0.1, 8.0, len(w))
    return w, v / np.abs(v).sum() if len(w) else v


class Scenario:
    """The restatement's database next to the arrays orbdb_select_candidates takes: the live keyframes in
    insertion order, their neighbour lists as entry indices, the persistent score of the mode."""

    def __init__(self):
        self.ref = R.RefDatabase()
        self.order = []

    def add(self, kf):
        self.ref.add(kf)
        self.order.append(kf)
        return kf

    def erase(self, kf):
        self.ref.erase(kf)
        self.order.remove(kf)

    def arrays(self, q):
        sc = [R.l1_score(q.bow, k.bow) for k in self.order]
        return (np.array([s[1] for s in sc], np.int32), np.array([s[0] for s in sc], np.float32),
                np.array([s[2] for s in sc], np.uint32))

    def run(self, mode, q, min_score=0.0):
        """Both sides on the same state; returns the candidates (KF objects) after asserting they agree."""
        attr = "mLoopScore" if mode == MODE_LOOP else "mRelocScore"
        nc, sc, fw = self.arrays(q)
        idx = {id(k): i for i, k in enumerate(self.order)}
        neigh = [[idx.get(id(j), -1) for j in k.neigh[:10]] for k in self.order]
        last = np.array([getattr(k, attr) for k in self.order], np.float32)
        conn = np.array([k in q.connected for k in self.order], np.uint8) if mode == MODE_LOOP else None
        got = select_candidates(mode, nc, sc, fw, neigh, last, conn, min_score)
        if mode == MODE_LOOP:
            want = self.ref.detect_loop_candidates(q, min_score)
        else:
            want = self.ref.detect_relocalization_candidates(q)
        assert [self.order[i] for i in got] == want
        after = np.array([getattr(k, attr) for k in self.order], np.float32)
        assert np.array_equal(R.bits(last), R.bits(after)), "persistent scores differ from the restatement's"
        return want


@pytest.mark.parametrize("mode", [MODE_LOOP, MODE_RELOC])
@pytest.mark.parametrize("maxw", [5, 10])
def test_exactly_min_common_words_is_excluded(mode, maxw):
    rng = np.random.default_rng(maxw)
    minw = int(np.float32(maxw) * np.float32(0.8))
    assert minw == {5: 4, 10: 8}[maxw]
    s = Scenario()
    q = R.KF(*bow(range(0, 20), rng))
    full = s.add(R.KF(*bow(list(range(0, maxw)) + [100, 101], rng)))
    edge = s.add(R.KF(*bow(list(range(0, minw)) + [102, 103], rng)))       # exactly minCommonWords: excluded
    above = s.add(R.KF(*bow(list(range(0, minw + 1)) + [104], rng)))       # one more: scored
    for k in (full, edge, above):
        k.mLoopScore = k.mRelocScore = np.float32(7.5)  # sentinel
    out = s.run(mode, q, 0.0)
    assert edge not in out and full in out
    score = "mLoopScore" if mode == MODE_LOOP else "mRelocScore"
    assert getattr(edge, score) == np.float32(7.5), "an entry at minCommonWords must not be scored"
    assert getattr(above, score) != np.float32(7.5) and getattr(full, score) != np.float32(7.5)


def test_connected_keyframe_with_the_highest_score_loop():
    rng = np.random.default_rng(1)
    s = Scenario()
    qb = bow(range(0, 12), rng)
    q = R.KF(*qb)
    twin = s.add(R.KF(*qb))  # the query's own BowVector: the highest score, but connected
    a = s.add(R.KF(*bow(list(range(0, 11)) + [50], rng)))
    b = s.add(R.KF(*bow(list(range(1, 12)) + [51], rng)))
    q.connected = {twin}
    a.neigh = [twin, b]  # the connected neighbour never counts as queried
    b.neigh = [twin]
    twin.mLoopScore = np.float32(9.0)
    out = s.run(MODE_LOOP, q, 0.01)
    assert twin not in out and out
    assert twin.mLoopScore == np.float32(9.0) and twin.mnLoopQuery != q.mnId
    # without the connection it wins
    q2 = R.KF(*qb)
    assert s.run(MODE_LOOP, q2, 0.01)[0] is twin


def _stale_scene():
    rng = np.random.default_rng(2)
    s = Scenario()
    f1b = bow(range(100, 112), rng)
    a = s.add(R.KF(*bow(list(range(0, 10)) + [200], rng)))
    b = s.add(R.KF([5] + f1b[0].tolist(), np.concatenate([[0.01], f1b[1] * 0.99])))
    a.neigh = [b]
    f1 = R.KF(*f1b)               # scores b high, shares nothing with a
    f2 = R.KF(*bow(range(0, 10), rng))  # a shares 10 words; b shares word 5 only: not scored, still "queried"
    return s, a, b, f1, f2


def test_reloc_second_query_reads_a_stale_score():
    s, a, b, f1, f2 = _stale_scene()
    assert s.run(MODE_RELOC, f1) == [b]
    stale = b.mRelocScore
    assert stale > np.float32(0.5)
    out = s.run(MODE_RELOC, f2)
    assert b.mRelocScore == stale, "b was not scored by the second query"
    # fresh state: the same second query alone
    s0, a0, b0, _, f20 = _stale_scene()
    fresh = s0.run(MODE_RELOC, f20)
    assert fresh == [a0] and out == [b], "the stale mRelocScore must change the result"


def test_neighbours_outside_the_database():
    rng = np.random.default_rng(3)
    s = Scenario()
    q = R.KF(*bow(range(0, 10), rng))
    a = s.add(R.KF(*bow(range(0, 10), rng)))
    b = s.add(R.KF(*bow(range(0, 9), rng)))
    ghost = R.KF(*bow(range(0, 10), rng))  # never added: index -1
    ghost.mLoopScore = ghost.mRelocScore = np.float32(5.0)
    a.neigh = [ghost, b]
    b.neigh = [ghost, ghost, a]
    for mode in (MODE_LOOP, MODE_RELOC):
        assert s.run(mode, R.KF(*q.bow), 0.0)


def test_empty_database():
    s = Scenario()
    q = R.KF(*bow(range(5), np.random.default_rng(4)))
    assert s.run(MODE_LOOP, q, 0.0) == [] and s.run(MODE_RELOC, q) == []
    db = KeyFrameDatabase(8, 16)
    keys, nc, sc, fw = db.query(*q.bow)  # no entry, no launch: answers without a device
    assert len(keys) == 0
    assert db.detect_loop_candidates(q.bow[0], q.bow[1], [], {}, 0.0) == []
    assert db.detect_relocalization_candidates(q.bow[0], q.bow[1], {}) == []


def test_all_scores_below_min_score():
    rng = np.random.default_rng(5)
    s = Scenario()
    q = R.KF(*bow(range(0, 10), rng))
    ks = [s.add(R.KF(*bow(range(0, 10), rng))) for _ in range(4)]
    assert s.run(MODE_LOOP, q, 2.0) == []  # an L1 score never exceeds 1
    assert all(k.mLoopScore < np.float32(2.0) and k.mnLoopQuery == q.mnId for k in ks)


def test_ties_on_first_common_word_follow_insertion_order():
    rng = np.random.default_rng(6)
    s = Scenario()
    qb = bow(range(10, 20), rng)
    mk = lambda extra: R.KF(*bow(list(range(10, 20)) + [extra], rng))  # noqa: E731
    early = s.add(R.KF(*bow(list(range(12, 20)) + [3, 4], rng)))  # first common word 12: after the tied pair
    a, b = s.add(mk(30)), s.add(mk(31))
    out = s.run(MODE_RELOC, R.KF(*qb))
    assert out.index(a) < out.index(b)
    assert s.run(MODE_LOOP, R.KF(*qb), 0.0) == out
    s.erase(a)
    s.add(a)  # a new insertion sequence number: now behind b
    out = s.run(MODE_RELOC, R.KF(*qb))
    assert out.index(b) < out.index(a)
    assert early in s.order


@pytest.mark.parametrize("seed", range(6))
def test_random_sequences(seed):
    """Loop and reloc queries interleaved with erase / re-add over one persistent state."""
    rng = np.random.default_rng(100 + seed)
    s = Scenario()
    nwords = 40

    def rand_kf():
        return R.KF(*bow(rng.choice(nwords, int(rng.integers(3, 25)), replace=False).tolist(), rng))

    pool = [rand_kf() for _ in range(30)]
    for k in pool:
        k.neigh = [pool[j] for j in rng.choice(30, int(rng.integers(0, 11)), replace=False)]
    for k in pool[:24]:
        s.add(k)
    nonempty = 0
    for step in range(12):
        q = rand_kf()
        if step % 2 == 0:
            q.connected = {pool[j] for j in rng.choice(30, 5, replace=False)}
            ms = float(rng.choice([0.0, 0.05, 0.2]))
            nonempty += bool(s.run(MODE_LOOP, q, ms))
        else:
            nonempty += bool(s.run(MODE_RELOC, q))
        victim = s.order[int(rng.integers(len(s.order)))]
        s.erase(victim)
        if step % 3:
            s.add(victim)
        elif pool[24 + step % 6] not in s.order:
            s.add(pool[24 + step % 6])
    assert nonempty >= 6


def test_select_candidates_argument_checks():
    lib = orbamd.load()
    n = C.c_int(7)
    z = np.zeros(4, np.int32)
    f = np.zeros(4, np.float32)
    assert lib.orbdb_select_candidates(2, 0, None, None, None, None, None, None, 0.0, None, None, C.byref(n)) == -1
    assert lib.orbdb_select_candidates(0, 0, None, None, None, None, None, None, 0.0, None, None, C.byref(n)) == 0
    assert n.value == 0
    off = np.array([0, 1], np.int32)
    bad = np.array([1], np.int32)  # neighbour index out of range
    assert lib.orbdb_select_candidates(1, 1, z.ctypes.data, f.ctypes.data, z.ctypes.data, None, off.ctypes.data,
                                       bad.ctypes.data, 0.0, f.ctypes.data, z.ctypes.data, C.byref(n)) == -1


def test_host_add_rejects_unsorted_and_overlong_input():
    lib = orbamd.load()
    h = C.c_void_p()
    assert lib.orbdb_create(0, 4, 8, 1, C.byref(h)) == -1, "only L1 scoring"
    assert lib.orbdb_create(0, 4, 4097, 0, C.byref(h)) == -1
    assert lib.orbdb_create(0, 0, 8, 0, C.byref(h)) == -1
    assert lib.orbdb_create(0, 4, 8, 0, C.byref(h)) == 0
    try:
        v = np.full(9, 1.0 / 9)
        for words in ([3, 2, 5], [1, 1, 2], list(range(9))):
            w = np.array(words, np.uint32)
            assert lib.orbdb_add(h, 1, w.ctypes.data, v.ctypes.data, len(w), None) == -1, words
        n = C.c_int(-1)
        assert lib.orbdb_entries(h, 0, None, None, C.byref(n)) == 0 and n.value == 0
        assert lib.orbdb_erase(h, 1, None) == 0  # unknown keys are ignored
        assert lib.orbdb_check_error(h, None) == 0
    finally:
        lib.orbdb_destroy(h)

"""GPU: the keyframe database (orbdb_*, db_kernels.hip) against the pure-Python restatement tests/kfdb_ref.py of
DBoW2's L1Scoring::score and KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates
(KeyFrameDatabase.cc:76-309). Scores are compared as raw float bits: the device adds the per-word terms in
ascending word order, as the restatement's sequential double loop does."""
import numpy as np
import pytest

import kfdb_ref as R
import orbamd
import proj_scenes as ps
from orbamd import exchange
from orbamd.database import KeyFrameDatabase
from orbamd.vocabulary import L1_NORM, TF_IDF, synth_vocabulary

pytestmark = pytest.mark.gpu
NEG_ZERO = 0x80000000


def _cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _norm(v):
    return v / np.abs(v).sum() if len(v) else v


def _expect(q, entries):
    sc = [R.l1_score(q, e) for e in entries]
    return (np.array([s[1] for s in sc], np.int32), np.array([s[0] for s in sc], np.float32),
            np.array([s[2] for s in sc], np.uint32))


def _assert_query(got, q, entries, what=""):
    keys, nc, sc, fw = got
    enc, esc, efw = _expect(q, entries)
    assert np.array_equal(keys, np.arange(len(entries), dtype=np.uint64)), what
    np.testing.assert_array_equal(nc, enc, what)
    np.testing.assert_array_equal(fw, efw, what)
    np.testing.assert_array_equal(R.bits(sc), R.bits(esc), what)


def test_chunk_edges():
    """Entry lengths around the 64-lane chunks (0, 1, 63, 64, 65, 129, word_stride), query lengths 0, 1 and 4096;
    common words on both sides of every chunk boundary, the no-common-word and the all-common cases."""
    rng = np.random.default_rng(11)
    stride = 200
    universe = 8192
    qw = np.sort(rng.choice(universe, 4096, replace=False)).astype(np.uint32)
    rest = np.setdiff1d(np.arange(universe, dtype=np.uint32), qw)
    big = (qw, _norm(rng.uniform(0.1, 8.0, 4096)))
    entries = []
    for n in (0, 1, 63, 64, 65, 129, stride):
        mixed = np.sort(rng.choice(universe, n, replace=False)).astype(np.uint32)
        inside = np.sort(rng.choice(qw, n, replace=False)).astype(np.uint32)   # all common
        outside = np.sort(rng.choice(rest, n, replace=False)).astype(np.uint32)  # none common
        # common words exactly at the chunk edges (lanes 63 | 64, 127 | 128, the last), the others not common:
        # position p takes its word from the p-th of n ascending 40-word ranges of the universe
        edge = np.zeros(n, np.uint32)
        for p, b in enumerate(np.sort(rng.choice(universe // 40, n, replace=False))):
            pool = qw if p in (0, 63, 64, 127, 128, n - 1) else rest
            edge[p] = pool[(pool >= 40 * b) & (pool < 40 * b + 40)][0]
        for w in (mixed, inside, outside, edge):
            entries.append((w, _norm(rng.uniform(0.1, 8.0, len(w)))))
    for n in rng.integers(2, stride, 40 - len(entries)):
        w = np.sort(rng.choice(universe, int(n), replace=False)).astype(np.uint32)
        entries.append((w, _norm(rng.uniform(0.1, 8.0, len(w)))))
    assert len(entries) == 40
    db = KeyFrameDatabase(48, stride)
    for i, (w, v) in enumerate(entries):
        db.add(i, w, v)
    one = entries[6 * 4 + 1]  # word_stride words, all common: its word at lane 0 of the second chunk
    queries = [(np.zeros(0, np.uint32), np.zeros(0)), (one[0][64:65], np.ones(1)), big]
    for q in queries:
        _assert_query(db.query(*q), q, entries, "query of %d words" % len(q[0]))
    # the cases by name
    keys, nc, sc, fw = db.query(*big)
    for n_i, n in enumerate((0, 1, 63, 64, 65, 129, stride)):
        assert nc[4 * n_i + 1] == n, "all common"
        assert nc[4 * n_i + 2] == 0 and R.bits(sc)[4 * n_i + 2] == NEG_ZERO and fw[4 * n_i + 2] == 0xFFFFFFFF
    keys, nc, sc, fw = db.query(*queries[0])
    assert not nc.any() and (R.bits(sc) == NEG_ZERO).all()
    assert not db.check_error()
    db.close()


def test_summation_order():
    """Values over three decades: the sum of the terms depends on their order; the device must give the forward
    (ascending word id) order's bits."""
    rng = np.random.default_rng(12)
    n = 300
    words = np.sort(rng.choice(5000, n, replace=False)).astype(np.uint32)
    q = (words, _norm(10.0 ** rng.uniform(-1.5, 1.5, n)))
    entries = [(words, _norm(10.0 ** rng.uniform(-1.5, 1.5, n))) for _ in range(12)]
    differ = 0
    for e in entries:
        terms, _ = R.l1_terms(q, e)
        fwd = rev = 0.0
        for t in terms:
            fwd += t
        for t in reversed(terms):
            rev += t
        differ += np.float64(fwd).view(np.uint64) != np.float64(rev).view(np.uint64)
    assert differ >= 1, "the inputs do not distinguish summation orders"
    db = KeyFrameDatabase(16, 512)
    for i, (w, v) in enumerate(entries):
        db.add(i, w, v)
    _assert_query(db.query(*q), q, entries)
    db.close()


def test_end_to_end_candidates():
    """ComputeBoW (orbv_transform) -> add_device -> detect_loop_candidates / detect_relocalization_candidates with
    synthetic connected sets and neighbour lists, through an erase, a re-add and later queries that reuse the
    stored scores; key lists, counts and scores against the restatement."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(13)
    k, L = 10, 4
    v = synth_vocabulary(k, L, 3)
    gv = orbamd.ORBVocabulary.from_arrays(k, L, L1_NORM, TF_IDF, *v[2:])
    descs = [ps.frame_features(a, t, 1000)[1] for a, t in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1))]

    def keyframe(f):  # a keyframe seeing a random 30 % of frame f's features
        d = descs[f]
        bow, _ = gv.transform(d[np.sort(rng.choice(len(d), int(0.3 * len(d)), replace=False))], 2)
        return bow

    nkf = 60
    kfs = [R.KF(*keyframe(i % 6), key=1000 + i) for i in range(nkf)]
    for kf in kfs:
        kf.neigh = [kfs[j] for j in rng.choice(nkf, int(rng.integers(0, 11)), replace=False)]
    neighbours = {kf.key: [n.key for n in kf.neigh] for kf in kfs}
    db = KeyFrameDatabase(64, 512)
    ref = R.RefDatabase()
    order, keep = [], []

    def add(kf):
        t = (_cuda(torch, kf.bow[0]), _cuda(torch, kf.bow[1]), _cuda(torch, np.array([len(kf.bow[0])], np.int32)))
        keep.append(t)
        db.add_device(kf.key, *t)
        ref.add(kf)
        order.append(kf)

    def erase(kf):
        db.erase(kf.key)
        ref.erase(kf)
        order.remove(kf)

    def check(mode, q, min_score=0.0):
        if mode == "loop":
            got = db.detect_loop_candidates(q.bow[0], q.bow[1], [c.key for c in q.connected], neighbours, min_score)
            want = ref.detect_loop_candidates(q, min_score)
            store, attr = db.loop_score, "mLoopScore"
        else:
            got = db.detect_relocalization_candidates(q.bow[0], q.bow[1], neighbours)
            want = ref.detect_relocalization_candidates(q)
            store, attr = db.reloc_score, "mRelocScore"
        keys, nc, sc, fw = db.last
        assert keys.tolist() == [kf.key for kf in order]
        enc, esc, efw = _expect(q.bow, [kf.bow for kf in order])
        np.testing.assert_array_equal(nc, enc)
        np.testing.assert_array_equal(R.bits(sc), R.bits(esc))
        np.testing.assert_array_equal(fw, efw)
        assert got == [kf.key for kf in want]
        stored = np.array([store[kf.key] for kf in order], np.float32)
        np.testing.assert_array_equal(R.bits(stored), R.bits(np.array([getattr(kf, attr) for kf in order])))
        return got

    for kf in kfs[:54]:
        add(kf)
    found = 0
    for step in range(3):
        q = R.KF(*keyframe(step))
        q.connected = {kfs[j] for j in rng.choice(nkf, 6, replace=False)}
        found += len(check("loop", q, 0.02))
        found += len(check("reloc", R.KF(*keyframe(step + 3))))
    victim = order[5]
    erase(victim)
    erase(order[20])
    found += len(check("reloc", R.KF(*keyframe(0))))
    add(victim)  # re-added: a new sequence number, behind the others
    for kf in kfs[54:]:
        add(kf)
    assert order[-7] is victim
    q = R.KF(*keyframe(1))
    q.connected = {kfs[j] for j in rng.choice(nkf, 6, replace=False)}
    found += len(check("loop", q, 0.02))
    found += len(check("reloc", R.KF(*keyframe(1))))  # reads the scores the earlier queries stored
    assert found >= 6
    assert not db.check_error()
    db.close()


def test_slots_in_place():
    """add_slots_device fills entries from the BOWWORD / BOWVALUE sections and header nbow of slots in a receive
    buffer; query_device with byte stride slot_bytes takes the queries from the same slots in place."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(14)
    cap = 300
    kps = np.zeros(4, exchange.KP_DTYPE)
    desc = np.zeros((4, 32), np.uint8)
    bows, hosts = [], []
    for r, n in enumerate((250, 64, 129)):
        w = np.sort(rng.choice(600, n, replace=False)).astype(np.uint32)
        bows.append((w, _norm(rng.uniform(0.1, 8.0, n))))
        hosts.append(exchange.pack_host(exchange.make_meta(agent=r, mnId=r), kps, desc, cap, bow=bows[-1]))
    sb = exchange.slot_bytes(cap)
    assert all(h.size == sb for h in hosts)
    slots = _cuda(torch, np.concatenate(hosts))
    db = KeyFrameDatabase(8, cap)
    db.add_slots_device(slots, sb, [0, 1, 2])
    host_db = KeyFrameDatabase(8, cap)
    for i, (w, v) in enumerate(bows):
        host_db.add(i, w, v)
    q = bows[0]
    a, b = db.query(*q), host_db.query(*q)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    _assert_query(a, q, bows)
    # the explicit capacity gives the same section offsets as the header
    db2 = KeyFrameDatabase(8, cap)
    db2.add_slots_device(slots, sb, [0, 1, 2], cap=cap)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(db2.query(*q), a))
    nc, sc, fw = db.query_slots_device(slots, sb, 3)
    torch.cuda.synchronize()
    for r in range(3):
        single = db.query(*bows[r])
        got = db.compact(nc[r], sc[r], fw[r])
        for x, y in zip(got, single):
            assert x.tobytes() == y.tobytes(), r
        _assert_query(got, bows[r], bows)
    assert not db.check_error()
    for d in (db, db2, host_db):
        d.close()


def test_bad_device_input():
    """A count above word_stride and a descending word pair: the error flag is raised, the entries are empty, the
    other entries of the same query stay bit-exact."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(15)
    stride = 64
    db = KeyFrameDatabase(8, stride)
    good = []
    for n in (64, 10, 33):
        w = np.sort(rng.choice(200, n, replace=False)).astype(np.uint32)
        good.append((w, _norm(rng.uniform(0.1, 8.0, n))))
    long_w = np.arange(128, dtype=np.uint32)  # 128 valid words behind the pointer, count 65 > word_stride
    long_v = np.full(128, 1.0 / 128)
    desc_w = good[1][0].copy()
    desc_w[[4, 5]] = desc_w[[5, 4]]
    empty = (np.zeros(0, np.uint32), np.zeros(0))
    plan = [good[0], (long_w, long_v, 65), good[1], (desc_w, good[1][1], len(desc_w)), good[2]]
    keep = []
    for i, e in enumerate(plan):
        n = e[2] if len(e) == 3 else len(e[0])
        t = (_cuda(torch, e[0]), _cuda(torch, e[1]), _cuda(torch, np.array([n], np.int32)))
        keep.append(t)
        db.add_device(i, *t)
    assert db.check_error(), "the device add must flag its bad input"
    assert not db.check_error(), "the flag is cleared by reading it"
    stored = [good[0], empty, good[1], empty, good[2]]
    q = (np.arange(200, dtype=np.uint32), _norm(rng.uniform(0.1, 8.0, 200)))
    got = db.query(*q)
    _assert_query(got, q, stored)
    assert got[1][1] == 0 and got[1][3] == 0 and R.bits(got[2])[1] == NEG_ZERO and R.bits(got[2])[3] == NEG_ZERO
    assert not db.check_error()
    db.close()

"""CPU: the oracle's FeatureVector matchers (oc_search_for_triangulation, oc_search_by_bow_kf_f,
oc_search_by_bow_kf_kf) against the restatements of match_py.py, written from the reference text, on the hand-made
cases of match_cases.py and on random scenes; and, from the restatements' stats, that every hand-made case takes
the exit it was built for. This is where the oracle is judged: the GPU tests only ask kernel == oracle.
"""
import numpy as np
import pytest

import match_cases as mc
import match_py as mp
import oracle_py
from orbamd.matcher import KeyFrameView

f32 = np.float32


def run_py(c, call, _memo={}):
    key = (c.name, call["key"])
    if key not in _memo:
        v1, v2 = c.views()
        st = mp.MatchStats(v1.n)
        if call["kind"] == "tri":
            n, m = mp.search_for_triangulation_py(v1, v2, c.F12, c.ex, c.ey, call["only_stereo"], call["check_ori"], st)
        elif call["kind"] == "bow0":
            n, m = mp.search_by_bow_kf_f_py(v1, v2, call["nnratio"], call["check_ori"], st)
        else:
            n, m = mp.search_by_bow_kf_kf_py(v1, v2, call["nnratio"], call["check_ori"], st)
        _memo[key] = (n, m, st)
    return _memo[key]


def _case(g, name):
    return next(c for c in mc.group(g) if c.name == name)


def _stats(g, name, key=None):
    c = _case(g, name)
    call = next(k for k in c.calls if key is None or k["key"] == key)
    return c, run_py(c, call)[2].d


@pytest.mark.parametrize("g", list(mc.GROUPS))
def test_match_cases_oracle_matches_restatement(g):
    ncalls = 0
    for c in mc.group(g):
        for call in c.calls:
            n, m, _ = run_py(c, call)
            no, mo = mc.oracle_result(c, call)
            assert n == no == int((m >= 0).sum()), (c.name, call["key"])
            np.testing.assert_array_equal(m, mo, err_msg="%s %s" % (c.name, call["key"]))
            ncalls += 1
    assert ncalls >= len(mc.group(g))


@pytest.mark.parametrize("g", list(mc.GROUPS))
def test_match_cases_take_their_exits(g):
    checked = 0
    for c in mc.group(g):
        for call in c.calls:
            n, m, st = run_py(c, call)
            for i in c.expect:
                e, b = c.expected(call, i)
                if e is None:
                    continue
                who = (c.name, call["key"], [k for k, v in c.names.items() if v == i])
                assert st.d["exit"][i] == e, (who, st.d["best"][i], st.d["tested"][i][:4])
                if e == "accepted":
                    kfkf_or_tri = call["kind"] != "bow0"
                    partner = st.d["best"][i][1]
                    assert b is None or partner == b, who
                    assert (m[i] == partner) if kfkf_or_tri else (m[partner] == i), who
                elif call["kind"] != "bow0":
                    assert m[i] == -1, who
                checked += 1
    assert checked > 0 or g == "h"   # group h states histograms, not exits (test_match_cases_rotation)


# ---- group-wide conditions: that the cases sit on the edge they are named for
def test_match_cases_epipolar_threshold():
    for c in mc.group("a"):
        if not c.name.startswith("a_exact"):
            continue
        dsq, s = c.notes["dsq"], c.notes["sigma"]
        th = 3.84 * float(s)
        at = c.name.endswith("_at")
        nxt = float(np.nextafter(f32(dsq), f32(np.inf), dtype=f32))
        assert (dsq < th <= nxt) if at else (th <= dsq and 3.84 * float(mc.up(s)) > dsq)
        if at and dsq == 49.0:   # a threshold rounded to the nearest float would be 49 and reject dsqr = 49
            assert f32(th) == f32(dsq)
        d = run_py(c, c.calls[0])[2].d
        for i in c.expect:
            (idx2, pos, dist, what, dsqr, tht), = d["tested"][i]
            assert dsqr == f32(dsq) and tht == th and what == ("ok" if at else "epi_fail")
    for c in mc.group("a"):
        if c.name.startswith("a_general"):
            d = run_py(c, c.calls[0])[2].d
            v2 = c.views()[1]
            ins = [i for n, i in c.names.items() if n.endswith("_in")]
            outs = [i for n, i in c.names.items() if n.endswith("_out")]
            assert len(ins) == len(outs) >= 1
            for i, o in zip(ins, outs):   # adjacent floats of y2, the same x2 and octave, opposite decisions
                ci, co = d["tested"][i][0][0], d["tested"][o][0][0]
                assert mc.up(v2.y[ci]) == v2.y[co] and v2.x[ci] == v2.x[co] and v2.octave[ci] == v2.octave[co]
                assert float(d["tested"][i][0][4]) < d["tested"][i][0][5] <= float(d["tested"][o][0][4])
    octs = {(len(c.scale), o) for c in mc.group("a") for o in c.k2.o}
    assert {(8, 0), (8, 3), (8, 7), (1, 0), (16, 15)} <= octs


def test_match_cases_den_zero():
    c, d = _stats("b", "b_F_zero")
    assert all(t[3] == "den0" for i in c.expect for t in d["tested"][i]) and all(d["tested"][i] for i in c.expect)
    c, d = _stats("b", "b_one_position")
    kinds = {n: [t[3] for t in d["tested"][i]] for n, i in c.names.items()}
    assert kinds["den0"] == ["den0"] and all(k == ["ok"] for n, k in kinds.items() if n != "den0")
    a, b, _ = mp.epipolar_line_py(300.0, 100.0, c.F12)
    assert a == 0 and b == 0


def test_match_cases_epipole_radius():
    c, d = _stats("c", "c_exact")
    kinds = {n: [t[3] for t in d["tested"][i]] for n, i in c.names.items()}
    assert kinds == {"on_radius": ["ok"], "inside": ["near", "ok"], "inside_only": ["near"]}
    assert f32(100) * c.scale[0] == f32(100)
    c, d = _stats("c", "c_scale12")
    assert mc.up(c.notes["xa"]) == c.notes["xb"] and f32(f32(100) * c.scale[1]) != np.floor(f32(100) * c.scale[1])
    assert [t[3] for t in d["tested"][c.names["in"]]] == ["near", "ok"]
    assert [t[3] for t in d["tested"][c.names["out"]]] == ["ok"]
    c, d = _stats("c", "c_stereo", "tri")
    near = {n for n, i in c.names.items() if d["tested"][i][0][3] == "near"}
    assert near == {"qm_cm"}   # only the monocular pair meets the radius test; -0.0 >= 0 counts as stereo
    v1, v2 = c.views()
    assert {float(u) for u in v1.uright} >= {-1.0, 0.0, 250.0} and np.signbit(v1.uright).sum() > (v1.uright == -1).sum()


def test_match_cases_hamming_and_ties():
    c, d = _stats("d", "d_hamming")
    i = c.names
    assert [d["best"][i[k]][0] for k in ("d49", "d50", "d0")] == [49, 50, 0]
    assert len(d["ties"][i["tie2"]]) == 2 and len(d["ties"][i["tie3"]]) == 3 and len(d["ties"][i["tie16"]]) == 16
    assert d["better_rejected"][i["bad_before"]] == 1 and d["better_rejected"][i["bad_after"]] == 1
    assert [t[3] for t in d["tested"][i["bad_tie_later"]]] == ["ok", "epi_fail"]
    dec = d["decisive"][i["all_bad"]]   # the D = 4 candidate, 200 rows off the line
    assert dec[1] == f32(200.0 * 200.0) and dec[1] >= dec[2]


def test_match_cases_mfma_structure():
    for form in ("m", "s"):
        cases = [c for c in mc.group("e") if c.name.startswith("e" + form)]
        assert cases[0].k2.n == 0 and cases[0].k1.n > 0   # the empty candidate frame leads its batch
        n2s = {c.k2.n for c in cases if c.k1.n == 33}
        n1s = {c.k1.n for c in cases if c.k2.n == 129}
        assert n2s >= set(mc.E_N2) and n1s >= set(mc.E_N1)
        straddled, won = set(), set()
        for c in cases:
            d = run_py(c, c.calls[0])[2].d
            for i in c.expect:
                if d["exit"][i] != "accepted":
                    continue
                ties = d["ties"][i]
                won.add(ties[-1])
                if c.k2.n - 1 == ties[-1]:
                    won.add("last")
                if len(ties) == 2 and tuple(ties) in mc.E_STRADDLE:
                    straddled.add(tuple(ties))
            if "walk" in c.names:   # the k best fail the geometry, all in rows of one lane; then the winner
                w = c.names["walk"]
                k, winner = c.notes["k"], c.notes["winner"]
                assert d["better_rejected"][w] == k and d["best"][w] == (20, winner)
                rows = sorted(t[1] for t in d["tested"][w] if t[3] == "epi_fail")
                assert rows == sorted(mc.E_LANE_ROWS[:k])
                if k == 16:   # the lane ran dry: the winner lies in the other half, the next tile or the next chunk
                    assert winner not in mc.E_LANE_ROWS
            if "zero" in c.names:
                z = c.names["zero"]
                assert not c.k1.d[z].any() and c.k2.n == 33 and d["best"][z][0] in (0, 10)
        assert straddled == set(mc.E_STRADDLE)
        assert won >= set(mc.E_WIN) | {"last"}
        walks = {(c.notes["k"], c.notes["winner"] // 32) for c in cases if "walk" in c.names}
        assert walks == {(1, 0), (2, 0), (15, 0), (16, 0), (16, 1), (16, 2)}


def _dispatch(c):
    """what matcher.cpp's tri_common looks at: the largest candidate node among the common nodes, the number of
    64-query tasks, and the FeatureVector entries of each side"""
    v1, v2 = c.views()
    ids2 = {int(n): k for k, n in enumerate(v2.node_id)}
    max_nc = tasks = 0
    for k1, n in enumerate(v1.node_id):
        if int(n) in ids2:
            k2 = ids2[int(n)]
            max_nc = max(max_nc, int(v2.node_off[k2 + 1] - v2.node_off[k2]))
            tasks += -(-int(v1.node_off[k1 + 1] - v1.node_off[k1]) // 64)
    return max_nc, tasks, int(v1.node_off[-1]), int(v2.node_off[-1])


def test_match_cases_dispatch_sizes():
    seen = {}
    for c in mc.group("f"):
        max_nc, tasks, e1, e2 = _dispatch(c)
        small = max_nc <= 256 and tasks <= 160 and e1 <= 2048 and e2 <= 2048
        seen[c.name] = (max_nc, tasks, e1, e2, small)
        d = run_py(c, c.calls[0])[2].d
        acc = [i for i in c.expect if d["exit"][i] == "accepted"]
        assert acc and "has_mp" in d["exit"] or not c.name.startswith("f_nc")
        assert "no_common_node" in d["exit"] or not c.name.startswith("f_nc")
        if not small:   # k_tri_nodes: four waves scan the quarters j mod 4 of 256-candidate rounds
            ties = [d["ties"][i] for i in acc if len(d["ties"][i]) == 2]
            assert any(a % 4 != b % 4 for a, b in ties), c.name
            assert any(d["ties"][i][-1] % 4 != 0 for i in acc), c.name
            if max_nc > 256:
                assert any(a // 256 != b // 256 for a, b in ties), c.name
    assert [seen["f_nc%d" % n][0] for n in (1, 63, 64, 65, 255, 256, 257, 513)] == [1, 63, 64, 65, 255, 256, 257, 513]
    assert [seen["f_nc%d" % n][4] for n in (256, 257, 513)] == [True, False, False]
    assert seen["f_161_nodes"][1] == 161 and not seen["f_161_nodes"][4]
    assert seen["f_2049_entries"][3] == 2049 and seen["f_2049_entries"][0] <= 256 and not seen["f_2049_entries"][4]
    for c in mc.group("f"):   # the MapPoint on the candidate side removed a candidate some query would have taken
        if c.name.startswith("f_nc") and c.notes["nc"] >= 3:
            assert any(c.k2.mp)


def test_match_cases_bow_rules():
    c = _case("g", "g_th_low")
    d0, d1 = run_py(c, c.calls[0])[2].d, run_py(c, c.calls[1])[2].d
    i = c.names
    assert d0["best"][i["single"]][2] == 256 and d0["best"][i["equal0"]][::2] == (0, 0)
    assert d0["best"][i["dup_later"]][::2] == (10, 10) and d0["best"][i["first_min"]][::2] == (10, 20)
    assert d0["best"][i["second_no_mp"]][2] == 11 and d1["best"][i["second_no_mp"]][2] == 40
    assert len(d1["ineligible"][i["second_bad"]]) == 1 and len(d1["ineligible"][i["no_cand_mp"]]) == 2
    decided = {}
    for c in mc.group("g"):
        if c.name.startswith("g_ratio"):
            d = run_py(c, c.calls[0])[2].d
            for n, q in c.names.items():
                decided[(c.notes["ratio"], d["best"][q][0], d["best"][q][2])] = (d["exit"][q], d["ratio"][q])
    # what the float comparison decides: 30 < 0.75f * 40 = 30 fails and (30, 41) passes; 0.6f lies above 0.6 and
    # 0.6f * 50 rounds up to the float after 30, so (30, 50) passes; 0.7f and 0.9f lie below 0.7 and 0.9 and their
    # products round to 35 and 45 exactly, so those two fail
    assert {k: v[0] for k, v in decided.items()} == {
        (0.75, 30, 40): "ratio_fail", (0.75, 30, 41): "accepted", (0.6, 30, 50): "accepted",
        (0.7, 35, 50): "ratio_fail", (0.9, 45, 50): "ratio_fail"}
    assert decided[(0.6, 30, 50)][1] == (f32(30), mc.up(30.0)) and decided[(0.7, 35, 50)][1] == (f32(35), f32(35))
    for c in mc.group("g"):
        if c.name.startswith("g_greedy"):
            for call in c.calls:
                d = run_py(c, call)[2].d
                for node in {0, 1} & set(c.k1.node):
                    a, b = c.names["A%d" % node], c.names["B%d" % node]
                    assert d["skipped"][b] == [d["best"][a][1]] and d["best"][b][0] == 12 and d["best"][b][2] == 40
                    pos = sorted(i for i, nd in enumerate(c.k1.node) if nd == node)
                    if c.notes["nq"] > 64:   # A is the last query of the first 64-query chunk, B the first of the next
                        assert (pos.index(a), pos.index(b)) == (63, 64)
    c = _case("g", "g_exhausted")
    for call in c.calls:
        d = run_py(c, call)[2].d
        assert [len(d["skipped"][c.names["q%d" % k]]) for k in range(5)] == [0, 1, 2, 3, 3]


def test_match_cases_rotation():
    for c in mc.group("h"):
        for call in c.calls:
            n, m, st = run_py(c, call)
            d = st.d
            assert d["hist"] is not None and sum(d["hist"]) == len(c.rots or [])
            name = c.name.replace("_trin", "").replace("_tri", "")
            h = sorted(d["hist"], reverse=True)
            kept = [b for b in d["kept_bins"] if b >= 0]
            if name == "h_values":
                ps = [float(d["rot"][i][1]) for i in c.expect]
                assert any(p % 1 == 0.5 and int(p) % 2 == 0 for p in ps)   # roundf and rintf part on these
                bins = [d["rot"][i][0] for i in c.expect]
                assert bins[:7] == [1, 2, 12, 12, 0, 0, 12] and bins[7] == 1 and bins[8] == 3
            elif name == "h_tie_first":
                assert h[:4] == [4, 4, 4, 4] and kept == [2, 5, 9] and n == 12
            elif name == "h_tie_second":
                assert kept == [1, 4, 7] and n == 12
            elif name == "h_tie_third":
                assert kept == [1, 4, 7] and n == 13
            elif name == "h_cut_10_1":   # the float product rounds to 1; left unrounded (in double) it would cut the bin
                assert kept == [3, 6] and n == 11 and float(f32(0.1)) * 10 > 1 and f32(0.1) * f32(10) == f32(1)
            elif name == "h_cut_20_1_2":
                assert kept == [3, 8] and n == 22
            elif name == "h_cut_20_2_1":
                assert kept == [3, 6] and n == 22
            elif name == "h_cut_11_1":
                assert kept == [3] and n == 11
            elif name == "h_single_bin":
                assert kept == [12] and n == 5
            else:
                assert name == "h_none" and kept == [] and n == 0
            assert ("rot_removed" in d["exit"]) == (n < sum(d["hist"]))


# ---- random scenes
def _random_view(rng, n, nodes, node_ids, scale, stereo_frac, mp_frac, bad_frac, pool):
    k = np.zeros(n, mc.KP)
    k["x"], k["y"] = rng.uniform(0, 640, n).astype(f32), rng.uniform(80, 120, n).astype(f32)
    k["angle"] = rng.choice([0.0, 15.0, 30.0, 44.99, 200.0, 345.0, 359.9], n).astype(f32)
    k["octave"] = rng.integers(0, len(scale), n)
    # descriptors near a small pool, so that distances fall on both sides of TH_LOW and tie
    d = pool[rng.integers(0, len(pool), n)].copy()
    for i in range(n):
        for p in rng.permutation(256)[:rng.integers(0, 40)]:
            d[i, p >> 3] ^= np.uint8(1 << (p & 7))
    fv = {int(i): [] for i in node_ids}
    for i in range(n):
        fv[int(node_ids[rng.integers(0, len(node_ids))])].append(i)
    fv = {a: b for a, b in fv.items() if b}
    ur = np.where(rng.random(n) < stereo_frac, rng.uniform(0, 600, n), -1).astype(f32)
    return KeyFrameView(k, d, scale, (scale * scale).astype(f32), feat_vec=fv, uright=ur,
                        has_mp=rng.random(n) < mp_frac, mp_bad=rng.random(n) < bad_frac)


@pytest.mark.parametrize("seed", range(6))
def test_random_scenes_oracle_matches_restatement(seed):
    rng = np.random.default_rng([522655, seed])
    scale = mc.scale_table(8)
    pool = rng.integers(0, 256, (12, 32)).astype(np.uint8)
    ids = np.sort(rng.choice(1000, 9, replace=False))
    n1, n2 = int(rng.integers(40, 160)), int(rng.integers(40, 160))
    F12, ex, ey = mc.default_f12()
    accepted = 0
    for mp_frac in (0.3, 0.8):
        v1 = _random_view(rng, n1, 9, ids[:7], scale, 0.4, mp_frac, 0.1, pool)
        v2 = _random_view(rng, n2, 9, ids[2:], scale, 0.4, mp_frac, 0.1, pool)
        for F, e in ((mc.F_ROW, mc.FAR), (F12, (ex, ey)), (mc.F_ROW, (300.0, 100.0))):
            for only_stereo in (False, True):
                for ori in (False, True):
                    n, m = mp.search_for_triangulation_py(v1, v2, F, e[0], e[1], only_stereo, ori)
                    no, mo = oracle_py.search_for_triangulation(v1, v2, F, float(e[0]), float(e[1]), only_stereo, ori)
                    assert n == no
                    np.testing.assert_array_equal(m, mo)
                    accepted += n
        for ratio in (0.6, 0.7, 0.75, 0.9):
            for ori in (False, True):
                for kfkf, fn in ((False, mp.search_by_bow_kf_f_py), (True, mp.search_by_bow_kf_kf_py)):
                    n, m = fn(v1, v2, ratio, ori)
                    no, mo = oracle_py.search_by_bow(v1, v2, ratio, ori, other_is_keyframe=kfkf)
                    assert n == no
                    np.testing.assert_array_equal(m, mo)
                    accepted += n
    assert accepted > 0

"""CPU: the oracle's Frame-level restatements (oracle/orb_oracle_frame.c) against independent
numpy/pure-Python restatements written from the reference text.

Frame::ComputeStereoMatches (ORB_SLAM2.1/src/Frame.cc:470-641) is restated below line by line
with float32 scalars; parity with the reference itself is unpinned (OpenCV absent).
"""
import numpy as np
import pytest

import oracle_py
import orbamd

f32 = np.float32


def roundf(v):
    """C roundf (half away from zero) for v >= 0; v - floor(v) is exact for floats."""
    fl = np.floor(v)
    return f32(fl + (1 if v - fl >= 0.5 else 0))


def stereo_py(ol, orr, kl, dl, kr, dr, mbf, mb, stats=None):
    """Pure-Python restatement of Frame::ComputeStereoMatches (Frame.cc:470-641). `stats` (a dict) receives the
    exit each left keypoint took ("exit": list of names, "count": exit -> number) and what the scene exercised:
    hamming_tie, sad_tie, deltaR_nz, branch_001, matched_level / kept_level (per pyramid level), max_sad (the
    largest L1 distance evaluated at any shift), median, th_dist."""
    tabs = ol.tables()
    scale, inv = tabs["scale"], tabs["inv_scale"]
    N = len(kl)
    st = {"exit": ["?"] * N, "count": {}, "hamming_tie": 0, "sad_tie": 0, "deltaR_nz": 0, "branch_001": 0,
          "matched_level": [0] * 8, "kept_level": [0] * 8, "max_sad": 0, "median": None, "th_dist": None}

    def leave(i, name):
        st["exit"][i] = name
        st["count"][name] = st["count"].get(name, 0) + 1

    ur = np.full(N, -1, np.float32)
    dp = np.full(N, -1, np.float32)
    nRows = ol.level_size(0)[1]
    rows = [[] for _ in range(nRows)]
    for iR in range(len(kr)):
        y = f32(kr["y"][iR])
        r = f32(2.0) * scale[kr["octave"][iR]]
        maxr = int(np.ceil(f32(y + r)))
        minr = int(np.floor(f32(y - r)))
        for yi in range(minr, maxr + 1):
            if 0 <= yi < nRows:  # outside is undefined behaviour in the reference
                rows[yi].append(iR)
    maxD = f32(mbf) / f32(mb)
    pyrL = [ol.pyramid(l) for l in range(8)]
    pyrR = [orr.pyramid(l) for l in range(8)]
    hd = np.unpackbits(dl, axis=1)
    hr = np.unpackbits(dr, axis=1)
    vdi = []
    for iL in range(N):
        lev = int(kl["octave"][iL])
        vL, uL = f32(kl["y"][iL]), f32(kl["x"][iL])
        cand = rows[int(vL)]
        if not cand:
            leave(iL, "no_cand")
            continue
        minU, maxU = f32(uL - maxD), uL
        best, bestR, nbest = 100, 0, 0
        for iR in cand:
            o = int(kr["octave"][iR])
            if o < lev - 1 or o > lev + 1:
                continue
            uR = f32(kr["x"][iR])
            if minU <= uR <= maxU:
                d = int(np.count_nonzero(hd[iL] != hr[iR]))
                if d < best:
                    best, bestR, nbest = d, iR, 1
                elif d == best:
                    nbest += 1
        if best >= 75:
            leave(iL, "hamming")
            continue
        st["hamming_tie"] += nbest > 1
        sf = inv[lev]
        suL = roundf(f32(uL * sf))
        svL = roundf(f32(vL * sf))
        suR0 = roundf(f32(f32(kr["x"][bestR]) * sf))
        PL, PR = pyrL[lev], pyrR[lev]
        r0, c0 = int(svL) - 5, int(suL) - 5
        assert r0 >= 0 and c0 >= 0 and r0 + 11 <= PL.shape[0] and c0 + 11 <= PL.shape[1], "the reference throws"
        IL = PL[r0:r0 + 11, c0:c0 + 11].astype(np.int64)
        IL = IL - IL[5, 5]
        if suR0 < 0 or suR0 + 11 >= PR.shape[1]:
            leave(iL, "right_edge")
            continue
        assert suR0 >= 10, "the reference throws"
        vd = []
        for inc in range(-5, 6):
            cc = int(suR0) + inc - 5
            IR = PR[r0:r0 + 11, cc:cc + 11].astype(np.int64)
            IR = IR - IR[5, 5]
            vd.append(int(np.abs(IL - IR).sum()))
        st["max_sad"] = max(st["max_sad"], max(vd))
        bi = int(np.argmin(vd))  # first minimum, like `dist < bestDist`
        if bi in (0, 10):
            leave(iL, "end_shift")
            continue
        st["sad_tie"] += vd.count(vd[bi]) > 1
        d1, d2, d3 = f32(vd[bi - 1]), f32(vd[bi]), f32(vd[bi + 1])
        deltaR = f32(f32(d1 - d3) / f32(f32(2) * f32(f32(d1 + d3) - f32(2) * d2)))
        if deltaR < -1 or deltaR > 1:
            leave(iL, "deltaR_range")
            continue
        bestuR = f32(scale[lev] * f32(f32(suR0 + f32(bi - 5)) + deltaR))
        disp = f32(uL - bestuR)
        if disp >= 0 and disp < maxD:
            if disp <= 0:
                disp = f32(0.01)
                bestuR = f32(float(uL) - 0.01)
                st["branch_001"] += 1
            dp[iL] = f32(f32(mbf) / disp)
            ur[iL] = bestuR
            vdi.append((vd[bi], iL))
            st["deltaR_nz"] += deltaR != 0
            st["matched_level"][lev] += 1
            leave(iL, "kept")
        else:
            leave(iL, "neg_disp" if disp < 0 else "maxD")
    vdi.sort()
    kept = len(vdi)
    if vdi:
        med = f32(vdi[len(vdi) // 2][0])
        th = f32(f32(f32(1.5) * f32(1.4)) * med)
        st["median"], st["th_dist"] = float(med), float(th)
        for d, i in reversed(vdi):
            if f32(d) < th:
                break
            ur[i] = dp[i] = -1
            kept -= 1
            st["count"]["kept"] -= 1
            leave(i, "median_rej")
    for i in range(N):
        if st["exit"][i] == "kept":
            st["kept_level"][int(kl["octave"][i])] += 1
    if stats is not None:
        stats.update(st)
    return ur, dp, kept


@pytest.mark.parametrize("W,H,nf,dx,agent", [(752, 480, 1200, 8, 0), (640, 480, 1000, 3, 2),
                                             (1241, 376, 2000, 20, 1)])
def test_stereo_oracle_matches_restatement(W, H, nf, dx, agent):
    L = orbamd.synth_frames(agent, 4, 1, W, H)[0]
    R = orbamd.synth_frames(agent, 4, 1, W, H, dx=dx)[0]
    ol = oracle_py.OracleExtractor(nf, 1.2, 8, 20, 7)
    orr = oracle_py.OracleExtractor(nf, 1.2, 8, 20, 7)
    kl, dl = ol(L)
    kr, dr = orr(R)
    mbf, mb = 47.90639384423901, 0.11
    ur, dp, n = oracle_py.compute_stereo_matches(ol, orr, kl, dl, kr, dr, mbf, mb)
    ur2, dp2, n2 = stereo_py(ol, orr, kl, dl, kr, dr, mbf, mb)
    assert n == n2 and n > len(kl) // 4
    np.testing.assert_array_equal(ur.view(np.uint32), ur2.view(np.uint32))
    np.testing.assert_array_equal(dp.view(np.uint32), dp2.view(np.uint32))
    # a fronto-parallel scene at disparity dx: the kept matches sit within a pixel of it
    v = ur >= 0
    assert np.abs((kl["x"][v] - ur[v]) - dx).max() < 2.5


def test_stereo_oracle_no_right_keypoints():
    W, H = 640, 480
    L = orbamd.synth_frames(0, 0, 1, W, H)[0]
    ol = oracle_py.OracleExtractor(1000, 1.2, 8, 20, 7)
    orr = oracle_py.OracleExtractor(1000, 1.2, 8, 20, 7)
    kl, dl = ol(L)
    orr(np.full((H, W), 128, np.uint8))  # flat right image: no keypoints
    ur, dp, n = oracle_py.compute_stereo_matches(ol, orr, kl, dl, kl[:0], dl[:0], 40.0, 0.1)
    assert n == 0 and (ur == -1).all() and (dp == -1).all()


# ---- varied disparities and hand-made edge cases (stereo_scenes.py). The coverage conditions are asserted here, from
# the restatement's stats, never from the code under test; the GPU tests run the same scenes (test_gpu_stereo.py).
import stereo_scenes as ss  # noqa: E402

MBF, MB = 47.90639384423901, 0.11


def _same_bits(res, ref):
    assert res[2] == ref[2]
    np.testing.assert_array_equal(res[0].view(np.uint32), ref[0].view(np.uint32))
    np.testing.assert_array_equal(res[1].view(np.uint32), ref[1].view(np.uint32))


@pytest.mark.parametrize("W,seed,bands", ss.BAND_CASES)
def test_stereo_band_scene_oracle_matches_restatement(W, seed, bands):
    L, R = ss.band_scene(seed, W, 240, bands)
    ol = oracle_py.OracleExtractor(500, 1.2, 8, 20, 7)
    orr = oracle_py.OracleExtractor(500, 1.2, 8, 20, 7)
    kl, dl = ol(L)
    kr, dr = orr(R)
    st = {}
    res = stereo_py(ol, orr, kl, dl, kr, dr, MBF, MB, st)
    _same_bits(oracle_py.compute_stereo_matches(ol, orr, kl, dl, kr, dr, MBF, MB), res)
    c = st["count"]
    matched = c["kept"] + c["median_rej"]
    assert c["median_rej"] > 0 and c["end_shift"] > 0 and c["neg_disp"] > 0
    assert st["deltaR_nz"] > 0.9 * matched
    assert min(st["kept_level"]) >= 1
    assert res[2] == c["kept"] >= 0.1 * len(kl)
    assert c.get("deltaR_range", 0) == 0  # |deltaR| <= 0.5 always (module docstring of test_gpu_stereo.py)


def test_stereo_band_scene_left_image_is_shared():
    """BANDS and BANDS_ALT give two right images for one left image (the batch test pairs it with both)"""
    for W, seed in ss.BAND_SHARED_SEED.items():
        assert (W, seed, ss.BANDS) in ss.BAND_CASES and (W, seed, ss.BANDS_ALT) in ss.BAND_CASES
        a, b = ss.band_scene(seed, W, 240, ss.BANDS), ss.band_scene(seed, W, 240, ss.BANDS_ALT)
        assert (a[0] == b[0]).all() and (a[1] != b[1]).any()


@pytest.fixture(scope="module", params=[320, 323, 376, 375])
def directed(request):
    c = ss.directed_cases(request.param, 240)
    ol = oracle_py.OracleExtractor(500, 1.2, 8, 20, 7)
    orr = oracle_py.OracleExtractor(500, 1.2, 8, 20, 7)
    ol(c["left"])
    orr(c["right"])
    return c, ol, orr


def test_stereo_directed_tables(directed):
    c, ol, _ = directed
    scale, inv, sizes = ss.tables(c["left"].shape[1], 240)
    np.testing.assert_array_equal(ol.tables()["scale"], scale)
    np.testing.assert_array_equal(ol.tables()["inv_scale"], inv)
    assert [ol.level_size(l) for l in range(8)] == sizes
    assert any(w % 4 for w, _ in sizes[1:])  # a level above 0 whose width is no multiple of 4
    kl, kr = c["kl"], c["kr"]
    for k in (kl, kr):  # every input valid
        assert (k["octave"] >= 0).all() and (k["octave"] < 8).all()
        assert (k["x"] >= 0).all() and (k["x"] <= c["left"].shape[1] - 1).all()
        assert (k["y"] >= 0).all() and (k["y"] <= 239).all()
    assert len(kr) > len(kl) and len(kl) % 16 != 0


def test_stereo_directed_oracle_matches_restatement(directed):
    c, ol, orr = directed
    st = {}
    res = stereo_py(ol, orr, c["kl"], c["dl"], c["kr"], c["dr"], c["mbf"], c["mb"], st)
    _same_bits(oracle_py.compute_stereo_matches(ol, orr, c["kl"], c["dl"], c["kr"], c["dr"], c["mbf"], c["mb"]), res)
    for i, name in enumerate(c["names"]):
        assert st["exit"][i] in c["expect"][name], "%s ended in %s" % (name, st["exit"][i])
    assert st["max_sad"] == 61200  # 120 * 510, 33 150 of it in one 16-bit half
    assert st["branch_001"] == 1 and st["hamming_tie"] == 2 and st["sad_tie"] == 1
    assert st["count"].get("deltaR_range", 0) == 0
    # 1.5f * 1.4f * 10 lies half-way between 21 and the float below it and rounds to 21: sad_21 is not < it, sad_20 is
    assert st["median"] == 10 and 20 < st["th_dist"] <= 21
    assert res[2] == st["count"]["kept"] > 0
    ur, dp = res[0], res[1]
    i = c["names"].index("branch001")
    assert ur[i] == f32(float(c["kl"]["x"][i]) - 0.01) and dp[i] == f32(f32(c["mbf"]) / f32(0.01))
    x = {n: float(c["kl"]["x"][j]) - float(ur[j]) for j, n in enumerate(c["names"])}  # disparities
    assert abs(x["hamming_tie"] - 4) < 0.5 and abs(x["many_cands"] - 4) < 0.5  # the lower iR of the tie, not the 28 px copy
    assert abs(x["sad_tie_first"] - 6) < 0.5  # shift 3 of the tied 3, 5, 7, 9
    assert abs(x["uR_eq_minU"] - 39) < 0.5 and abs(x["uR_eq_maxU"] - 2) < 0.5
    assert abs(x["shift_1"] - 6) < 0.5 and abs(x["shift_9"] - 6) < 0.5 and abs(x["border_right"] - 6) < 0.5
    # the second trip of 64 candidates: many_cands has more than 64 right keypoints in the buckets of its band
    j = c["names"].index("many_cands")
    r = f32(2.0) * ol.tables()["scale"][c["kr"]["octave"]]
    minr = np.floor(c["kr"]["y"] - r)
    v = int(c["kl"]["y"][j])
    assert np.count_nonzero((minr <= v) & (minr >= v - 4)) > 64


@pytest.mark.parametrize("name", sorted(ss.MEDIAN_SUBSETS))
def test_stereo_directed_median_subsets(directed, name):
    c, ol, orr = directed
    names, median, kept = ss.MEDIAN_SUBSETS[name]
    kl, dl = ss.subset(c, names)
    st = {}
    res = stereo_py(ol, orr, kl, dl, c["kr"], c["dr"], c["mbf"], c["mb"], st)
    _same_bits(oracle_py.compute_stereo_matches(ol, orr, kl, dl, c["kr"], c["dr"], c["mbf"], c["mb"]), res)
    assert st["median"] == median and res[2] == kept
    assert len(kl) < 16 or len(kl) % 16


def test_stereo_oracle_raises_on_throw_cases(directed):
    c, ol, orr = directed
    cases = ss.throw_cases(c["left"].shape[1], 240)
    assert [t[0] for t in cases] == ["left_window_only", "both"]
    for name, kl, dl, kr, dr in cases:
        with pytest.raises(RuntimeError):
            oracle_py.compute_stereo_matches(ol, orr, kl, dl, kr, dr, c["mbf"], c["mb"])
        # without the offending keypoint the call is fine
        oracle_py.compute_stereo_matches(ol, orr, kl[:-1], dl[:-1], kr, dr, c["mbf"], c["mb"])
    # `both`: the best right keypoint fails Frame.cc:586's iniu / endu test as well
    kr = cases[1][3]
    assert kr["x"][-1] + 11 >= c["left"].shape[1] and cases[0][3]["x"][-1] + 11 < c["left"].shape[1]


# ------------------------------------------------------------------ SearchByProjection
import proj_scenes as ps  # noqa: E402


def grid_py(F):
    """Frame::AssignFeaturesToGrid + PosInGrid (Frame.cc:235-250, 391-401); kept on the view together with the bytes
    it was made from (a 40 000-feature frame is gridded once, not once per call; a changed x or y makes a new grid)"""
    key = (F.n, F.x.tobytes(), F.y.tobytes(), float(F.min_x), float(F.min_y), float(F.grid_w_inv), float(F.grid_h_inv))
    if getattr(F, "_grid_py", (None, None))[0] != key:
        F._grid_py = (key, _grid_py(F))
    return F._grid_py[1]


def _grid_py(F):
    g = {}
    for i in range(F.n):
        px = int(roundf_signed(f32(f32(F.x[i] - F.min_x) * F.grid_w_inv)))
        py = int(roundf_signed(f32(f32(F.y[i] - F.min_y) * F.grid_h_inv)))
        if 0 <= px < 64 and 0 <= py < 48:
            g.setdefault((px, py), []).append(i)
    return g


def roundf_signed(v):
    return roundf(v) if v >= 0 else -roundf(-v)


def area_py(F, g, x, y, r, minL=-1, maxL=-1):
    """Frame::GetFeaturesInArea (Frame.cc:332-389)."""
    x, y, r = f32(x), f32(y), f32(r)
    x0 = max(0, int(np.floor(f32(f32(f32(x - F.min_x) - r) * F.grid_w_inv))))
    if x0 >= 64:
        return []
    x1 = min(63, int(np.ceil(f32(f32(f32(x - F.min_x) + r) * F.grid_w_inv))))
    if x1 < 0:
        return []
    y0 = max(0, int(np.floor(f32(f32(f32(y - F.min_y) - r) * F.grid_h_inv))))
    if y0 >= 48:
        return []
    y1 = min(47, int(np.ceil(f32(f32(f32(y - F.min_y) + r) * F.grid_h_inv))))
    if y1 < 0:
        return []
    check = minL > 0 or maxL >= 0
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for k in g.get((ix, iy), []):
                if check:
                    if F.octave[k] < minL:
                        continue
                    if maxL >= 0 and F.octave[k] > maxL:
                        continue
                if abs(f32(F.x[k] - x)) < r and abs(f32(F.y[k] - y)) < r:
                    out.append(k)
    return out


class _Stats:
    """What a restatement did with each MapPoint i: exit[i] (skipped, depth, out_of_image, dist_range, view_angle,
    no_candidates, th_reject, ratio_reject, accepted, and after the loop overwritten / rot_removed), uv[i] / radius[i]
    / level[i] of the search, ncand[i] = len(vIndices), ranked[i] = [(dist, scan position, idx)] of the candidates that
    pass every per-candidate test but the occupancy one, sorted (what a scan that ignores claims would list),
    occ_seen[i] = the idx of ranked[i] that were occupied at that moment, best[i] / second[i] = (dist, idx) kept by
    the loop, rot[i] = (bin, rot * factor) of an accepted query, hist / kept_bins of the rotation filter."""

    def __init__(self, n):
        self.d = {k: [None] * n for k in ("uv", "radius", "level", "ranked", "occ_seen", "best", "second", "rot")}
        self.d["exit"] = ["?"] * n
        self.d["ncand"] = [0] * n
        self.d["hist"] = None
        self.d["kept_bins"] = None

    def leave(self, i, name):
        self.d["exit"][i] = name

    def search(self, i, u, v, radius, level, ncand):
        self.d["uv"][i], self.d["radius"][i], self.d["level"][i] = (f32(u), f32(v)), f32(radius), level
        self.d["ncand"][i] = ncand

    def cands(self, i, lst, occ):
        """lst: (dist, scan position, idx) in scan order"""
        self.d["ranked"][i] = sorted(lst)
        self.d["occ_seen"][i] = [k for _, _, k in lst if occ[k]]

    def finish(self, match, stats):
        keep = self.d["kept_bins"]
        for i, e in enumerate(self.d["exit"]):
            if e == "accepted" and keep is not None and self.d["rot"][i][0] not in keep:
                self.d["exit"][i] = "rot_removed"
            elif e == "accepted" and match[self.d["best"][i][1]] != i:
                self.d["exit"][i] = "overwritten"  # by a later query, or reset through another query's bin
        self.d["any_occ"] = [bool(o) for o in self.d["occ_seen"]]
        if stats is not None:
            stats.update(self.d)


def local_py(F, mp, th, nnratio, stats=None):
    """ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th) (ORBmatcher.cc:45-129)."""
    g = grid_py(F)
    bits = np.unpackbits(F.desc, axis=1)
    occ = F.occupied.astype(bool).copy() if F.occupied is not None else np.zeros(F.n, bool)
    match = np.full(F.n, -1, np.int32)
    st = _Stats(mp.n)
    nm = 0
    for i in range(mp.n):
        if not mp.track_in_view[i] or (mp.bad is not None and mp.bad[i]):
            st.leave(i, "skipped")
            continue
        lvl = int(mp.track_level[i])
        r = f32(2.5) if float(mp.track_view_cos[i]) > 0.998 else f32(4.0)
        if th != 1.0:
            r = f32(r * f32(th))
        rad = f32(r * F.scale_factors[lvl])
        qb = np.unpackbits(mp.desc[i])
        best, bl, best2, bl2, bi, si = 256, -1, 256, -1, -1, -1
        cand = area_py(F, g, mp.track_proj_x[i], mp.track_proj_y[i], rad, lvl - 1, lvl)
        st.search(i, mp.track_proj_x[i], mp.track_proj_y[i], rad, lvl, len(cand))
        if not cand:
            st.leave(i, "no_candidates")
            continue
        seen = []
        for pos, idx in enumerate(cand):
            if F.uright is not None and F.uright[idx] > 0:
                if abs(f32(mp.track_proj_xr[i] - F.uright[idx])) > rad:
                    continue
            dist = int(np.count_nonzero(bits[idx] != qb))
            if dist < 256:
                seen.append((dist, pos, idx))
            if occ[idx]:  # (the reference tests this first; neither test has a side effect)
                continue
            if dist < best:
                best2, best, bl2, bl, si, bi = best, dist, bl, int(F.octave[idx]), bi, idx
            elif dist < best2:
                bl2, best2, si = int(F.octave[idx]), dist, idx
        st.cands(i, seen, occ)
        st.d["best"][i], st.d["second"][i] = (best, bi), (best2, si)
        if best <= 100:
            if bl == bl2 and f32(best) > f32(f32(nnratio) * f32(best2)):
                st.leave(i, "ratio_reject")
                continue
            match[bi] = i
            occ[bi] = bool(mp.has_obs[i]) if mp.has_obs is not None else False
            nm += 1
            st.leave(i, "accepted")
        else:
            st.leave(i, "th_reject")
    st.finish(match, stats)
    return nm, match


def _mat34(T):
    T = np.asarray(T, np.float32).reshape(4, 4)
    return [[f32(T[r][c]) for c in range(3)] for r in range(3)], [f32(T[r][3]) for r in range(3)]


def _rt_neg(R, t):
    """-R.t() * t: cv::gemm's generic path, double accumulation, one rounding"""
    return [f32(-1.0 * sum(float(R[k][i]) * float(t[k]) for k in range(3))) for i in range(3)]


def _flag(a, i):
    return a is not None and bool(a[i])


from match_py import _rot_filter_py, _rot_push, _three_maxima_py  # noqa: E402,F401


def last_frame_py(F, Tcw, mp, Tl, th, bmono, check_ori, stats=None):
    """ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (ORBmatcher.cc:1328-1470)."""
    hist = [[] for _ in range(30)]
    Rcw, tcw = _mat34(Tcw)
    twc = _rt_neg(Rcw, tcw)  # :1341
    Rlw, tlw = _mat34(Tl)
    tlc = _gemm33_fast(Rlw, twc, tlw)  # :1346
    fwd = bool(tlc[2] > F.b) and not bmono
    bwd = bool(f32(-tlc[2]) > F.b) and not bmono
    g = grid_py(F)
    bits = np.unpackbits(F.desc, axis=1)
    occ = F.occupied.astype(bool).copy() if F.occupied is not None else np.zeros(F.n, bool)
    match = np.full(F.n, -1, np.int32)
    st = _Stats(mp.n)
    st.d["forward"], st.d["backward"], st.d["tlc_z"] = fwd, bwd, tlc[2]
    nm = 0
    for i in range(mp.n):
        if _flag(mp.skip, i):  # :1355-1357
            st.leave(i, "skipped")
            continue
        x3 = _gemm33_fast(Rcw, [f32(c) for c in mp.pos[i]], tcw)
        xc, yc = x3[0], x3[1]
        invzc = f32(1.0 / float(x3[2]))
        if invzc < 0:
            st.leave(i, "depth")
            continue
        u = f32(f32(f32(F.fx * xc) * invzc) + F.cx)
        v = f32(f32(f32(F.fy * yc) * invzc) + F.cy)
        if u < F.min_x or u > F.max_x or v < F.min_y or v > F.max_y:
            st.leave(i, "out_of_image")
            continue
        lo = int(mp.octave[i])
        radius = f32(f32(th) * F.scale_factors[lo])
        if fwd:
            cand = area_py(F, g, u, v, radius, lo)
        elif bwd:
            cand = area_py(F, g, u, v, radius, 0, lo)
        else:
            cand = area_py(F, g, u, v, radius, lo - 1, lo + 1)
        st.search(i, u, v, radius, lo, len(cand))
        if not cand:
            st.leave(i, "no_candidates")
            continue
        qb = np.unpackbits(mp.desc[i])
        best, bi, seen = 256, -1, []
        for pos, i2 in enumerate(cand):
            if F.uright is not None and F.uright[i2] > 0:
                ur = f32(u - f32(F.bf * invzc))
                if abs(f32(ur - F.uright[i2])) > radius:
                    continue
            dist = int(np.count_nonzero(bits[i2] != qb))
            if dist < 256:
                seen.append((dist, pos, i2))
            if occ[i2]:  # (tested first in the reference, :1403-1405)
                continue
            if dist < best:
                best, bi = dist, i2
        st.cands(i, seen, occ)
        st.d["best"][i] = (best, bi)
        if best <= 100:
            match[bi] = i
            occ[bi] = _flag(mp.has_obs, i)
            nm += 1
            st.leave(i, "accepted")
            if check_ori:
                _rot_push(hist, st, i, mp.angle[i], F.angle[bi], bi)
        else:
            st.leave(i, "th_reject")
    if check_ori:
        nm = _rot_filter_py(hist, st, match, nm)
    st.finish(match, stats)
    return nm, match


def keyframe_py(F, Tcw, mp, th, orb_dist, check_ori, stats=None):
    """ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist)
    (ORBmatcher.cc:1472-1599)."""
    Rcw, tcw = _mat34(Tcw)
    Ow = _rt_neg(Rcw, tcw)
    hist = [[] for _ in range(30)]
    g = grid_py(F)
    bits = np.unpackbits(F.desc, axis=1)
    occ = F.occupied.astype(bool).copy() if F.occupied is not None else np.zeros(F.n, bool)
    match = np.full(F.n, -1, np.int32)
    st = _Stats(mp.n)
    nm = 0
    for i in range(mp.n):
        if _flag(mp.skip, i) or _flag(mp.bad, i):  # :1492-1494
            st.leave(i, "skipped")
            continue
        p = [f32(c) for c in mp.pos[i]]
        x3 = _gemm33_fast(Rcw, p, tcw)
        xc, yc = x3[0], x3[1]
        invzc = f32(1.0 / float(x3[2]))  # no sign test here (:1502)
        u = f32(f32(f32(F.fx * xc) * invzc) + F.cx)
        v = f32(f32(f32(F.fy * yc) * invzc) + F.cy)
        if u < F.min_x or u > F.max_x or v < F.min_y or v > F.max_y:
            st.leave(i, "out_of_image")
            continue
        PO = [f32(p[k] - Ow[k]) for k in range(3)]
        d3 = _norm3(PO)
        if d3 < f32(f32(0.8) * f32(mp.min_dist[i])) or d3 > f32(f32(1.2) * f32(mp.max_dist[i])):
            st.leave(i, "dist_range")
            continue
        lvl = _predict_scale(mp.max_dist[i], d3, F)
        radius = f32(f32(th) * F.scale_factors[lvl])
        cand = area_py(F, g, u, v, radius, lvl - 1, lvl + 1)
        st.search(i, u, v, radius, lvl, len(cand))
        if not cand:
            st.leave(i, "no_candidates")
            continue
        qb = np.unpackbits(mp.desc[i])
        best, bi, seen = 256, -1, []
        for pos, i2 in enumerate(cand):
            dist = int(np.count_nonzero(bits[i2] != qb))
            if dist < 256:
                seen.append((dist, pos, i2))
            if occ[i2]:
                continue
            if dist < best:
                best, bi = dist, i2
        st.cands(i, seen, occ)
        st.d["best"][i] = (best, bi)
        if best <= orb_dist:
            match[bi] = i
            occ[bi] = True
            nm += 1
            st.leave(i, "accepted")
            if check_ori:
                _rot_push(hist, st, i, mp.angle[i], F.angle[bi], bi)
        else:
            st.leave(i, "th_reject")
    if check_ori:
        nm = _rot_filter_py(hist, st, match, nm)
    st.finish(match, stats)
    return nm, match


def _decompose_scw(Scw):
    """ORBmatcher.cc:298-303 / 985-990: scw, Rcw = sRcw / scw, tcw = t / scw (convertTo with the float 1 / scw), Ow"""
    Scw = np.asarray(Scw, np.float32).reshape(4, 4)
    scw = f32(np.sqrt(sum(float(Scw[0][c]) * float(Scw[0][c]) for c in range(3))))
    inv = f32(1.0 / float(scw))
    R = [[f32(Scw[r][c] * inv) for c in range(3)] for r in range(3)]
    t = [f32(Scw[r][3] * inv) for r in range(3)]
    return R, t, _rt_neg(R, t)


def sim3proj_py(KF, Scw, mp, th, stats=None):
    """ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, int th) (ORBmatcher.cc:290-403)."""
    Rcw, tcw, Ow = _decompose_scw(Scw)
    g = grid_py(KF)
    bits = np.unpackbits(KF.desc, axis=1)
    occ = KF.occupied.astype(bool).copy() if KF.occupied is not None else np.zeros(KF.n, bool)  # vpMatched[idx]
    match = np.full(KF.n, -1, np.int32)
    st = _Stats(mp.n)
    nm = 0
    for i in range(mp.n):
        if _flag(mp.bad, i) or _flag(mp.skip, i):  # :317
            st.leave(i, "skipped")
            continue
        p = [f32(c) for c in mp.pos[i]]
        pc = _gemm33_fast(Rcw, p, tcw)
        if pc[2] < 0.0:
            st.leave(i, "depth")
            continue
        invz = f32(f32(1) / pc[2])
        x, y = f32(pc[0] * invz), f32(pc[1] * invz)
        u = f32(f32(KF.fx * x) + KF.cx)
        v = f32(f32(KF.fy * y) + KF.cy)
        if not (u >= KF.min_x and u < KF.max_x and v >= KF.min_y and v < KF.max_y):  # KeyFrame::IsInImage
            st.leave(i, "out_of_image")
            continue
        PO = [f32(p[k] - Ow[k]) for k in range(3)]
        d3 = _norm3(PO)
        if d3 < f32(f32(0.8) * f32(mp.min_dist[i])) or d3 > f32(f32(1.2) * f32(mp.max_dist[i])):
            st.leave(i, "dist_range")
            continue
        if _dot3(PO, mp.normal[i]) < 0.5 * float(d3):
            st.leave(i, "view_angle")
            continue
        lvl = _predict_scale(mp.max_dist[i], d3, KF)
        radius = f32(f32(int(th)) * KF.scale_factors[lvl])
        cand = area_py(KF, g, u, v, radius)
        st.search(i, u, v, radius, lvl, len(cand))
        if not cand:
            st.leave(i, "no_candidates")
            continue
        qb = np.unpackbits(mp.desc[i])
        best, bi, seen = 256, -1, []
        for pos, idx in enumerate(cand):
            kl = int(KF.octave[idx])
            if kl < lvl - 1 or kl > lvl:
                continue
            dist = int(np.count_nonzero(bits[idx] != qb))
            if dist < 256:
                seen.append((dist, pos, idx))
            if occ[idx]:  # (tested before the level in the reference, :375)
                continue
            if dist < best:
                best, bi = dist, idx
        st.cands(i, seen, occ)
        st.d["best"][i] = (best, bi)
        if best <= 50:
            match[bi] = i
            occ[bi] = True
            nm += 1
            st.leave(i, "accepted")
        else:
            st.leave(i, "th_reject")
    st.finish(match, stats)
    return nm, match


@pytest.mark.parametrize("seed,stereo,th", [(1, True, 3.0), (2, False, 1.0), (3, True, 5.0)])
def test_projection_local_oracle_matches_restatement(seed, stereo, th):
    F, mps = ps.local_scene(seed, stereo)
    n, m = oracle_py.search_by_projection_local(F, mps, th, 0.8)
    n2, m2 = local_py(F, mps, th, 0.8)
    assert n == n2 and n > F.n // 4
    np.testing.assert_array_equal(m, m2)


@pytest.mark.parametrize("seed,bmono,forward,check_ori,th", [(4, False, 0, True, 7.0), (5, True, 0, True, 15.0),
                                                             (6, False, 1, False, 7.0), (7, False, -1, True, 7.0)])
def test_projection_last_frame_oracle_matches_restatement(seed, bmono, forward, check_ori, th):
    F, Tcw, mps, Tl = ps.last_frame_scene(seed, bmono, not bmono, forward)
    st = {}
    n, m = oracle_py.search_by_projection_last_frame(F, Tcw, mps, Tl, th, bmono, check_ori)
    n2, m2 = last_frame_py(F, Tcw, mps, Tl, th, bmono, check_ori, st)
    assert n == n2 and n > F.n // 4
    np.testing.assert_array_equal(m, m2)
    # (the scene moves the last frame by 0.5 along z for forward = +-1: one of the two directions, never both)
    assert (st["forward"] != st["backward"]) == (forward != 0 and not bmono) and not (st["forward"] and st["backward"])
    assert not check_ori or "rot_removed" in st["exit"]


@pytest.mark.parametrize("seed,th,orb_dist,check_ori", [(5, 10.0, 100, True), (9, 3.0, 64, False),
                                                        (10, 10.0, 100, False)])
def test_projection_keyframe_oracle_matches_restatement(seed, th, orb_dist, check_ori):
    F, Tcw, mps = ps.keyframe_scene(seed)
    n, m = oracle_py.search_by_projection_keyframe(F, Tcw, mps, th, orb_dist, check_ori)
    n2, m2 = keyframe_py(F, Tcw, mps, th, orb_dist, check_ori)
    assert n == n2 and n > F.n // 8
    np.testing.assert_array_equal(m, m2)


@pytest.mark.parametrize("seed,th", [(6, 10), (11, 3)])
def test_projection_sim3_oracle_matches_restatement(seed, th):
    F, Scw, mps = ps.sim3_scene(seed)
    n, m = oracle_py.search_by_projection_sim3(F, Scw, mps, th)
    n2, m2 = sim3proj_py(F, Scw, mps, th)
    assert n == n2 and n > F.n // 8
    np.testing.assert_array_equal(m, m2)


def test_projection_variants_oracle_sanity():
    """one scene per variant (the seeds this test always had): count and every element of the match array equal the
    restatement's, where it used to look at the counts only"""
    F, Tcw, mps, Tl = ps.last_frame_scene(4)
    n, m = oracle_py.search_by_projection_last_frame(F, Tcw, mps, Tl, 7.0, False, True)
    n2, m2 = last_frame_py(F, Tcw, mps, Tl, 7.0, False, True)
    assert n == n2 and n > F.n // 4 and n >= (m >= 0).sum()  # has_obs == 0 claimers can be overwritten (last wins)
    np.testing.assert_array_equal(m, m2)
    F, Tcw, mps = ps.keyframe_scene(5)
    n, m = oracle_py.search_by_projection_keyframe(F, Tcw, mps, 10.0, 100, True)
    n2, m2 = keyframe_py(F, Tcw, mps, 10.0, 100, True)
    assert n == n2 and n > F.n // 4 and n == (m >= 0).sum()  # every claim occupies
    np.testing.assert_array_equal(m, m2)
    F, Scw, mps = ps.sim3_scene(6)
    n, m = oracle_py.search_by_projection_sim3(F, Scw, mps, 10)
    n2, m2 = sim3proj_py(F, Scw, mps, 10)
    assert n == n2 and n > F.n // 8 and n == (m >= 0).sum()
    np.testing.assert_array_equal(m, m2)


# ---- hand-made cases (proj_cases.py): oracle == restatement on every call of every group, and every named case
# takes the exit it is built for (from the restatement's stats, so a case that stops reaching its edge fails here)
import proj_cases as pc  # noqa: E402


def run_py(c, F, mps, st):
    k = c["kind"]
    if k == "local":
        return local_py(F, mps, c["th"], c["nnratio"], st)
    if k == "last":
        return last_frame_py(F, c["Tcw"], mps, c["Tl"], c["th"], c["bmono"], c["check_ori"], st)
    if k == "keyframe":
        return keyframe_py(F, c["Tcw"], mps, c["th"], c["orb_dist"], c["check_ori"], st)
    if k == "sim3":
        return sim3proj_py(F, c["Tcw"], mps, c["th"], st)
    if k == "fuse":
        R, t = _mat34(c["Tcw"])
        return fuse_py(F, mps, c["th"], R, t, c["Ow"], c["inv"], stats=st)
    R, t, Ow = _decompose_scw(c["Tcw"])
    return fuse_py(F, mps, c["th"], R, t, Ow, sim3=True, stats=st)


_py_results = {}


def py_result(gname):
    """[(call, F, mps, (count, array), stats)] of a group, computed once"""
    if gname not in _py_results:
        out = []
        for c, F, mps in pc.group(gname).calls():
            st = {}
            out.append((c, F, mps, run_py(c, F, mps, st), st))
        _py_results[gname] = out
    return _py_results[gname]


@pytest.mark.parametrize("gname", pc.GROUPS)
def test_projection_cases_oracle_matches_restatement(gname):
    g = pc.group(gname)
    for c, F, mps, (n2, m2), st in py_result(gname):
        n, m = pc.run_oracle(c, F, mps)
        bad = np.nonzero(m != m2)[0]
        fuse = c["kind"].startswith("fuse")
        assert bad.size == 0, "oracle %s restatement %s at %s" % (m[bad[:8]], m2[bad[:8]], g.describe(
            c, queries=bad if fuse else [v for v in list(m[bad]) + list(m2[bad]) if v >= 0], feats=() if fuse else bad))
        assert n == n2, "%s/%s: count %d, restatement %d" % (gname, c["key"], n, n2)


@pytest.mark.parametrize("gname", pc.GROUPS)
def test_projection_cases_take_their_exits(gname):
    g = pc.group(gname)
    F = g.frame()
    assert F.n < 65536 and all(0 <= o < 8 for o in F.octave) and np.isfinite(F.x).all() and np.isfinite(F.y).all()
    wrong = []
    for c, F, mps, (n, m), st in py_result(gname):
        names = g.names(c)
        assert len(names) == mps.n and "?" not in st["exit"]
        for i, name in enumerate(names):
            e = g.expected(c, name)
            if e is None:
                continue
            if st["exit"][i] != e:
                wrong.append((c["key"], name, "exit", st["exit"][i], e))
                continue
            b = g.expected(c, name, g.best)
            if b is not None and e in ("accepted", "overwritten", "rot_removed"):
                got = st["best"][i][1]
                if g.fname[got] != b:
                    wrong.append((c["key"], name, "best", g.fname[got], b))
            if gname != "real" and st["level"][i] is not None and st["level"][i] != g.qs[i]["level"]:
                wrong.append((c["key"], name, "level", st["level"][i], g.qs[i]["level"]))
    assert not wrong, wrong
    assert g.name == "real" or any(e is not None for e in g.expect.values())


def _call(gname, key):
    g = pc.group(gname)
    for c, F, mps, res, st in py_result(gname):
        if c["key"] == key:
            return g, c, F, res, st, {n: i for i, n in enumerate(g.names(c))}
    raise KeyError(key)


def test_projection_cases_grid_edges():
    """what the grid group is about, from grid_py: the border cells are populated, the three features that round to
    column 64 / row 48 are in no cell, one cell holds 70 features, x * 0.1f == 10.5 went to column 11"""
    g = pc.group("grid")
    F = g.frame()
    cells = grid_py(F)
    where = {g.fname[i]: cell for cell, lst in cells.items() for i in lst}
    assert where["col0"][0] == 0 and where["col1"][0] == 1 and where["col63"][0] == 63 and where["x634_99"][0] == 63
    assert where["row0"][1] == 0 and where["row1"][1] == 1 and where["row47"][1] == 47 and where["y474_99"][1] == 47
    assert where["cell_3071"] == (63, 47)
    for name in ("x635_dropped", "y475_dropped", "x639_9_dropped"):
        assert name not in where
    assert f32(f32(635.0) * F.grid_w_inv) == f32(63.5) and f32(f32(475.0) * F.grid_h_inv) == f32(47.5)
    assert f32(f32(105.0) * F.grid_w_inv) == f32(10.5) and where["half_A"] == (11, 20) and where["half_B"] == (10, 20)
    assert where["halfy_A"] == (30, 11) and where["halfy_B"] == (30, 10)
    assert len(cells[(30, 30)]) == 70
    # the empty returns and the clamps of GetFeaturesInArea, the whole grid, a window of more than 16 cells
    for key in ("local",):
        _, c, _, _, st, at = _call("grid", key)
        for name in ("out_right", "out_left", "out_below", "out_above"):
            assert st["ncand"][at[name]] == 0
    g2, c, F2, _, st, at = _call("clamp", "local")
    for name, (u, v) in (("clamp_right", (700, 200)), ("clamp_left", (-60, 240)), ("clamp_below", (320, 540)),
                         ("clamp_above", (360, -60))):
        assert st["uv"][at[name]] == (u, v) and st["radius"][at[name]] == 80 and st["ncand"][at[name]] == 1
    _, c, _, _, st, at = _call("wide", "keyframe")
    assert st["radius"][at["wide_0"]] > 640 and st["ncand"][at["wide_0"]] == 4
    assert [k for _, _, k in st["ranked"][at["wide_0"]]] == [3, 2, 1, 0]  # the cell order against the index order
    _, c, _, _, st, at = _call("lanes", "sim3")
    assert [k for _, _, k in st["ranked"][at["lanes_0"]]] == [2, 1, 0]


def test_projection_cases_candidate_edges():
    g, c, F, _, st, at = _call("cand", "fuse")
    chi = {n: float(st["chi2"][at[n]][0][1]) for n in ("chi2_mono_under", "chi2_mono_over", "chi2_stereo_under",
                                                     "chi2_stereo_over")}
    assert 5.9 < chi["chi2_mono_under"] <= 5.99 < chi["chi2_mono_over"] < 6.1
    assert 7.7 < chi["chi2_stereo_under"] <= 7.8 < chi["chi2_stereo_over"] < 7.9
    assert pc.INV_SIGMA2[1] != 1
    i, j = g.fname.index("er_eq_radius"), g.fname.index("er_ulp_over")
    xr = lambda n: g.qs[at[n]]["xr"]
    assert f32(xr("er_eq_radius") - F.uright[i]) == 4 and 4 < f32(xr("er_ulp_over") - F.uright[j]) < 4.00002
    assert F.uright[j] == pc.down(f32(xr("er_ulp_over") - f32(4)))
    assert F.uright[g.fname.index("ur_zero")] == 0 and F.uright[g.fname.index("ur_minus1")] == -1
    _, c, _, _, st, at = _call("cand", "local")
    assert st["ranked"][at["all_256"]] == [] and st["ncand"][at["all_256"]] == 2
    assert st["second"][at["rival_at_256"]] == (256, -1)
    # the ratio group: 0.8f * 75 == 60.0f exactly; the second best of the tie cases
    _, c, _, _, st, at = _call("ratio", "local")
    assert st["best"][at["ratio_eq"]][0] == 60 and st["second"][at["ratio_eq"]][0] == 75
    assert st["best"][at["ratio_over"]][0] == 61 and st["second"][at["single"]] == (256, -1)
    second = lambda n: g2.fname[st["second"][at[n]][1]]
    g2 = pc.group("ratio")
    assert second("tie_50_45_50_first") == "tie_50_45_50_first_0"
    assert second("tie_50_45_50_first_b") == "tie_50_45_50_first_b_0"
    assert second("tie_50_70_60") == "tie_50_70_60_2" and second("tie_5_5_levels") == "tie_5_5_levels_1"
    assert st["radius"][at["viewcos_below"]] == 4 and st["radius"][at["viewcos_0998"]] == 2.5
    _, c, _, _, st2, _ = _call("ratio", "local_th")
    assert st["radius"][at["th_factor"]] == 4 and 4 < st2["radius"][at["th_factor"]] < 4.001


def test_projection_cases_levels_and_front():
    flags = {}
    for k in ("last_fwd", "last_bwd", "last_eq_mb", "last_eq_neg_mb", "last_mono"):
        st = _call("levels", k)[4]
        flags[k] = (st["forward"], st["backward"], float(st["tlc_z"]))
    assert flags == {"last_fwd": (True, False, 0.75), "last_bwd": (False, True, -0.75),
                     "last_eq_mb": (False, False, 0.5), "last_eq_neg_mb": (False, False, -0.5),
                     "last_mono": (False, False, 0.75)}
    assert pc.group("levels").frame().b == f32(0.5)
    g, c, F, _, st, at = _call("front", "keyframe")
    q = lambda n: g.qs[at[n]]
    assert st["uv"][at["u_eq_maxx"]][0] == F.max_x and st["uv"][at["v_eq_maxy"]][1] == F.max_y
    assert q("u_below_0")["u"] < 0 and pc.up(q("u_below_0")["u"]) == 0 and st["uv"][at["u_eq_0"]][0] == 0
    assert q("behind")["pos"][2] < 0 and st["uv"][at["behind"]] == (300, 100)
    assert q("dist_eq_min")["dist"] == f32(f32(0.8) * q("dist_eq_min")["min_dist"]) == 9
    assert q("dist_below_min")["dist"] == pc.down(f32(f32(0.8) * q("dist_below_min")["min_dist"])) == 9
    assert q("dist_eq_max")["dist"] == f32(f32(1.2) * q("dist_eq_max")["max_dist"]) == 17
    assert q("dist_above_max")["dist"] == pc.up(f32(f32(1.2) * q("dist_above_max")["max_dist"])) == 19
    assert _dot3(q("normal_eq_half")["pos"], q("normal_eq_half")["normal"]) == 0.5 * 19
    assert 1.4999 < _dot3(q("normal_below_half")["pos"], q("normal_below_half")["normal"]) < 0.5 * 3
    # nScale = -1 before the clamp, inside the distance test, searched at level 0 by all four variants that predict
    assert pc.raw_scale(q("scale_low")["max_dist"], q("scale_low")["dist"]) == -1
    assert q("scale_low")["dist"] == f32(f32(1.2) * q("scale_low")["max_dist"])
    for key in ("keyframe", "sim3", "fuse", "fuse_sim3"):
        st_k, at_k = _call("front", key)[4], _call("front", key)[5]
        assert st_k["exit"][at_k["scale_low"]] == "accepted" and st_k["level"][at_k["scale_low"]] == 0
    assert pc.raw_scale(q("scale_high")["max_dist"], q("scale_high")["dist"]) > 7 and st["level"][at["scale_high"]] == 7
    e = pc.group("empty")
    assert e.frame().n == 0 and len(e.qs) > 0


def test_projection_cases_arbitration():
    """the claimed entry really is the loser's best (or second), claimer and loser sit where the case says, the
    rescan cases have more than four candidates whose first four are taken"""
    g = pc.group("arb")
    assert g.frame().n == pc.ARB_N and g.fname.index("idx_last_A") == pc.ARB_N - 1
    assert g.fname.index("idx_32768_A") == 32768
    pos = {r["name"]: i for i, r in enumerate(g.qs)}
    assert (pos["adjacent_claimer"], pos["adjacent_loser"]) == (10, 11)
    assert (pos["chunk_edge_claimer"], pos["chunk_edge_loser"]) == (63, 64)
    assert (pos["far_claimer"], pos["far_loser"]) == (5, 200)
    assert pos["collide_2048_1"] == pos["collide_2048_0"] + 1 and pos["collide_2048_1"] // 64 == pos["collide_2048_0"] // 64
    assert pos["collide_4096_1"] == pos["collide_4096_0"] + 1 and pos["collide_4096_1"] // 64 == pos["collide_4096_0"] // 64
    for n, d in (("collide_2048", 2048), ("collide_4096", 4096)):
        assert g.fname.index(n + "_1") - g.fname.index(n + "_0") == d
    for key in ("local", "last", "keyframe", "sim3"):
        _, c, F, (n, m), st, at = _call("arb", key)
        for i in range(len(at)):  # every query is active: position in the list = position in the device batch
            assert st["exit"][i] not in ("skipped", "depth", "out_of_image", "dist_range", "view_angle"), (key, i)
        for loser, claimer, rank in g.pairs:
            if key != "local" and loser in ("second_claimed_loser", "best_claimed_loser"):  # about the ratio test
                continue
            claimed = st["best"][at[claimer]][1]
            assert st["exit"][at[claimer]] == "accepted" and st["ranked"][at[loser]][rank][2] == claimed, (key, loser)
            assert claimed in st["occ_seen"][at[loser]], (key, loser)
        resc = g.rescan + (g.rescan_claiming if key in ("keyframe", "sim3") else [])
        for name in resc:
            r = st["ranked"][at[name]]
            assert len(r) > 4 and all(k in st["occ_seen"][at[name]] for _, _, k in r[:4]), (key, name)
        occ = g.fname.index("occupied_best")
        for k in range(3):
            assert st["ranked"][at["occupied_%d" % k]][0][2] == occ and F.occupied[occ]
        if key in ("local", "last"):
            assert m[g.fname.index("noobs_0")] == at["six_noobs_5"] and n == (m >= 0).sum() + 5
    # the second-entry claim flips a ratio rejection, the best-entry claim causes one (nnratio 0.8)
    _, c, F, _, st, at = _call("arb", "local")
    r = st["ranked"][at["second_claimed_loser"]]
    assert [d for d, _, _ in r] == [50, 55, 90]
    assert f32(50) > f32(f32(0.8) * f32(55)) and not f32(50) > f32(f32(0.8) * f32(90))
    r = st["ranked"][at["best_claimed_loser"]]
    assert [d for d, _, _ in r] == [40, 50, 55]
    assert not f32(40) > f32(f32(0.8) * f32(50)) and f32(50) > f32(f32(0.8) * f32(55))
    for nq in (0, 1, 63, 64, 65):
        assert len(_call("arb", "keyframe_nq%d" % nq)[5]) == nq


def test_projection_cases_rotation():
    g = pc.group("rot")
    _, c, F, (n, m), st, at = _call("rot", "last_nq30")
    assert [st["rot"][i][0] for i in range(30)] == [0] * 20 + [5] * 2 + [9] * 2 + [12] * 2 + [1] * 2 + [7, 0]
    assert st["rot"][26][1] == f32(0.5) and 12 < st["rot"][24][1] < 12.00001  # exactly .5; a negative rot wrapped to 360
    assert g.qs[0]["angle"] == 0 and np.signbit(g.qs[0]["angle"]) and st["rot"][0][1] == 0  # rot = -0.0
    assert f32(g.qs[24]["angle"] - F.angle[24]) < 0
    assert st["hist"][0] == 21 and st["kept_bins"] == [0, -1, -1] and f32(2) < f32(f32(0.1) * f32(21))
    shared = g.fname.index("shared")
    # 30 accepted on 29 features; eight in dropped bins of 2 and the discarded writer are subtracted, the later writer of
    # the shared feature stays counted although the feature is reset
    assert m[shared] == -2 and n == 30 - 9 and (m >= 0).sum() == 29 - 9
    hists = {k: _call("rot", "last_nq%d" % k)[4] for k in (20, 21, 22, 23, 24, 26, 28)}
    assert [h for h in hists[20]["hist"] if h] == [20] and hists[20]["kept_bins"] == [0, -1, -1]  # one bin
    assert hists[21]["kept_bins"] == [0, -1, -1] and hists[22]["kept_bins"] == [0, 5, -1]  # max2 = 1 and 2 against 2.0f
    assert hists[23]["kept_bins"] == [0, 5, -1] and hists[24]["kept_bins"] == [0, 5, 9]  # the same for max3
    assert hists[26]["kept_bins"] == [0, 5, 9] and hists[26]["hist"][12] == 2  # tie: the first index stays
    assert hists[28]["kept_bins"] == [0, 1, 5] and f32(f32(0.1) * f32(20)) == f32(2)
    _, c, _, (n, m), st, at = _call("rot", "keyframe_nq30")
    assert st["exit"][29] == "th_reject" and st["occ_seen"][29] == [shared] and m[shared] == -2

# ------------------------------------------------------------------ Fuse x2 (ORBmatcher.cc:825-1100)
import ctypes as _C  # noqa: E402

_libm = _C.CDLL("libm.so.6")
_libm.logf.restype = _C.c_float
_libm.logf.argtypes = [_C.c_float]


def _gemm33_fast(A, x, c):
    """cv::Mat A*x + c, 3x3 by 3x1 (OpenCV's small-matrix gemm: float products and sums, + c in double)."""
    out = []
    for i in range(3):
        t0 = f32(f32(f32(A[i][0] * x[0]) + f32(A[i][1] * x[1])) + f32(A[i][2] * x[2]))
        out.append(f32(float(t0) + float(c[i])))
    return out


def _norm3(v):
    return f32(np.sqrt(sum(float(a) * float(a) for a in v)))


def _dot3(a, b):
    return sum(float(x) * float(y) for x, y in zip(a, b))


def _predict_scale(max_dist, d, F):
    """MapPoint::PredictScale (MapPoint.cc:385-417), logf of the float ratio."""
    ratio = f32(f32(max_dist) / f32(d))
    n = int(np.ceil(f32(f32(_libm.logf(float(ratio))) / f32(F.log_scale_factor))))
    return min(max(n, 0), len(F.scale_factors) - 1)


def fuse_py(F, mp, th, R, t, Ow, inv=None, sim3=False, stats=None):
    """ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:825-975) or, with sim3, Fuse(pKF, Scw,
    vpPoints, th, vpReplacePoint) (:977-1100): per MapPoint the bestIdx that the reference fuses."""
    g = grid_py(F)
    bits = np.unpackbits(F.desc, axis=1)
    best = np.full(mp.n, -1, np.int32)
    st = _Stats(mp.n)
    st.d["chi2"] = [[] for _ in range(mp.n)]  # (idx, e2 * invSigma2) of the candidates that reach the test
    for i in range(mp.n):
        if _flag(mp.skip, i) or _flag(mp.bad, i):
            st.leave(i, "skipped")
            continue
        p = [f32(v) for v in mp.pos[i]]
        pc = _gemm33_fast(R, p, t)
        if pc[2] < f32(0):
            st.leave(i, "depth")
            continue
        invz = f32(1.0 / float(pc[2])) if sim3 else f32(f32(1) / pc[2])
        u = f32(f32(f32(F.fx) * f32(pc[0] * invz)) + f32(F.cx))
        v = f32(f32(f32(F.fy) * f32(pc[1] * invz)) + f32(F.cy))
        if not (u >= F.min_x and u < F.max_x and v >= F.min_y and v < F.max_y):
            st.leave(i, "out_of_image")
            continue
        ur = f32(u - f32(f32(F.bf) * invz))
        PO = [f32(p[k] - f32(Ow[k])) for k in range(3)]
        d3 = _norm3(PO)
        if d3 < f32(f32(0.8) * f32(mp.min_dist[i])) or d3 > f32(f32(1.2) * f32(mp.max_dist[i])):
            st.leave(i, "dist_range")
            continue
        if _dot3(PO, mp.normal[i]) < 0.5 * float(d3):
            st.leave(i, "view_angle")
            continue
        lvl = _predict_scale(mp.max_dist[i], d3, F)
        rad = f32(f32(th) * f32(F.scale_factors[lvl]))
        qb = np.unpackbits(mp.desc[i])
        bd, bi, seen = 1 << 30, -1, []
        cand = area_py(F, g, u, v, rad)
        st.search(i, u, v, rad, lvl, len(cand))
        if not cand:
            st.leave(i, "no_candidates")
            continue
        for pos, idx in enumerate(cand):
            kl = int(F.octave[idx])
            if kl < lvl - 1 or kl > lvl:
                continue
            if not sim3:
                ex, ey = f32(u - F.x[idx]), f32(v - F.y[idx])
                if F.uright is not None and F.uright[idx] >= 0:
                    er = f32(ur - F.uright[idx])
                    e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                    st.d["chi2"][i].append((idx, f32(e2 * inv[kl])))
                    if float(f32(e2 * inv[kl])) > 7.8:
                        continue
                else:
                    e2 = f32(f32(ex * ex) + f32(ey * ey))
                    st.d["chi2"][i].append((idx, f32(e2 * inv[kl])))
                    if float(f32(e2 * inv[kl])) > 5.99:
                        continue
            dist = int(np.count_nonzero(bits[idx] != qb))
            if dist < 256:
                seen.append((dist, pos, idx))
            if dist < bd:
                bd, bi = dist, idx
        st.cands(i, seen, np.zeros(F.n, bool))
        st.d["best"][i] = (bd, bi)
        if bd <= 50:
            best[i] = bi
            st.leave(i, "accepted")
        else:
            st.leave(i, "th_reject")
    if stats is not None:
        st.d["any_occ"] = [False] * mp.n
        stats.update(st.d)
    return int((best >= 0).sum()), best


@pytest.mark.parametrize("seed,stereo,th", [(3, True, 3.0), (4, False, 3.0), (5, True, 5.0)])
def test_fuse_oracle_matches_restatement(seed, stereo, th):
    F, Tcw, Ow, mps, inv = ps.fuse_scene(seed, stereo)
    n, b = oracle_py.fuse(F, Tcw, Ow, mps, th, inv)
    R = [[f32(Tcw[r][c]) for c in range(3)] for r in range(3)]
    t = [f32(Tcw[r][3]) for r in range(3)]
    n2, b2 = fuse_py(F, mps, th, R, t, Ow, inv)
    assert n == n2 and n > mps.n // 4
    np.testing.assert_array_equal(b, b2)


def test_fuse_sim3_oracle_matches_restatement():
    F, Scw, mps = ps.fuse_sim3_scene(6)
    n, b = oracle_py.fuse_sim3(F, Scw, mps, 4.0)
    scw = f32(np.sqrt(sum(float(Scw[0][c]) * float(Scw[0][c]) for c in range(3))))
    inv = f32(1.0 / float(scw))
    R = [[f32(Scw[r][c] * inv) for c in range(3)] for r in range(3)]
    t = [f32(Scw[r][3] * inv) for r in range(3)]
    Ow = [f32(-sum(float(R[k][i]) * float(t[k]) for k in range(3))) for i in range(3)]
    n2, b2 = fuse_py(F, mps, 4.0, R, t, Ow, sim3=True)
    assert n == n2 and n > mps.n // 4
    np.testing.assert_array_equal(b, b2)


# ------------------------------------------------------------------ ComputeDistinctiveDescriptors
def distinctive_scene(seed, big=False):
    rng = np.random.default_rng(seed)
    sizes = list(rng.integers(0, 70, 300)) + [1, 2, 3, 0]
    if big:
        sizes += [1100, 1500]
    rows = []
    for n in sizes:
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        obs = np.repeat(base[None], n, 0)
        if n:
            obs = ps.flip_bits(rng, obs, 30)
            dup = rng.random(n) < 0.1  # exact duplicates -> median ties
            obs[dup] = obs[0]
        rows.append(obs)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return off, np.concatenate(rows).astype(np.uint8)


def distinctive_py(off, desc):
    out = []
    for p in range(len(off) - 1):
        d = desc[off[p]:off[p + 1]]
        n = len(d)
        if n == 0:
            out.append(-1)
            continue
        bits = np.unpackbits(d, axis=1).astype(np.int32)
        D = (bits[:, None, :] != bits[None, :, :]).sum(-1)
        med = np.sort(D, axis=1)[:, int(0.5 * (n - 1))]
        out.append(int(np.argmin(med)))  # first minimum
    return np.array(out, np.int32)


def test_distinctive_oracle_matches_restatement():
    off, desc = distinctive_scene(1)
    np.testing.assert_array_equal(oracle_py.compute_distinctive_descriptors(off, desc), distinctive_py(off, desc))


# ------------------------------------------------------------------ SearchForInitialization (ORBmatcher.cc:405-520)
def init_py(F1, F2, prev, window, nnratio, check_ori):
    """literal restatement: in-order queries, vMatchedDistance / vnMatches21 with stealing, rotation bins
    that keep stolen entries, ComputeThreeMaxima, vbPrevMatched update"""
    g = grid_py(F2)
    b2 = np.unpackbits(F2.desc, axis=1)
    m12 = np.full(F1.n, -1, np.int32)
    md = np.full(F2.n, 2 ** 31 - 1, np.int64)
    m21 = np.full(F2.n, -1, np.int64)
    hist = [[] for _ in range(30)]
    nm = 0
    for i1 in range(F1.n):
        l1 = int(F1.octave[i1])
        if l1 > 0:
            continue
        cand = area_py(F2, g, prev[i1, 0], prev[i1, 1], float(window), l1, l1)
        if not cand:
            continue
        qb = np.unpackbits(F1.desc[i1])
        best, best2, bi = 2 ** 31 - 1, 2 ** 31 - 1, -1
        for i2 in cand:
            dist = int(np.count_nonzero(b2[i2] != qb))
            if md[i2] <= dist:
                continue
            if dist < best:
                best2, best, bi = best, dist, i2
            elif dist < best2:
                best2 = dist
        if best <= 50 and f32(best) < f32(f32(best2) * f32(nnratio)):
            if m21[bi] >= 0:
                m12[m21[bi]] = -1
                nm -= 1
            m12[i1], m21[bi], md[bi] = bi, i1, best
            nm += 1
            if check_ori:
                rot = f32(F1.angle[i1] - F2.angle[bi])
                if rot < 0:
                    rot = f32(rot + f32(360))
                b = int(roundf(float(f32(rot * f32(1.0 / 30)))))
                hist[0 if b == 30 else b].append(i1)
    if check_ori:
        sizes = [len(h) for h in hist]
        i1s = [-1, -1, -1]
        m = [0, 0, 0]
        for i, sz in enumerate(sizes):
            if sz > m[0]:
                m, i1s = [sz, m[0], m[1]], [i, i1s[0], i1s[1]]
            elif sz > m[1]:
                m, i1s = [m[0], sz, m[1]], [i1s[0], i, i1s[1]]
            elif sz > m[2]:
                m[2], i1s[2] = sz, i
        if m[1] < f32(f32(0.1) * f32(m[0])):
            i1s[1] = i1s[2] = -1
        elif m[2] < f32(f32(0.1) * f32(m[0])):
            i1s[2] = -1
        for i in range(30):
            if i in i1s:
                continue
            for idx1 in hist[i]:
                if m12[idx1] >= 0:
                    m12[idx1] = -1
                    nm -= 1
    prev = prev.copy()
    for i1 in np.nonzero(m12 >= 0)[0]:
        prev[i1] = (F2.x[m12[i1]], F2.y[m12[i1]])
    return nm, m12, prev


@pytest.mark.parametrize("seed,noise,check_ori,ratio", [(1, 0.0, True, 0.9), (2, 3.0, True, 0.9), (3, 0.0, False, 0.7)])
def test_search_for_initialization_oracle_matches_restatement(seed, noise, check_ori, ratio):
    F1, F2, prev = ps.init_scene(seed, prev_noise=noise)
    n, m, p = oracle_py.search_for_initialization(F1, F2, prev, 100, ratio, check_ori)
    n2, m2, p2 = init_py(F1, F2, prev, 100, ratio, check_ori)
    assert n == n2 and n > 100
    np.testing.assert_array_equal(m, m2)
    np.testing.assert_array_equal(p, p2)


# ------------------------------------------------------------------ SearchBySim3 (ORBmatcher.cc:1102-1326)
def sim3_py(KF1, T1w, mp1, KF2, T2w, mp2, s12, R12, t12, th):
    inv_s = f32(1.0 / float(s12))
    sR12 = [[f32(R12[r][c] * s12) for c in range(3)] for r in range(3)]
    sR21 = [[f32(R12[c][r] * inv_s) for c in range(3)] for r in range(3)]
    t21 = [f32(-float(f32(f32(f32(sR21[r][0] * t12[0]) + f32(sR21[r][1] * t12[1])) + f32(sR21[r][2] * t12[2]))))
           for r in range(3)]
    fx, fy, cx, cy = KF1.fx, KF1.fy, KF1.cx, KF1.cy

    def direction(KF, T, mp, sR, t):
        g = grid_py(KF)
        bits = np.unpackbits(KF.desc, axis=1)
        R = [[f32(T[r][c]) for c in range(3)] for r in range(3)]
        tw = [f32(T[r][3]) for r in range(3)]
        out = np.full(mp.n, -1, np.int32)
        for i in range(mp.n):
            if mp.skip[i] or mp.bad[i]:
                continue
            pc = _gemm33_fast(sR, _gemm33_fast(R, [f32(v) for v in mp.pos[i]], tw), t)
            if pc[2] < 0:
                continue
            invz = f32(1.0 / float(pc[2]))
            u = f32(f32(fx * f32(pc[0] * invz)) + cx)
            v = f32(f32(fy * f32(pc[1] * invz)) + cy)
            if not (u >= KF.min_x and u < KF.max_x and v >= KF.min_y and v < KF.max_y):
                continue
            d3 = _norm3(pc)
            if d3 < f32(f32(0.8) * mp.min_dist[i]) or d3 > f32(f32(1.2) * mp.max_dist[i]):
                continue
            lvl = _predict_scale(mp.max_dist[i], d3, KF)
            rad = f32(f32(th) * KF.scale_factors[lvl])
            qb = np.unpackbits(mp.desc[i])
            bd, bi = 2 ** 31 - 1, -1
            for idx in area_py(KF, g, u, v, rad):
                if KF.octave[idx] < lvl - 1 or KF.octave[idx] > lvl:
                    continue
                dist = int(np.count_nonzero(bits[idx] != qb))
                if dist < bd:
                    bd, bi = dist, idx
            if bd <= 100:
                out[i] = bi
        return out

    v1 = direction(KF2, T1w, mp1, sR21, t21)
    v2 = direction(KF1, T2w, mp2, sR12, [f32(x) for x in t12])
    m12 = np.full(mp1.n, -1, np.int32)
    for i1 in range(mp1.n):
        if v1[i1] >= 0 and v2[v1[i1]] == i1:
            m12[i1] = v1[i1]
    return int((m12 >= 0).sum()), m12


@pytest.mark.parametrize("seed", [2, 5])
def test_search_by_sim3_oracle_matches_restatement(seed):
    sc = ps.sim3_pair_scene(seed)
    n, m = oracle_py.search_by_sim3(*sc)
    n2, m2 = sim3_py(*sc)
    assert n == n2 and n > 100
    np.testing.assert_array_equal(m, m2)

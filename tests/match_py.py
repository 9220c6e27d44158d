"""numpy / pure-Python restatements of the three FeatureVector matchers, written from the reference text
(ORB_SLAM2/src/ORBmatcher.cc), not from the C oracle:

  search_for_triangulation_py   ORBmatcher.cc:657-823, CheckDistEpipolarLine :140-157
  search_by_bow_kf_f_py         ORBmatcher.cc:159-288
  search_by_bow_kf_kf_py        ORBmatcher.cc:522-655

and the rotation-consistency pieces every matcher shares (ComputeThreeMaxima :1601-1642, the histogram push and
the filter). The views are orbamd.matcher.KeyFrameView (mvKeysUn, mDescriptors, mvuRight, GetMapPoint / isBad,
mFeatVec, mvScaleFactors, mvLevelSigma2).

Arithmetic: every float operation is one np.float32 step in the reference's order (no fused multiply-add); the
epipolar comparison is made in double against 3.84 * float64(sigma2) (`dsqr<3.84*...`: a double literal times a
float); `100*mvScaleFactors[octave]` is a float product; `(float)best1 < mfNNratio*(float)best2` is a float
comparison.

Each function also returns, through `stats`, the exit every query took (MatchStats), so that a hand-made case
can be shown to sit where it was built to sit without asking the code under test.
"""
import bisect

import numpy as np

f32 = np.float32
TH_LOW = 50  # ORBmatcher.cc:38
HISTO_LENGTH = 30  # ORBmatcher.cc:39


def roundf(v):
    """C roundf (half away from zero) for v >= 0; v - floor(v) is exact for floats."""
    fl = np.floor(v)
    return f32(fl + (1 if v - fl >= 0.5 else 0))


# ------------------------------------------------------------------ rotation consistency
def _three_maxima_py(sizes):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1601-1642): the kept bins"""
    ind, m = [-1, -1, -1], [0, 0, 0]
    for i, s in enumerate(sizes):
        if s > m[0]:
            m, ind = [s, m[0], m[1]], [i, ind[0], ind[1]]
        elif s > m[1]:
            m, ind = [m[0], s, m[1]], [ind[0], i, ind[1]]
        elif s > m[2]:
            m[2], ind[2] = s, i
    if f32(m[1]) < f32(f32(0.1) * f32(m[0])):
        ind[1] = ind[2] = -1
    elif f32(m[2]) < f32(f32(0.1) * f32(m[0])):
        ind[2] = -1
    return ind


def _rot_push(hist, st, i, a1, a2, idx):
    """ORBmatcher.cc:1431-1441 / 1560-1570 (the matchers: :236-246, :604-614, :764-774)"""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    p = f32(rot * f32(f32(1.0) / f32(30)))
    b = int(roundf(p))
    if b == 30:
        b = 0
    assert 0 <= b < 30
    hist[b].append(idx)
    st.d["rot"][i] = (b, p)


def _rot_filter_py(hist, st, match, nm, null=-2):
    """ORBmatcher.cc:1447-1467 / 1577-1596 (-2 stands for the NULL the reference writes); the FeatureVector
    matchers write -1 into vMatches12 (:799-808) or NULL into a vector the caller reads as "no match"
    (:275-284, :635-651): null = -1"""
    keep = _three_maxima_py([len(h) for h in hist])
    st.d["hist"], st.d["kept_bins"] = [len(h) for h in hist], keep
    for b in range(30):
        if b not in keep:
            for idx in hist[b]:
                match[idx] = null
                nm -= 1
    return nm


# ------------------------------------------------------------------ DescriptorDistance
def descriptor_distance_py(a, b):
    """ORBmatcher::DescriptorDistance (ORBmatcher.cc:1647-1663) for arrays of descriptors [..., 32] (broadcast):
    the eight 32-bit words, each counted with the bit trick of the reference in unsigned 32-bit arithmetic"""
    pa = np.ascontiguousarray(a, np.uint8).view("<u4")
    pb = np.ascontiguousarray(b, np.uint8).view("<u4")
    v = pa ^ pb
    v = v - ((v >> np.uint32(1)) & np.uint32(0x55555555))
    v = (v & np.uint32(0x33333333)) + ((v >> np.uint32(2)) & np.uint32(0x33333333))
    w = ((v + (v >> np.uint32(4))) & np.uint32(0xF0F0F0F)).astype(np.uint64) * np.uint64(0x1010101)
    return ((w & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.int64).sum(axis=-1)


def _dist_block(d1, idx1, d2, idx2):
    """distances of the descriptors idx1 of d1 (rows) to idx2 of d2 (columns)"""
    if len(idx1) == 0 or len(idx2) == 0:
        return np.zeros((len(idx1), len(idx2)), np.int64)
    return descriptor_distance_py(d1[np.asarray(idx1)][:, None, :], d2[np.asarray(idx2)][None, :, :])


# ------------------------------------------------------------------ stats
class MatchStats:
    """per query (a feature index of KF1 / of the KeyFrame): d["exit"][i] and what decided it.

    SearchForTriangulation exits: "no_common_node" (its node is not in the other FeatureVector, or it is in no
    node), "has_mp", "mono_only_stereo", "no_low_dist" (no eligible candidate reached the geometric tests),
    "all_near_epipole", "all_epi_fail" (d["decisive"][i] = (idx2, dsqr or None when den == 0, threshold) of the
    rejected candidate of least distance, the later on ties), "accepted", "rot_removed".
      d["tested"][i] = [(idx2, node position, dist, "near" | "den0" | "epi_fail" | "ok", dsqr, th)] in scan order
      d["best"][i] = (dist, idx2); d["ties"][i] = node positions of the candidates that passed at the winning
      distance; d["better_rejected"][i] = how many candidates of smaller distance the geometry rejected
    SearchByBoW exits: "no_common_node", "no_good_mp", "no_candidate", "over_th_low", "ratio_fail"
    (d["ratio"][i] = the two floats compared), "accepted", "rot_removed".
      d["best"][i] = (best1, idx, best2); d["skipped"][i] = candidates passed over as already matched;
      d["ineligible"][i] = candidates without a good MapPoint (KF,KF)
    d["rot"][i] = (bin, rot * factor before rounding); d["hist"], d["kept_bins"] after the filter."""

    def __init__(self, n):
        self.d = {k: [None] * n for k in ("rot", "best", "decisive", "ratio")}
        self.d["exit"] = ["no_common_node"] * n
        for k in ("tested", "ties", "skipped", "ineligible"):
            self.d[k] = [[] for _ in range(n)]
        self.d["better_rejected"] = [0] * n
        self.d["hist"] = None
        self.d["kept_bins"] = None

    def exit(self, i, name):
        self.d["exit"][i] = name

    def finish(self):
        keep = self.d["kept_bins"]
        if keep is None:
            return
        for i, e in enumerate(self.d["exit"]):
            if e == "accepted" and self.d["rot"][i][0] not in keep:
                self.d["exit"][i] = "rot_removed"


def _feat_vec(v):
    """mFeatVec as the reference holds it: ascending node ids and each node's feature indices in stored order"""
    ids = [int(i) for i in v.node_id]
    off = v.node_off
    return ids, [[int(f) for f in v.node_feat[off[k]:off[k + 1]]] for k in range(len(ids))]


def _merge_walk(ids1, ids2):
    """the walk over two FeatureVectors (ORBmatcher.cc:180-264, 545-631, 691-789): positions (k1, k2) of the
    nodes visited as equal; an unequal pair advances the smaller side with lower_bound of the other's id"""
    k1 = k2 = 0
    while k1 < len(ids1) and k2 < len(ids2):
        if ids1[k1] == ids2[k2]:
            yield k1, k2
            k1 += 1
            k2 += 1
        elif ids1[k1] < ids2[k2]:
            k1 = bisect.bisect_left(ids1, ids2[k2])
        else:
            k2 = bisect.bisect_left(ids2, ids1[k1])


def _flag(a, i):
    return a is not None and bool(a[i])


def _uright(v, i):
    """mvuRight[i]; a monocular KeyFrame holds -1 everywhere (Frame.cc:222-223)"""
    return f32(-1) if v.uright is None else f32(v.uright[i])


# ------------------------------------------------------------------ CheckDistEpipolarLine
def epipolar_line_py(x1, y1, F12):
    """(a, b, c) of ORBmatcher.cc:143-145; F12 row-major 3x3"""
    F = np.asarray(F12, f32).reshape(3, 3)
    x1, y1 = f32(x1), f32(y1)
    a = f32(f32(f32(x1 * F[0, 0]) + f32(y1 * F[1, 0])) + F[2, 0])
    b = f32(f32(f32(x1 * F[0, 1]) + f32(y1 * F[1, 1])) + F[2, 1])
    c = f32(f32(f32(x1 * F[0, 2]) + f32(y1 * F[1, 2])) + F[2, 2])
    return a, b, c


def check_dist_epipolar_py(x1, y1, x2, y2, F12, sigma2):
    """ORBmatcher::CheckDistEpipolarLine (:140-157): (accepted, dsqr or None when den == 0, threshold)"""
    with np.errstate(over="ignore", invalid="ignore"):
        a, b, c = epipolar_line_py(x1, y1, F12)
        x2, y2 = f32(x2), f32(y2)
        num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
        den = f32(f32(a * a) + f32(b * b))
        th = 3.84 * float(f32(sigma2))  # double
        if den == 0:
            return False, None, th
        dsqr = f32(f32(num * num) / den)
        return bool(float(dsqr) < th), dsqr, th


def near_epipole_py(ex, ey, x2, y2, scale):
    """ORBmatcher.cc:745-748: distex*distex+distey*distey < 100*mvScaleFactors[octave], all float"""
    distex = f32(f32(ex) - f32(x2))
    distey = f32(f32(ey) - f32(y2))
    return bool(f32(f32(distex * distex) + f32(distey * distey)) < f32(f32(100) * f32(scale)))


# ------------------------------------------------------------------ SearchForTriangulation
def search_for_triangulation_py(kf1, kf2, F12, ex, ey, only_stereo=False, check_ori=False, stats=None):
    """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:657-823): (nmatches, vMatches12). vbMatched2 is
    created all false (:677) and never set, so `vbMatched2[idx2] ||` (:725) never skips anything and one
    candidate can be the match of several queries; it is left out here for that reason."""
    st = stats if stats is not None else MatchStats(kf1.n)
    nmatches = 0
    match = np.full(kf1.n, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    ids1, fv1 = _feat_vec(kf1)
    ids2, fv2 = _feat_vec(kf2)
    for k1, k2 in _merge_walk(ids1, ids2):
        D = _dist_block(kf1.desc, fv1[k1], kf2.desc, fv2[k2])
        for i1, idx1 in enumerate(fv1[k1]):
            if _flag(kf1.has_mp, idx1):  # pMP1 (:699-703)
                st.exit(idx1, "has_mp")
                continue
            stereo1 = bool(_uright(kf1, idx1) >= 0)
            if only_stereo and not stereo1:
                st.exit(idx1, "mono_only_stereo")
                continue
            best_dist, best_idx2 = TH_LOW, -1
            tested = st.d["tested"][idx1]
            for i2, idx2 in enumerate(fv2[k2]):
                if _flag(kf2.has_mp, idx2):
                    continue
                stereo2 = bool(_uright(kf2, idx2) >= 0)
                if only_stereo and not stereo2:
                    continue
                dist = int(D[i1, i2])
                if dist > TH_LOW or dist > best_dist:
                    continue
                oct2 = int(kf2.octave[idx2])
                if not stereo1 and not stereo2:
                    if near_epipole_py(ex, ey, kf2.x[idx2], kf2.y[idx2], kf2.scale_factors[oct2]):
                        tested.append((idx2, i2, dist, "near", None, None))
                        continue
                ok, dsqr, th = check_dist_epipolar_py(kf1.x[idx1], kf1.y[idx1], kf2.x[idx2], kf2.y[idx2], F12,
                                                      kf2.level_sigma2[oct2])
                tested.append((idx2, i2, dist, "ok" if ok else ("den0" if dsqr is None else "epi_fail"), dsqr, th))
                if ok:
                    best_idx2, best_dist = idx2, dist
            if best_idx2 >= 0:
                match[idx1] = best_idx2
                nmatches += 1
                st.exit(idx1, "accepted")
                st.d["best"][idx1] = (best_dist, best_idx2)
                st.d["ties"][idx1] = [t[1] for t in tested if t[2] == best_dist and t[3] == "ok"]
                st.d["better_rejected"][idx1] = sum(1 for t in tested if t[2] < best_dist)
                if check_ori:
                    _rot_push(hist, st, idx1, kf1.angle[idx1], kf2.angle[best_idx2], idx1)
            elif not tested:
                st.exit(idx1, "no_low_dist")
            elif all(t[3] == "near" for t in tested):
                st.exit(idx1, "all_near_epipole")
            else:
                st.exit(idx1, "all_epi_fail")
                fails = [t for t in tested if t[3] != "near"]
                t = min(reversed(fails), key=lambda t: t[2])  # least distance, the later on ties
                st.d["decisive"][idx1] = (t[0], t[4], t[5])
    if check_ori:
        nmatches = _rot_filter_py(hist, st, match, nmatches, null=-1)
    st.finish()
    return nmatches, match


# ------------------------------------------------------------------ SearchByBoW x2
def _search_by_bow_py(kf, other, nnratio, check_ori, kfkf, st):
    n_out = kf.n if kfkf else other.n
    match = np.full(n_out, -1, np.int32)  # (KF,F): vpMapPointMatches by F index; (KF,KF): vpMatches12 by idx1
    matched2 = np.zeros(other.n, bool)    # (KF,KF): vbMatched2 (:535); (KF,F): vpMapPointMatches[realIdxF] != NULL
    nmatches = 0
    hist = [[] for _ in range(HISTO_LENGTH)]
    ids1, fv1 = _feat_vec(kf)
    ids2, fv2 = _feat_vec(other)
    ratio = f32(nnratio)
    for k1, k2 in _merge_walk(ids1, ids2):
        D = _dist_block(kf.desc, fv1[k1], other.desc, fv2[k2])
        for i1, idx1 in enumerate(fv1[k1]):
            if not _flag(kf.has_mp, idx1) or _flag(kf.mp_bad, idx1):  # !pMP / pMP->isBad() (:193-197, :558-562)
                st.exit(idx1, "no_good_mp")
                continue
            best1, best_idx, best2 = 256, -1, 256
            for i2, idx2 in enumerate(fv2[k2]):
                if matched2[idx2]:
                    st.d["skipped"][idx1].append(idx2)
                    continue
                if kfkf and (not _flag(other.has_mp, idx2) or _flag(other.mp_bad, idx2)):  # :574-580
                    st.d["ineligible"][idx1].append(idx2)
                    continue
                dist = int(D[i1, i2])
                if dist < best1:
                    best2, best1, best_idx = best1, dist, idx2
                elif dist < best2:
                    best2 = dist
            st.d["best"][idx1] = (best1, best_idx, best2)
            if best_idx < 0:
                st.exit(idx1, "no_candidate")  # best1 stays 256: over TH_LOW in the reference's own terms
                continue
            if not (best1 < TH_LOW if kfkf else best1 <= TH_LOW):  # :598 `<`, :228 `<=`
                st.exit(idx1, "over_th_low")
                continue
            lhs, rhs = f32(best1), f32(ratio * f32(best2))
            st.d["ratio"][idx1] = (lhs, rhs)
            if not lhs < rhs:
                st.exit(idx1, "ratio_fail")
                continue
            st.exit(idx1, "accepted")
            matched2[best_idx] = True
            nmatches += 1
            if kfkf:
                match[idx1] = best_idx
                if check_ori:  # rot = vKeysUn1[idx1].angle - vKeysUn2[bestIdx2].angle, rotHist[bin].push_back(idx1)
                    _rot_push(hist, st, idx1, kf.angle[idx1], other.angle[best_idx], idx1)
            else:
                match[best_idx] = idx1
                if check_ori:  # rot = kp.angle - F.mvKeys[bestIdxF].angle, rotHist[bin].push_back(bestIdxF)
                    _rot_push(hist, st, idx1, kf.angle[idx1], other.angle[best_idx], best_idx)
    if check_ori:
        nmatches = _rot_filter_py(hist, st, match, nmatches, null=-1)
    st.finish()
    return nmatches, match


def search_by_bow_kf_f_py(kf, f, nnratio, check_ori, stats=None):
    """ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cc:159-288): (nmatches, by F index the KF
    feature whose MapPoint it received, -1 = NULL)"""
    return _search_by_bow_py(kf, f, nnratio, check_ori, False, stats if stats is not None else MatchStats(kf.n))


def search_by_bow_kf_kf_py(kf1, kf2, nnratio, check_ori, stats=None):
    """ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (ORBmatcher.cc:522-655): (nmatches, by idx1 the idx2
    whose MapPoint it received, -1 = NULL)"""
    return _search_by_bow_py(kf1, kf2, nnratio, check_ori, True, stats if stats is not None else MatchStats(kf1.n))

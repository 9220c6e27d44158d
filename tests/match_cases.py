"""Hand-made keyframe pairs for SearchForTriangulation (ORBmatcher.cc:657-823) and the two SearchByBoW overloads
(:159-288, :522-655): one query per edge of the algorithm.

A keyframe is arrays of x, y, octave, angle, descriptor, uRight, MapPoint flags and a FeatureVector: no image, no
extractor. A descriptor at Hamming distance h from another is that one with exactly h bits flipped. A Case holds
one pair (KF1 / KeyFrame = the query side, KF2 / Frame = the candidate side), the geometry and scale tables the
entry points take as inputs, the calls it is meant for, and `expect`: the exit of the reference each named query
is built to take in each call. Whether it takes that exit is asserted on the CPU from the restatements' stats
(match_py.py, test_oracle_match.py), never from the code under test.

The default geometry makes every pair of equal y pass: F12 = F_ROW gives the line a = 0, b = 1, c = -y1, so
dsqr = fl(fl(y2 - y1)^2), and the epipole lies far outside the image. Cases that test the geometry replace it.

Everything is inside the reference's domain: finite values, octaves < nlevels, n < 65536, every feature in
exactly one FeatureVector node.
"""
import numpy as np

import match_py as mp
from orbamd.matcher import KeyFrameView

f32 = np.float32
F_ROW = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
FAR = (f32(-4000.0), f32(-4000.0))  # an epipole no keypoint is near
KP = [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")]


def up(v):
    return np.nextafter(f32(v), f32(np.inf), dtype=f32)


def down(v):
    return np.nextafter(f32(v), f32(-np.inf), dtype=f32)


def scale_table(nlevels=8, factor=1.2):
    s = [f32(1)]
    for _ in range(1, nlevels):
        s.append(f32(s[-1] * f32(factor)))
    return np.array(s, f32)


def default_f12():
    import orbamd
    return orbamd.device.default_geometry()


class KF:
    def __init__(self):
        self.x, self.y, self.o, self.a, self.d, self.ur, self.mp, self.bad, self.node = ([] for _ in range(9))

    @property
    def n(self):
        return len(self.x)

    def add(self, x, y, d, octave=0, angle=0.0, ur=-1.0, mp=0, bad=0, node=0):
        for lst, v in zip((self.x, self.y, self.o, self.a, self.d, self.ur, self.mp, self.bad, self.node),
                          (f32(x), f32(y), int(octave), f32(angle), np.asarray(d, np.uint8), f32(ur), int(mp),
                           int(bad), int(node))):
            lst.append(v)
        return self.n - 1

    def keypoints(self):
        k = np.zeros(self.n, KP)
        k["x"], k["y"], k["octave"], k["angle"] = self.x, self.y, self.o, self.a
        return k

    def descriptors(self):
        return np.array(self.d, np.uint8).reshape(self.n, 32)

    def feat_vec(self):
        fv = {}
        for i, nd in enumerate(self.node):
            fv.setdefault(nd, []).append(i)
        return fv

    def view(self, scale, sigma2):
        return KeyFrameView(self.keypoints(), self.descriptors(), scale, sigma2, feat_vec=self.feat_vec(),
                            uright=np.array(self.ur, f32), has_mp=np.array(self.mp, np.uint8),
                            mp_bad=np.array(self.bad, np.uint8))


class Case:
    """expect / best: by KF1 feature index; a value is a string / index (every call) or a dict by call key"""

    def __init__(self, name, seed, F12=F_ROW, epipole=FAR, scale=None, sigma2=None):
        self.name = name
        self.rng = np.random.default_rng([657823, seed])
        self.F12 = np.ascontiguousarray(F12, f32).reshape(3, 3)
        self.ex, self.ey = float(epipole[0]), float(epipole[1])
        self.scale = scale_table() if scale is None else np.asarray(scale, f32)
        self.sigma2 = (self.scale * self.scale).astype(f32) if sigma2 is None else np.asarray(sigma2, f32)
        assert len(self.scale) == len(self.sigma2) and 1 <= len(self.scale) <= 16
        self.k1, self.k2 = KF(), KF()
        self.calls, self.expect, self.best, self.names, self.notes = [], {}, {}, {}, {}
        self._views = None
        self.rots, self.stereo_form = None, False

    # ---- primitives
    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def flip(self, d, h):
        d = np.array(d, np.uint8)
        for p in self.rng.permutation(256)[:h]:
            d[p >> 3] ^= np.uint8(1 << (p & 7))
        return d

    def q(self, name, d, expect, best=None, x=None, y=100.0, **kw):
        i = self.k1.add(40.0 + self.k1.n if x is None else x, y, d, **kw)
        self.names[name] = i
        self.expect[i], self.best[i] = expect, best
        return i

    def c(self, d, x=None, y=100.0, **kw):
        return self.k2.add(40.0 + self.k2.n if x is None else x, y, d, **kw)

    def probe(self, name, hs, expect="accepted", best=None, qkw=None, ckw=None, node=0):
        """a query with a descriptor of its own and one candidate per entry of hs at that Hamming distance;
        best = position in hs of the candidate an accepted query takes; ckw[k]: overrides of candidate k"""
        d = self.desc()
        ids = [self.c(self.flip(d, h), node=node, **((ckw or {}).get(k, {}))) for k, h in enumerate(hs)]

        def tr(b):
            return None if b is None else ids[b]
        best = {k: tr(b) for k, b in best.items()} if isinstance(best, dict) else tr(best)
        return self.q(name, d, expect, best, node=node, **(qkw or {})), ids

    def tri(self, key="tri", only_stereo=False, check_ori=False):
        self.calls.append(dict(key=key, kind="tri", only_stereo=only_stereo, check_ori=check_ori, nnratio=0.6))

    def bow(self, key, mode, nnratio=0.75, check_ori=False):
        self.calls.append(dict(key=key, kind="bow%d" % mode, only_stereo=False, check_ori=check_ori,
                               nnratio=nnratio))

    def both_bow(self, nnratio=0.75, check_ori=False):
        self.bow("bow0", 0, nnratio, check_ori)
        self.bow("bow1", 1, nnratio, check_ori)

    # ---- what the entry points take
    def views(self):
        if self._views is None:
            for k in (self.k1, self.k2):
                assert k.n < 65536 and all(0 <= o < len(self.scale) for o in k.o)
                assert np.isfinite(np.array(k.x + k.y + k.a + k.ur, f32)).all()
            self._views = (self.k1.view(self.scale, self.sigma2), self.k2.view(self.scale, self.sigma2))
        return self._views

    def expected(self, call, i):
        e, b = self.expect[i], self.best[i]
        e = e.get(call["key"], e.get("*")) if isinstance(e, dict) else e
        b = b.get(call["key"], b.get("*")) if isinstance(b, dict) else b
        return e, b

    # ---- which batch entry points can express the pair
    @property
    def one_node(self):
        return len(set(self.k1.node)) <= 1 and set(self.k1.node) == set(self.k2.node) or not (self.k1.n and self.k2.n)

    @property
    def no_mp(self):
        return not any(self.k1.mp) and not any(self.k2.mp)

    @property
    def mono(self):
        return not (np.array(self.k1.ur + self.k2.ur + [-1.0], f32) >= 0).any()


# ===================================================================== a. epipolar distance
def sigma_just_above(dsq):
    """the level_sigma2 entry s (a float) with 3.84 * float64(s) just above dsq: the smallest such float"""
    s = f32(dsq / 3.84)
    while 3.84 * float(s) <= dsq:
        s = up(s)
    while 3.84 * float(down(s)) > dsq:
        s = down(s)
    return s


def flip_float(decide, lo, hi):
    """adjacent floats (a, b), lo <= a < b <= hi, with decide(a) != decide(b); decide(lo) != decide(hi)"""
    lo, hi = f32(lo), f32(hi)
    assert decide(lo) != decide(hi)
    while up(lo) < hi:
        mid = f32((float(lo) + float(hi)) / 2)
        if mid <= lo or mid >= hi:
            mid = up(lo)
        if decide(mid) == decide(lo):
            lo = mid
        else:
            hi = mid
    return lo, hi


def group_a():
    cases = []
    # exact threshold. |y2 - y1| = 2: dsqr = 4 and 3.84 * s in (4, nextafter(4)]; |y2 - y1| = 7: dsqr = 49 and
    # 3.84 * s = 49.0000012 lies below the midpoint of 49 and the next float, so a threshold rounded to the
    # nearest float instead of up becomes 49 and rejects what the reference accepts (at 2 the product lies above
    # the midpoint, where both roundings agree)
    for nlevels, octs in ((8, (0, 3, 7)), (1, (0,)), (16, (15,))):
        for dy in (2.0, 7.0):
            s = sigma_just_above(dy * dy)
            for which, sv, exp in (("at", s, "accepted"), ("below", down(s), "all_epi_fail")):
                sc = scale_table(nlevels)
                sg = (sc * sc).astype(f32)
                for o in octs:
                    sg[o] = sv
                c = Case("a_exact_L%d_dy%d_%s" % (nlevels, dy, which), 1, scale=sc, sigma2=sg)
                for o in octs:
                    c.probe("oct%d" % o, [5], exp, 0 if exp == "accepted" else None,
                            ckw={0: dict(octave=o, y=100.0 + dy)})
                    c.probe("oct%d_neg" % o, [5], exp, 0 if exp == "accepted" else None,
                            ckw={0: dict(octave=o, y=100.0 - dy)})
                c.notes = dict(dsq=dy * dy, sigma=sv, octs=octs)
                c.tri()
                cases.append(c)
    # a general F12: the two adjacent y2 between which the restatement's decision flips, one candidate on each
    F12, ex, ey = default_f12()
    for nlevels, octs in ((8, (0, 3, 7)), (1, (0,)), (16, (15,))):
        sc = scale_table(nlevels)
        c = Case("a_general_L%d" % nlevels, 2, F12=F12, epipole=FAR, scale=sc)
        for o in octs:
            x1, y1, x2 = 200.0 + 10 * o, 150.0, 260.0
            def decide(y2, o=o, x1=x1, y1=y1, x2=x2):
                return mp.check_dist_epipolar_py(x1, y1, x2, y2, F12, c.sigma2[o])[0]
            # on the line at some y2 near y1 (the pose is a sideways step); walk out until it is rejected
            on = min(np.arange(100.0, 200.0, 0.25), key=lambda y2: float(
                mp.check_dist_epipolar_py(x1, y1, x2, y2, F12, c.sigma2[o])[1]))
            assert decide(on) and not decide(on + 60.0)
            ya, yb = flip_float(decide, on, on + 60.0)
            c.probe("oct%d_in" % o, [5], "accepted", 0, qkw=dict(x=x1, y=y1), ckw={0: dict(octave=o, x=x2, y=ya)})
            c.probe("oct%d_out" % o, [5], "all_epi_fail", None, qkw=dict(x=x1, y=y1),
                    ckw={0: dict(octave=o, x=x2, y=yb)})
        c.tri()
        cases.append(c)
    return cases


# ===================================================================== b. den == 0
def group_b():
    c0 = Case("b_F_zero", 3, F12=np.zeros((3, 3), f32))
    for k in range(5):
        c0.probe("q%d" % k, [0, 7], "all_epi_fail")
    c0.tri()
    # a = x1 - 300, b = y1 - 100, c = -100: the query at (300, 100) has den == 0 exactly, its neighbours do not
    F = np.array([[1, 0, 0], [0, 1, 0], [-300, -100, -100]], f32)
    c1 = Case("b_one_position", 4, F12=F)
    c1.probe("den0", [3], "all_epi_fail", qkw=dict(x=300.0, y=100.0), ckw={0: dict(x=100.0, y=50.0)})
    c1.probe("a1", [3], "accepted", 0, qkw=dict(x=301.0, y=100.0), ckw={0: dict(x=100.0, y=50.0)})   # num = x2 - 100
    c1.probe("b1", [3], "accepted", 0, qkw=dict(x=300.0, y=101.0), ckw={0: dict(x=50.0, y=100.0)})   # num = y2 - 100
    c1.probe("bneg", [3], "accepted", 0, qkw=dict(x=300.0, y=99.0), ckw={0: dict(x=50.0, y=-100.0)})  # num = -y2 - 100
    c1.tri()
    return [c0, c1]


# ===================================================================== c. epipole radius
def group_c():
    cases = []
    # scale 1.0, epipole (106, 8): offsets (6, 8) give 36 + 64 = 100, `100 < 100` is false: not near; (6, down(8))
    # is near. Each query's near / not near candidate has D = 5, a far candidate at D = 20 stands behind it
    c = Case("c_exact", 5, epipole=(106.0, 8.0))
    tiny = f32(2.0 ** -21)  # 8 - 2^-21 = down(8) exactly
    assert f32(f32(8.0) - tiny) == down(8.0)
    c.probe("on_radius", [5, 20], "accepted", 0, qkw=dict(y=0.0), ckw={0: dict(x=100.0, y=0.0), 1: dict(x=400.0, y=0.0)})
    c.probe("inside", [5, 20], "accepted", 1, qkw=dict(y=tiny), ckw={0: dict(x=100.0, y=tiny), 1: dict(x=400.0, y=tiny)})
    c.probe("inside_only", [5], "all_near_epipole", qkw=dict(y=tiny), ckw={0: dict(x=100.0, y=tiny)})
    c.tri()
    cases.append(c)
    # an octave whose 100 * scale is no integer (1.2f): the adjacent floats of x2 around the restatement's flip
    c = Case("c_scale12", 6, epipole=(300.0, 200.0))
    s1 = c.scale[1]
    xa, xb = flip_float(lambda x2: mp.near_epipole_py(300.0, 200.0, x2, 200.0, s1), 300.0, 330.0)
    c.probe("in", [5, 20], "accepted", 1, qkw=dict(y=200.0), ckw={0: dict(x=xa, y=200.0, octave=1),
                                                                 1: dict(x=500.0, y=200.0, octave=1)})
    c.probe("out", [5, 20], "accepted", 0, qkw=dict(y=200.0), ckw={0: dict(x=xb, y=200.0, octave=1),
                                                                  1: dict(x=500.0, y=200.0, octave=1)})
    c.notes = dict(xa=xa, xb=xb)
    c.tri()
    cases.append(c)
    # stereo combinations next to the epipole: the D = 5 candidate sits on the epipole, a stereo D = 20 one far away
    c = Case("c_stereo", 7, epipole=(300.0, 200.0))
    for qn, ur1 in (("m", -1.0), ("z", 0.0), ("nz", -0.0), ("p", 250.0)):
        for cn, ur2 in (("m", -1.0), ("z", 0.0), ("nz", -0.0), ("p", 280.0)):
            st1, st2 = qn != "m", cn != "m"
            exp = {"tri": "accepted", "only": "accepted" if st1 else "mono_only_stereo"}
            best = {"tri": 1 if not st1 and not st2 else 0, "only": (0 if st2 else 1) if st1 else None}
            c.probe("q%s_c%s" % (qn, cn), [5, 20], exp, best, qkw=dict(y=200.0, ur=ur1),
                    ckw={0: dict(x=300.0, y=200.0, ur=ur2), 1: dict(x=600.0, y=200.0, ur=500.0)})
    c.tri("tri", only_stereo=False)
    c.tri("only", only_stereo=True)
    cases.append(c)
    return cases


# ===================================================================== d. Hamming distance and ties
def group_d():
    c = Case("d_hamming", 8)
    c.probe("d49", [49], "accepted", 0)
    c.probe("d50", [50], "accepted", 0)
    c.probe("d51", [51], "no_low_dist")
    c.probe("d0", [0], "accepted", 0)
    c.probe("d256", [256], "no_low_dist")
    c.probe("d128", [128], "no_low_dist")
    c.probe("d129", [129], "no_low_dist")
    c.probe("d0_after_256", [256, 129, 128, 0], "accepted", 3)
    c.probe("tie2", [9, 9], "accepted", 1)
    c.probe("tie3", [9, 30, 9, 9], "accepted", 3)
    c.probe("tie16", [12] * 16, "accepted", 15)
    c.probe("tie_at_50", [50, 50], "accepted", 1)
    off = dict(y=300.0)  # off the epipolar line
    c.probe("bad_before", [4, 9], "accepted", 1, ckw={0: off})
    c.probe("bad_after", [9, 4], "accepted", 0, ckw={1: off})
    c.probe("bad_tie_later", [9, 9], "accepted", 0, ckw={1: off})
    c.probe("all_bad", [4, 9], "all_epi_fail", ckw={0: off, 1: off})
    c.probe("best_first", [6, 20, 30, 40], "accepted", 0)
    c.probe("best_last", [40, 30, 20, 6], "accepted", 3)
    c.tri()
    return [c]


# ===================================================================== e. k_tri_mfma structure
E_N2 = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
E_N1 = (0, 1, 31, 32, 33, 255, 256, 257)
E_WIN = (0, 3, 4, 31, 32, 63, 64)
E_STRADDLE = ((3, 4), (31, 32), (63, 64), (127, 128))


def _e_frame(name, seed, n1, n2, stereo):
    """n2 candidates of random descriptors, n1 queries: query i wins candidate E_WIN[i mod] (or n2 - 1), and the
    tie pairs that fit get one query each whose two candidates straddle the boundary (the later one wins)"""
    c = Case(name, seed)
    c.stereo_form = stereo
    cd = [c.desc() for _ in range(n2)]
    wins = [w for w in E_WIN if w < n2 - 1] + ([n2 - 1] if n2 else [])
    ties = [(a, b) for a, b in E_STRADDLE if b < n2]
    qs = []
    for i in range(n1):
        if n2 == 0:
            qs.append((c.desc(), "no_common_node", None))  # an empty keyframe has an empty FeatureVector
        elif i < len(ties):
            a, b = ties[i]
            d = c.desc()
            cd[a], cd[b] = c.flip(d, 8), c.flip(d, 8)
            qs.append((d, "accepted", b))
        else:
            w = wins[i % len(wins)]
            qs.append((c.flip(cd[w], 2 + i % 7), "accepted", w))
    for j in range(n2):
        c.c(cd[j], x=30.0 + j, ur=(j % 3 == 0) * 20.0 - 1.0 if stereo else -1.0)
    for i, (d, exp, best) in enumerate(qs):
        c.q("q%d" % i, d, exp, best, x=30.0 + i, ur=(i % 2) * 25.0 - 1.0 if stereo else -1.0)
    c.tri()
    c.notes = dict(ties=ties[:n1], wins=wins)
    return c


# rows of tile 0 that lane half 0 of a query's lane owns (4 per register group: rows r .. r + 3 of 0, 8, 16, 24)
E_LANE_ROWS = [r + k for r in (0, 8, 16, 24) for k in range(4)]


def _e_walk(name, seed, k, winner, n2, stereo):
    """the key walk: the k best candidates of one query lie in rows one lane owns and fail the geometry (off the
    epipolar line); the winner (D = 20) lies at row `winner`"""
    c = Case(name, seed)
    c.stereo_form = stereo
    d = c.desc()
    cd = [c.desc() for _ in range(n2)]
    ys = [100.0] * n2
    for m, r in enumerate(E_LANE_ROWS[:k]):
        cd[r], ys[r] = c.flip(d, 1 + m // 2), 300.0   # pairs of equal distance: the walk steps through ties too
    cd[winner] = c.flip(d, 20)
    for j in range(n2):
        c.c(cd[j], x=30.0 + j, y=ys[j], ur=15.0 if stereo else -1.0)
    c.q("walk", d, "accepted", winner, ur=15.0 if stereo else -1.0)
    for i in range(3):  # neighbours in the same wave that match at once
        c.q("n%d" % i, c.flip(cd[winner], 3), "accepted", winner, ur=15.0 if stereo else -1.0)
    c.tri()
    c.notes = dict(k=k, winner=winner)
    return c


def _e_padding(name, seed, zero_cand, stereo):
    """an all-zero query over 33 candidates: rows 33 .. 63 of the chunk are expanded as zero descriptors (D = 0
    to this query) and must lose to the real candidate at D = 10, or to a real all-zero candidate"""
    c = Case(name, seed)
    c.stereo_form = stereo
    z = np.zeros(32, np.uint8)
    cd = [c.flip(255 - z, int(c.rng.integers(0, 60))) for _ in range(33)]  # D >= 196
    cd[17] = c.flip(z, 10)
    if zero_cand:
        cd[32] = z.copy()
    for j in range(33):
        c.c(cd[j], x=30.0 + j, ur=15.0 if stereo else -1.0)
    c.q("zero", z, "accepted", 32 if zero_cand else 17, ur=15.0 if stereo else -1.0)
    c.tri()
    return c


def _e_stereo_calls(c):
    """a stereo-form case also runs with bOnlyStereo; its exits there are the restatement's, not stated here"""
    if c.stereo_form:
        c.expect = {i: {"tri": e} for i, e in c.expect.items()}
        c.best = {i: {"tri": b} for i, b in c.best.items()}
        c.tri("only", only_stereo=True)
    return c


def group_e():
    cases = []
    for stereo in (False, True):
        s = "s" if stereo else "m"
        cases.append(_e_frame("e%s_n1_33_n2_0" % s, 10, 33, 0, stereo))  # first: the empty frame is frame 0 of its batch
        for n2 in E_N2[1:]:
            cases.append(_e_frame("e%s_n1_33_n2_%d" % (s, n2), 10 + n2, 33, n2, stereo))
        for n1 in E_N1:
            cases.append(_e_frame("e%s_n1_%d_n2_129" % (s, n1), 200 + n1, n1, 129, stereo))
        for k, winner, n2 in ((1, 27, 33), (2, 27, 33), (15, 27, 33), (16, 4, 33), (16, 40, 65), (16, 70, 129)):
            cases.append(_e_walk("e%s_walk%d_w%d" % (s, k, winner), 300 + k + winner, k, winner, n2, stereo))
        cases.append(_e_padding("e%s_pad" % s, 400, False, stereo))
        cases.append(_e_padding("e%s_pad_zero" % s, 401, True, stereo))
    return [_e_stereo_calls(c) for c in cases]


# ===================================================================== f. host-API dispatch of SearchForTriangulation
def _fill_node(c, node, nq, nc, tie_gaps=(), mp_kill=False):
    """node `node` with nq queries over nc candidates. The first queries are ties: two candidates at the same
    distance, `gap` positions apart (the later one wins), one per entry of tie_gaps that fits into the node; the
    others take the candidate at a position drawn from a permutation of the node. mp_kill: the first such
    candidate holds a MapPoint (its queries are left unchecked) and query 1 holds one"""
    cd = [c.desc() for _ in range(nc)]
    taken, qd, want = set(), [], []
    for t, gap in enumerate(tie_gaps):
        p = (5 * t + 1) % max(nc - gap, 1) if nc > gap else -1
        if len(qd) == nq or p < 0 or p in taken or p + gap in taken:
            continue
        d = c.desc()
        cd[p], cd[p + gap] = c.flip(d, 6), c.flip(d, 6)
        taken.update((p, p + gap))
        qd.append(d)
        want.append(p + gap)
    pos = c.rng.permutation(nc)
    for k in range(len(qd), nq):
        p = int(pos[k % nc])
        qd.append(c.flip(cd[p], 2 + k % 5))
        want.append(None if p in taken else p)   # a tie pair's position: whichever of the two the scan gives
    base2 = c.k2.n
    for j in range(nc):
        c.c(cd[j], x=20.0 + (j % 600), node=node)
    if mp_kill:
        killed = next((w for w in want if w is not None and w not in taken), None)
        if killed is not None:
            c.k2.mp[base2 + killed] = 1
            want = [None if w == killed else w for w in want]
    for k in range(nq):
        i = c.q("n%d_q%d" % (node, k), qd[k], None, None, x=20.0 + (k % 600), node=node)
        if mp_kill and k == 1:
            c.k1.mp[i] = 1
            c.expect[i] = "has_mp"
        elif want[k] is not None:
            c.expect[i], c.best[i] = "accepted", base2 + want[k]
    return base2


def group_f():
    cases = []
    for nc in (1, 63, 64, 65, 255, 256, 257, 513):
        c = Case("f_nc%d" % nc, 500 + nc)
        for node, nq in enumerate((1, 64, 65)):
            # gaps 1, 2, 3: the tie partners fall in different quarters (j mod 4); 256, 300: in different
            # 256-candidate rounds of k_tri_nodes
            _fill_node(c, 10 + 7 * node, nq, nc, tie_gaps=(1, 2, 3, 256, 300, 5), mp_kill=node == 1)
        c.k1.add(5.0, 100.0, c.desc(), node=3)   # nodes present on one side only, below, between and above
        c.k2.add(5.0, 100.0, c.desc(), node=12)
        c.k1.add(5.0, 100.0, c.desc(), node=900)
        c.k2.add(5.0, 100.0, c.desc(), node=901)
        c.tri("tri")
        c.tri("ori", check_ori=True)
        c.notes = dict(nc=nc)
        cases.append(c)
    c = Case("f_161_nodes", 600)
    for node in range(161):
        _fill_node(c, 5 + 2 * node, 3, 4, tie_gaps=(1,))
    c.tri()
    cases.append(c)
    c = Case("f_2049_entries", 601)   # the candidate side holds 2049 FeatureVector entries
    for node in range(8):
        _fill_node(c, 40 + node, 6, 256, tie_gaps=(3,))
    _fill_node(c, 90, 2, 1)
    c.tri()
    cases.append(c)
    return cases


# ===================================================================== g. SearchByBoW rules
def _bow_probe(c, name, hs, expect, best=None, node=0, ckw=None, qkw=None):
    kw = dict(mp=1)
    kw.update(qkw or {})
    ck = {k: dict(mp=1) for k in range(len(hs))}
    for k, v in (ckw or {}).items():
        ck[k].update(v)
    return c.probe(name, hs, expect, best, qkw=kw, ckw=ck, node=node)


def group_g():
    cases = []
    acc, th, rf = "accepted", "over_th_low", "ratio_fail"
    c = Case("g_th_low", 700)   # one node per query: no query sees another's candidates
    for k, (h, e0, e1) in enumerate(((49, acc, acc), (50, acc, th), (51, th, th))):
        _bow_probe(c, "b%d" % h, [h, 200], {"bow0": e0, "bow1": e1}, 0, node=k)
    _bow_probe(c, "single", [20], acc, 0, node=10)            # best2 stays 256
    _bow_probe(c, "equal", [20, 20], rf, node=11)             # best1 == best2
    _bow_probe(c, "equal0", [0, 0], rf, node=12)              # 0 < r * 0 is false
    _bow_probe(c, "dup_later", [10, 30, 10], rf, node=13)     # the duplicate is the second smallest
    _bow_probe(c, "first_min", [10, 30, 20], acc, 0, node=14)
    _bow_probe(c, "no_cand_mp", [5, 9], {"bow0": acc, "bow1": "no_candidate"}, {"bow0": 0, "bow1": None}, node=15,
               ckw={0: dict(mp=0), 1: dict(mp=1, bad=1)})
    # (KF,KF): the would-be second best has no MapPoint / a bad one and does not count
    _bow_probe(c, "second_no_mp", [10, 11, 40], {"bow0": rf, "bow1": acc}, {"bow0": None, "bow1": 0}, node=16,
               ckw={1: dict(mp=0)})
    _bow_probe(c, "second_bad", [10, 11, 40], {"bow0": rf, "bow1": acc}, {"bow0": None, "bow1": 0}, node=17,
               ckw={1: dict(bad=1)})
    _bow_probe(c, "q_no_mp", [5], "no_good_mp", node=18, qkw=dict(mp=0))
    _bow_probe(c, "q_bad", [5], "no_good_mp", node=19, qkw=dict(bad=1))
    c.k1.add(5.0, 5.0, c.desc(), mp=1, node=500)              # a node of one side only
    c.both_bow(0.75)
    cases.append(c)
    # ratio products: what the float comparison decides is recorded by the CPU test from the stats
    for ratio, pairs in ((0.75, ((30, 40), (30, 41))), (0.6, ((30, 50),)), (0.7, ((35, 50),)), (0.9, ((45, 50),))):
        c = Case("g_ratio_%s" % ratio, 710 + int(ratio * 100))
        for k, (b1, b2) in enumerate(pairs):
            lhs, rhs = f32(b1), f32(f32(ratio) * f32(b2))
            _bow_probe(c, "r%d_%d" % (b1, b2), [b1, b2], acc if lhs < rhs else rf, 0 if lhs < rhs else None, node=k)
        c.both_bow(ratio)
        c.notes = dict(ratio=ratio, pairs=pairs)
        cases.append(c)
    # greedy order: A takes X; B's best was X and it gets its next one, best2 over what remains. nq = 66 puts A and
    # B on both sides of the 64-query chunk edge; the case of 65 candidates also holds a node of 8, so that k_bow<true>
    # runs its staged branch and its lane-per-candidate branch
    def greedy_node(c, node, nc, nq):
        X = c.desc()
        cd = [c.desc() for _ in range(nc)]
        px, py, pz = nc - 1, nc // 2, 0
        cd[px] = X
        A, B = c.flip(X, 2), c.flip(X, 4)
        cd[py] = c.flip(B, 12)           # B's next one
        cd[pz] = c.flip(B, 40)           # and its second best over what remains: 12 < 0.75 * 40
        ids = [c.c(cd[j], node=node, mp=1) for j in range(nc)]
        ia, ib = (63, 64) if nq > 64 else (0, 2)
        for k in range(nq):
            if k == ia:
                c.q("A%d" % node, A, acc, ids[px], node=node, mp=1)
            elif k == ib:
                c.q("B%d" % node, B, acc, ids[py], node=node, mp=1)
            else:
                c.q("idle%d_%d" % (node, k), c.desc(), "over_th_low", node=node, mp=1)

    for nc, nq in ((8, 3), (65, 3), (513, 3), (8, 66), (65, 66), (513, 66)):
        c = Case("g_greedy_nc%d_nq%d" % (nc, nq), 720 + nc + nq)
        greedy_node(c, 0, nc, nq)
        if nc == 65:
            greedy_node(c, 1, 8, nq)
        c.both_bow(0.75)
        c.notes = dict(nc=nc, nq=nq)
        cases.append(c)
    # a node whose every candidate becomes matched before its queries end
    c = Case("g_exhausted", 730)
    cd = [c.desc() for _ in range(3)]
    for j in range(3):
        c.c(cd[j], node=0, mp=1)
    for k in range(5):
        c.q("q%d" % k, c.flip(cd[k % 3], 1 + k), acc if k < 3 else "no_candidate", k if k < 3 else None, node=0, mp=1)
    c.both_bow(0.75)
    cases.append(c)
    return cases


# ===================================================================== h. rotation
def _rot_case(name, seed, rots, F12=F_ROW):
    """one accepted match per entry of rots = [(angle1, angle2)]; the three functions run it"""
    c = Case(name, seed)
    for k, (a1, a2) in enumerate(rots):
        c.probe("r%d" % k, [4], None, None, qkw=dict(angle=a1, mp=1), ckw={0: dict(angle=a2, mp=1)}, node=k % 7)
    c.rots = rots
    c.both_bow(0.75, check_ori=True)
    return c


def _tri_twin(c, one_node):
    """the same pair without MapPoints, for SearchForTriangulation; one_node: every feature in node 0 (the probes
    keep descriptors of their own, so the matches are the same), which the brute-force batch can express"""
    t2 = Case(c.name + ("_tri" if one_node else "_trin"), 0)
    for src, dst in ((c.k1, t2.k1), (c.k2, t2.k2)):
        for i in range(src.n):
            dst.add(src.x[i], src.y[i], src.d[i], src.o[i], src.a[i], src.ur[i], 0, 0, 0 if one_node else src.node[i])
    t2.expect, t2.best, t2.names, t2.rots = dict(c.expect), dict(c.best), dict(c.names), c.rots
    t2.tri("ori", check_ori=True)
    return t2


def _bins(spec):
    """spec = {bin: count} -> (angle1, angle2) pairs whose rot lands in the middle of that bin"""
    out = []
    for b, cnt in spec.items():
        out += [(f32(30.0 * b), f32(0.0))] * cnt
    return out


def group_h():
    half = f32(15.0)
    singles = [(15.0, 0.0), (45.0, 0.0), (345.0, 0.0), (359.99, 0.0), (0.0, 0.0), (-0.0, 0.0), (0.0, 15.0),
               (10.0, 355.0), (f32(75.0), 0.0), (105.0, 0.0), (half * 3, 0.0), (200.0, 65.0)]
    specs = {
        "h_values": singles,
        "h_tie_first": _bins({2: 4, 5: 4, 9: 4, 11: 4}),           # four equal bins: the first three stay
        "h_tie_second": _bins({1: 6, 4: 3, 7: 3, 8: 3}),
        "h_tie_third": _bins({1: 6, 4: 5, 7: 2, 8: 2}),
        "h_cut_10_1": _bins({3: 10, 6: 1}),                        # 0.1f * 10 rounds to 1 in float (1.0000000149 unrounded): 1 < 1 is false, kept
        "h_cut_20_1_2": _bins({3: 20, 6: 1, 8: 2}),                # 0.1f * 20 is 2: max2 = 2 kept, max3 = 1 dropped
        "h_cut_20_2_1": _bins({3: 20, 6: 2, 8: 1}),
        "h_cut_11_1": _bins({3: 11, 6: 1}),                        # 1 < 1.1: max2 dropped
        "h_single_bin": _bins({12: 5}),
        "h_none": [],
    }
    cases = []
    for k, (name, rots) in enumerate(specs.items()):
        c = _rot_case(name, 800 + k, rots)
        if name == "h_none":
            c.probe("far", [80], None, None, qkw=dict(mp=1), ckw={0: dict(mp=1)})
        cases += [c, _tri_twin(c, True), _tri_twin(c, False)]
    return cases


def oracle_result(c, call, _memo={}):
    """the C oracle's (nmatches, matches) of one call of a case, computed once"""
    import oracle_py
    key = (c.name, call["key"])
    if key not in _memo:
        v1, v2 = c.views()
        if call["kind"] == "tri":
            _memo[key] = oracle_py.search_for_triangulation(v1, v2, c.F12, c.ex, c.ey, call["only_stereo"],
                                                            call["check_ori"])
        else:
            _memo[key] = oracle_py.search_by_bow(v1, v2, call["nnratio"], call["check_ori"],
                                                 other_is_keyframe=call["kind"] == "bow1")
    return _memo[key]


GROUPS = {"a": group_a, "b": group_b, "c": group_c, "d": group_d, "e": group_e, "f": group_f, "g": group_g,
          "h": group_h}
_cache = {}


def group(g):
    """the group's cases, built once and shared (views included): nobody writes to them"""
    if g not in _cache:
        _cache[g] = GROUPS[g]()
    return _cache[g]

"""Hand-made frames and MapPoints for the SearchByProjection family (ORBmatcher.cc:45-129, 290-403, 1328-1599) and
the two Fuse overloads (:825-1100): one named query (MapPoint) per edge of the algorithm.

A frame is arrays of x, y, octave, angle, descriptor, uRight and occupancy: no image, no extractor. A group holds
one 640x480 frame, a list of named queries and the calls (variant, th, flags) it is meant for; `expect` says which
exit of the reference each query is built to take in each call. Whether it really takes it is asserted on the CPU
from the restatements' stats (test_oracle_frame.py), never from the code under test.

Unit camera (fx = fy = 1, cx = cy = 0, identity pose, points (u z, v z, z) with z = 1, 2 or -1): the projection
is exact, so a query can sit on a bound. `real_group` uses the calibration and poses of proj_scenes.py.

Everything is inside the reference's domain: finite values, z != 0, octaves in [0, 8), n < 65536.
"""
import numpy as np

import orbamd

f32 = np.float32
W, H = 640, 480
NLEVELS = 8
KINDS = ("local", "last", "keyframe", "sim3", "fuse", "fuse_sim3")
THRESH = {"local": 100, "last": 100, "sim3": 50, "fuse": 50, "fuse_sim3": 50}  # TH_HIGH / TH_LOW (ORBmatcher.cc:37-38)
BF = 0.5  # stereo groups: mbf, and with fx = 1 also mb


def scale_table():
    s = [f32(1)]
    for _ in range(1, NLEVELS):
        s.append(f32(s[-1] * f32(1.2)))
    return np.array(s, f32)


SCALE = scale_table()
INV_SIGMA2 = (f32(1.0) / (SCALE * SCALE)).astype(f32)  # mvInvLevelSigma2


def up(v):
    return np.nextafter(f32(v), f32(np.inf), dtype=f32)


def down(v):
    return np.nextafter(f32(v), f32(-np.inf), dtype=f32)


def _kp(x, y, octave, angle):
    k = np.zeros(len(x), [("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("angle", "<f4")])
    k["x"], k["y"], k["octave"], k["angle"] = x, y, octave, angle
    return k


class Group:
    def __init__(self, name, seed, stereo=False, calib=(1.0, 1.0, 0.0, 0.0)):
        self.name, self.stereo, self.calib = name, stereo, calib
        self.rng = np.random.default_rng([290403, seed])
        self.fx, self.fy, self.fd, self.fo, self.fa, self.fur, self.focc, self.fname = [], [], [], [], [], [], [], []
        self.qs, self.expect, self.best, self.variants = [], {}, {}, []
        self.pairs, self.rescan = [], []  # arbitration: (loser, claimer, rank of the claimed entry); rescan query names
        self.Tcw = np.eye(4, dtype=f32)
        self._slots = iter([(60 + 40 * i, 60 + 40 * j) for j in range(9) for i in range(13)])
        self._frame = None

    # ---- primitives
    def slot(self):
        return next(self._slots)

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def flip(self, d, h):
        """d with exactly h bits flipped: Hamming distance h"""
        d = d.copy()
        for p in self.rng.permutation(256)[:h]:
            d[p >> 3] ^= np.uint8(1 << (p & 7))
        return d

    def feat(self, name, x, y, d, octave=0, angle=0.0, ur=-1.0, occ=0, at=None):
        assert 0 <= x < W and 0 <= y < H and 0 <= octave < NLEVELS and self._frame is None
        rec = (f32(x), f32(y), np.asarray(d, np.uint8), int(octave), f32(angle), f32(ur), int(occ), name)
        if at is None:
            at = len(self.fx)
            for lst in (self.fx, self.fy, self.fd, self.fo, self.fa, self.fur, self.focc, self.fname):
                lst.append(None)
        assert self.fname[at] is None or self.fname[at] == "filler"
        for lst, v in zip((self.fx, self.fy, self.fd, self.fo, self.fa, self.fur, self.focc, self.fname), rec):
            lst[at] = v
        return at

    def filler(self, n):
        """n level-7 features with random descriptors on a lattice: they fill the grid cells and the index range, and
        no query of level <= 5 can take them"""
        d = self.rng.integers(0, 256, (n, 32)).astype(np.uint8)
        for i in range(n):
            self.feat("filler", 5 + (i % 250) * 2.5, 5 + (i // 250) * 2.9, d[i], octave=7)

    def q(self, name, u, v, d, expect=None, best=None, level=0, z=1.0, **kw):
        """a MapPoint that projects to (u, v). expect / best: a string (every call), a dict by call key or kind
        ("*" = the rest), or a function of the call; best = the name of the feature an accepted query takes"""
        assert name not in self.expect and 0 <= level < NLEVELS and z != 0
        u, v, z = f32(u), f32(v), f32(z)
        pos = np.array([u * z, v * z, z], f32)
        assert f32(f32(pos[0]) * f32(1.0 / float(z))) == u and f32(f32(pos[1]) * f32(1.0 / float(z))) == v
        dist = f32(np.sqrt(float(pos[0]) ** 2 + float(pos[1]) ** 2 + float(pos[2]) ** 2))
        maxd = f32(dist * 1.2 ** (level - 0.5))
        rec = dict(name=name, u=u, v=v, desc=np.asarray(d, np.uint8), level=level, pos=pos, has_obs=1, skip=0, bad=0,
                   in_view=1, angle=f32(0), xr=f32(u - f32(f32(BF) * f32(1.0 / float(z)))), view_cos=f32(0.9),
                   min_dist=f32(maxd / 1.2 ** 7), max_dist=maxd, normal=(pos / dist).astype(f32), dist=dist)
        for k, val in kw.items():
            assert k in rec
            rec[k] = val
        self.qs.append(rec)
        self.expect[name] = expect
        self.best[name] = best
        return len(self.qs) - 1

    def idle(self, upto):
        """queries that find nothing, up to position `upto` of the query list (every one is active in every variant,
        so a query's position is its position in the device batch: the chunk of 64 it lands in)"""
        d = np.zeros(32, np.uint8)
        while len(self.qs) < upto:
            self.q("idle_%d" % len(self.qs), 20.0, 20.0, d)

    def variant(self, key, kind, th, **kw):
        c = dict(key=key, kind=kind, th=th, nnratio=0.8, bmono=False, check_ori=False, orb_dist=100, dz=0.0, nq=None)
        for k, v in kw.items():
            assert k in c
            c[k] = v
        c["thresh"] = c["orb_dist"] if kind == "keyframe" else THRESH[kind]
        self.variants.append(c)

    def all_kinds(self, r0, kinds=KINDS, **kw):
        """one call per kind, each with the th that gives a level-0 query the radius r0 (an integer: Sim3's th is int)"""
        assert r0 == int(r0)
        for kind in kinds:
            self.variant(kind, kind, r0 / 4.0 if kind == "local" else r0, **kw)

    # ---- what the entry points take
    def frame(self):
        if self._frame is None:
            n = len(self.fx)
            assert n < 65536 and all(v is not None for v in self.fx)
            k = _kp(np.array(self.fx, f32), np.array(self.fy, f32), np.array(self.fo, np.int32), np.array(self.fa, f32))
            fx, fy, cx, cy = self.calib
            self._frame = orbamd.FrameView(k, np.array(self.fd, np.uint8).reshape(n, 32), SCALE, W, H, fx, fy, cx, cy,
                                           bf=BF if self.stereo else 0.0,
                                           uright=np.array(self.fur, f32) if self.stereo else None,
                                           occupied=np.array(self.focc, np.uint8))
        return self._frame

    def mappoints(self, kind, nq=None):
        qs = self.qs if nq is None else self.qs[:nq]
        col = lambda k, dt, w=None: np.array([r[k] for r in qs], dt).reshape((len(qs), w) if w else (len(qs),))
        kw = dict(desc=col("desc", np.uint8, 32))
        if kind == "local":
            kw.update(bad=col("bad", np.uint8), has_obs=col("has_obs", np.uint8), track_in_view=col("in_view", np.uint8),
                      track_proj_x=col("u", f32), track_proj_y=col("v", f32), track_proj_xr=col("xr", f32),
                      track_level=col("level", np.int32), track_view_cos=col("view_cos", f32))
        elif kind == "last":
            kw.update(pos=col("pos", f32, 3), has_obs=col("has_obs", np.uint8), skip=col("skip", np.uint8),
                      octave=col("level", np.int32), angle=col("angle", f32))
        else:
            kw.update(pos=col("pos", f32, 3), min_dist=col("min_dist", f32), max_dist=col("max_dist", f32),
                      bad=col("bad", np.uint8), skip=col("skip", np.uint8))
            if kind == "keyframe":
                kw.update(angle=col("angle", f32))
            else:
                kw.update(normal=col("normal", f32, 3))
        return orbamd.MapPoints(len(qs), **kw)

    def calls(self):
        """[(call dict, F, MapPoints)]; call adds Tcw / Tl / Ow / inv for the kinds that take them"""
        out = []
        for c in self.variants:
            c = dict(c, Tcw=self.Tcw, Ow=np.zeros(3, f32), inv=INV_SIGMA2, group=self.name)
            Tl = self.Tcw.copy()
            Tl[2, 3] = f32(Tl[2, 3] + f32(c["dz"]))  # identity pose: tlc.z = dz exactly
            c["Tl"] = Tl
            out.append((c, self.frame(), self.mappoints(c["kind"], c["nq"])))
        return out

    def names(self, c):
        return [r["name"] for r in (self.qs if c["nq"] is None else self.qs[:c["nq"]])]

    def expected(self, c, name, table=None):
        e = (table or self.expect)[name]
        if callable(e):
            e = e(c)
        if isinstance(e, dict):
            e = e.get(c["key"], e.get(c["kind"], e.get("*")))
        return e

    def describe(self, c, feats=(), queries=()):
        """failure text: the cases behind differing feature / query indices"""
        names = self.names(c)
        return "%s/%s: features %s queries %s" % (self.name, c["key"], [(int(i), self.fname[i]) for i in feats][:8],
                                                   [(int(i), names[i]) for i in queries if 0 <= i < len(names)][:8])


def by_thresh(h):
    return lambda c: "accepted" if h <= c["thresh"] else "th_reject"


NOT_FUSE = lambda e: {"fuse": "th_reject", "*": e}  # Fuse's chi-square test rejects a candidate some pixels away


# ====================================================================================================== groups
def grid_group():
    """k_grid / PosInGrid and the cells at the borders; every query sits on its feature, level 0, radius 4"""
    g = Group("grid", 1)
    for name, x, y in (("col0", 2.0, 200.0), ("col1", 12.0, 240.0), ("col63", 634.0, 200.0), ("row0", 200.0, 3.0),
                       ("row1", 240.0, 11.0), ("row47", 200.0, 474.0), ("x634_99", 634.99, 280.0),
                       ("y474_99", 280.0, 474.99), ("cell_3071", 634.0, 474.0)):
        D = g.desc()
        g.feat(name, x, y, g.flip(D, 10))
        g.q(name, x, y, D, "accepted", best=name)
    # dropped from the grid (column 64 / row 48): the query on top of it takes the worse feature next to it, or nothing
    for name, x, y, wx, wy in (("x635_dropped", 635.0, 320.0, 633.0, 321.0), ("y475_dropped", 320.0, 475.0, 321.0, 473.0)):
        D = g.desc()
        g.feat(name, x, y, g.flip(D, 5))
        g.feat(name + "_worse", wx, wy, g.flip(D, 30))
        g.q(name, x, y, D, "accepted", best=name + "_worse")
    D = g.desc()
    g.feat("x639_9_dropped", 639.9, 360.0, g.flip(D, 5))
    g.q("x639_9_dropped", 639.9, 360.0, D, "no_candidates")
    # x * 0.1f exactly 10.5: roundf goes to column 11, so half_B (column 10, higher index) is scanned first
    D = g.desc()
    g.feat("half_A", 105.0, 200.0, g.flip(D, 20), octave=1)  # (levels 1 and 0: no ratio test in the local variant)
    g.feat("half_B", 103.0, 201.0, g.flip(D, 20))
    g.q("half_cell_x", 104.0, 200.5, D, "accepted", best="half_B", level=1)
    D = g.desc()
    g.feat("halfy_A", 300.0, 105.0, g.flip(D, 20), octave=1)
    g.feat("halfy_B", 301.0, 103.0, g.flip(D, 20))
    g.q("half_cell_y", 300.5, 104.0, D, "accepted", best="halfy_B", level=1)
    # 70 features in one cell (column 30, row 30); the best one is the 67th
    D = g.desc()
    for i in range(70):
        g.feat("cell70_%d" % i, 296.0 + (i % 8), 296.0 + (i // 8), g.flip(D, 12 if i == 66 else 20 + i))
    g.q("cell_70", 298.0, 303.0, D, "accepted", best="cell70_66")
    # projections outside the image: the four empty returns of GetFeaturesInArea (the local variant takes any u, v)
    D = g.desc()
    for name, u, v in (("out_right", 700.0, 200.0), ("out_left", -60.0, 200.0), ("out_below", 200.0, 540.0),
                       ("out_above", 200.0, -60.0)):
        g.q(name, u, v, D, {"local": "no_candidates", "*": "out_of_image"})
    g.all_kinds(4)
    return g


def clamp_group():
    """radius 80: windows that start outside the grid and are clamped back into it (local), the same projections
    dropped by the other variants"""
    g = Group("clamp", 2)
    for name, u, v, x, y in (("clamp_right", 700.0, 200.0, 630.0, 200.0), ("clamp_left", -60.0, 240.0, 10.0, 240.0),
                             ("clamp_below", 320.0, 540.0, 320.0, 470.0), ("clamp_above", 360.0, -60.0, 360.0, 8.0)):
        D = g.desc()
        g.feat(name, x, y, g.flip(D, 10))
        g.q(name, u, v, D, {"local": "accepted", "*": "out_of_image"}, best=name)
    g.all_kinds(80, kinds=("local", "last", "keyframe", "sim3"))
    return g


def wide_group():
    """radius 700 (840 at the queries' level 1) around the image centre: all 3072 cells. Four equal candidates in the
    corner cells, the first cell's with the highest index: the cell order decides, then each claimer takes the next"""
    g = Group("wide", 3)
    D = g.desc()
    for name, x, y in (("c3071", 634.0, 474.0), ("c63_0", 634.0, 3.0), ("c0_47", 2.0, 474.0), ("c0_0", 2.0, 3.0)):
        g.feat(name, x, y, g.flip(D, 20), octave=0 if name in ("c3071", "c0_47") else 1)
    order = ["c0_0", "c0_47", "c63_0", "c3071"]  # levels 1, 0, 1, 0: the local variant's ratio test never applies
    for i in range(4):
        g.q("wide_%d" % i, 320.0, 240.0, D, NOT_FUSE("accepted"), best={"fuse_sim3": "c0_0", "*": order[i]}, level=1)
    g.all_kinds(700)
    return g


def boundary_group():
    """|x_k - u| < r and |y_k - v| < r at r = 4: equal is outside, the float32 next to it is inside"""
    g = Group("boundary", 4)
    for name, axis, sign, inside in (("dx_eq_r", 0, 1, 0), ("dx_ulp_in", 0, 1, 1), ("dx_eq_r_neg", 0, -1, 0),
                                     ("dx_ulp_in_neg", 0, -1, 1), ("dy_eq_r", 1, 1, 0), ("dy_ulp_in", 1, 1, 1),
                                     ("dy_eq_r_neg", 1, -1, 0), ("dy_ulp_in_neg", 1, -1, 1)):
        x, y = g.slot()
        D = g.desc()
        g.feat(name, x, y, g.flip(D, 10))
        uv = [f32(x), f32(y)]
        e = f32(uv[axis] + f32(4 * sign))
        if inside:
            e = down(e) if sign > 0 else up(e)
        d = abs(f32(uv[axis] - e))
        assert (d == 4 and not inside) or (inside and 3.9999 < d < 4)  # one ulp of u, some 1e-5
        uv[axis] = e
        g.q(name, uv[0], uv[1], D, NOT_FUSE("accepted") if inside else "no_candidates", best=name)
    g.all_kinds(4)
    return g


def lanes_group():
    """radius 20 * 1.2f at (300, 200), level 1: a 7 x 7 window (49 cells, more than the 16 lanes of a query's scan
    group). Equal candidates in cells 8, 9 and 24 of the window (cells 8 and 24 belong to one lane), indices in
    reverse order, levels 1, 0, 1 (no ratio test)"""
    g = Group("lanes", 5)
    D = g.desc()
    r = f32(f32(20) * SCALE[1])
    x0, y0 = int(np.floor(f32(f32(300 - r) * f32(0.1)))), int(np.floor(f32(f32(200 - r) * f32(0.1))))
    ny = int(np.ceil(f32(f32(200 + r) * f32(0.1)))) - y0 + 1
    assert (x0, y0, ny) == (27, 17, 7)
    cell = lambda x, y: (int(np.floor(x * 0.1 + 0.5)) - x0) * ny + int(np.floor(y * 0.1 + 0.5)) - y0
    assert [cell(302, 203), cell(283, 190), cell(283, 183)] == [24, 9, 8]
    g.feat("cellk16", 302.0, 203.0, g.flip(D, 20), octave=1)
    g.feat("cellk1", 283.0, 190.0, g.flip(D, 20), octave=0)
    g.feat("cellk", 283.0, 183.0, g.flip(D, 20), octave=1)
    for i, b in enumerate(("cellk", "cellk1", "cellk16")):
        g.q("lanes_%d" % i, 300.0, 200.0, D, NOT_FUSE("accepted"), best={"fuse_sim3": "cellk", "*": b}, level=1)
    g.all_kinds(20)
    return g


def levels_group():
    """the minLevel / maxLevel forms of GetFeaturesInArea: per query level six or four features on one spot, the
    better the descriptor the further its level from the query's; each variant's level window picks another one"""
    g = Group("levels", 6, stereo=True)
    D3, D0 = g.desc(), g.desc()
    for lvl, h in ((7, 10), (5, 12), (1, 14), (4, 16), (2, 18), (3, 20)):
        g.feat("q3_l%d" % lvl, 200.0 + 0.25 * lvl, 200.0, g.flip(D3, h), octave=lvl)
    for lvl, h in ((7, 10), (2, 12), (1, 14), (0, 16)):
        g.feat("q0_l%d" % lvl, 400.0 + 0.25 * lvl, 200.0, g.flip(D0, h), octave=lvl)
    win = {"local": (2, 0), "last_fwd": (7, 7), "last_bwd": (1, 0), "last_eq_mb": (4, 1), "last_eq_neg_mb": (4, 1),
           "last_mono": (4, 1), "keyframe": (4, 1), "sim3": (2, 0), "fuse": (2, 0), "fuse_sim3": (2, 0)}
    g.q("level3", 201.0, 200.0, D3, "accepted", best={k: "q3_l%d" % a for k, (a, b) in win.items()}, level=3)
    g.q("level0", 401.0, 200.0, D0, "accepted", best={k: "q0_l%d" % b for k, (a, b) in win.items()}, level=0)
    g.variant("local", "local", 1.0)
    g.variant("last_fwd", "last", 4.0, dz=0.75)  # tlc.z > mb: GetFeaturesInArea(u, v, r, nLastOctave) -> (0, -1) at level 0
    g.variant("last_bwd", "last", 4.0, dz=-0.75)  # (0, nLastOctave)
    g.variant("last_eq_mb", "last", 4.0, dz=BF)  # tlc.z == mb: neither
    g.variant("last_eq_neg_mb", "last", 4.0, dz=-BF)
    g.variant("last_mono", "last", 4.0, dz=0.75, bmono=True)
    g.variant("keyframe", "keyframe", 4.0)
    g.variant("sim3", "sim3", 4)
    g.variant("fuse", "fuse", 4.0)
    g.variant("fuse_sim3", "fuse_sim3", 4.0)
    return g


def cand_group():
    """the per-candidate tests: uRight, Fuse's chi-square, the distance thresholds"""
    g = Group("cand", 7, stereo=True)

    def one(name, expect, ur, h=10, octave=0, dx=0.0, dy=0.0, level=0):
        x, y = g.slot()
        D = g.desc()
        xr = f32(f32(x) - f32(BF))
        g.feat(name, x + dx, y + dy, g.flip(D, h), octave=octave, ur=ur(xr) if callable(ur) else ur)
        g.q(name, x, y, D, expect, best=name, level=level)

    # uRight 0.0 and -1: no stereo test in the tracking variants (`> 0`); Fuse takes 0.0 as a stereo point (`>= 0`)
    one("ur_zero", {"fuse": "th_reject", "*": "accepted"}, 0.0)
    one("ur_minus1", "accepted", -1.0)
    one("ur_equal", "accepted", lambda xr: xr)
    # er == radius is kept, one ulp more is not (local, last-frame); Fuse: er^2 = 16 > 7.8
    one("er_eq_radius", {"fuse": "th_reject", "*": "accepted"}, lambda xr: f32(xr - f32(4)))
    one("er_ulp_over", {"local": "th_reject", "last": "th_reject", "fuse": "th_reject", "*": "accepted"},
        lambda xr: down(f32(xr - f32(4))))
    # chi-square on level 1 (invSigma2 = 1 / 1.44): 5.99 mono, 7.8 stereo
    one("chi2_mono_under", "accepted", -1.0, octave=1, level=1, dx=2.9, dy=0.4)
    one("chi2_mono_over", {"fuse": "th_reject", "*": "accepted"}, -1.0, octave=1, level=1, dx=2.9, dy=0.5)
    one("chi2_stereo_under", "accepted", lambda xr: f32(xr - f32(1.79)), octave=1, level=1, dx=2.0, dy=2.0)
    one("chi2_stereo_over", {"fuse": "th_reject", "*": "accepted"}, lambda xr: f32(xr - f32(1.81)), octave=1,
        level=1, dx=2.0, dy=2.0)
    for h in (50, 51, 64, 65, 100, 101):
        one("hamming_%d" % h, by_thresh(h), -1.0, h=h)
    # every candidate at distance 256; and a best whose only rival is at 256 (bestDist2 stays 256, bestLevel2 -1)
    x, y = g.slot()
    g.feat("all_256_a", x, y, np.zeros(32, np.uint8))
    g.feat("all_256_b", x + 1, y, np.zeros(32, np.uint8))
    g.q("all_256", x, y, np.full(32, 255, np.uint8), "th_reject")
    x, y = g.slot()
    ones = np.full(32, 255, np.uint8)
    g.feat("rival_256", x, y, np.zeros(32, np.uint8))
    g.feat("rival_best", x + 1, y, g.flip(ones, 40))
    g.q("rival_at_256", x, y, ones, "accepted", best="rival_best")
    g.all_kinds(4)
    g.variant("keyframe64", "keyframe", 4.0, orb_dist=64)
    g.variant("last_mono", "last", 4.0, bmono=True)
    return g


def ratio_group():
    """the local variant's ratio test (nnratio 0.8: 0.8f * 75 rounds to 60.0f), the order of ties, bFactor, the radius
    by viewing cosine. Candidates of one query share a grid cell, so the scan order is the index order."""
    g = Group("ratio", 8)
    assert f32(f32(0.8) * f32(75)) == f32(60)

    def case(name, cands, expect, best=0, level=1, **kw):
        x, y = g.slot()
        D = g.desc()
        for i, (h, lvl) in enumerate(cands):
            g.feat("%s_%d" % (name, i), x + 0.25 * i, y, g.flip(D, h), octave=lvl)
        g.q(name, x, y, D, expect, best="%s_%d" % (name, best) if expect == "accepted" else None, level=level, **kw)

    case("ratio_eq", [(60, 1), (75, 1)], "accepted")
    case("ratio_over", [(61, 1), (75, 1)], "ratio_reject")
    case("ratio_eq_levels", [(60, 1), (75, 0)], "accepted")
    case("ratio_over_levels", [(61, 1), (75, 0)], "accepted")
    case("single", [(90, 1)], "accepted")
    case("tie_5_5_same", [(50, 1), (50, 1)], "ratio_reject")
    case("tie_5_5_levels", [(50, 1), (50, 0)], "accepted")
    case("tie_5_5_levels_rev", [(50, 0), (50, 1)], "accepted")
    case("tie_50_45_50_first", [(50, 1), (45, 1), (50, 0)], "ratio_reject")  # second = the first 50 (level 1)
    case("tie_50_45_50_first_b", [(50, 0), (45, 1), (50, 1)], "accepted", best=1)  # second = the first 50 (level 0)
    case("tie_50_70_60", [(50, 1), (70, 0), (60, 1)], "ratio_reject")  # second = 60 (level 1), not 70 (level 0)
    case("tie_50_70_60_b", [(50, 1), (70, 1), (60, 0)], "accepted")
    # RadiusByViewingCos: `viewCos > 0.998` compares the float with a double; (float)0.998 is above the double
    for name, vc, e in (("viewcos_below", down(0.998), "accepted"), ("viewcos_0998", f32(0.998), "no_candidates"),
                        ("viewcos_above", up(0.998), "no_candidates")):
        x, y = g.slot()
        D = g.desc()
        g.feat(name, x + 3.0, y, g.flip(D, 10))
        g.q(name, x, y, D, e, best=name, view_cos=vc, level=0)
    # th == 1.0: r stays 4; th = 1.0001f: r = 4 * th
    x, y = g.slot()
    D = g.desc()
    g.feat("th_factor", x / 4.0 + 4.0, y + 20.0, g.flip(D, 10))
    g.q("th_factor", x / 4.0, y + 20.0, D, {"local": "no_candidates", "local_th": "accepted"}, best="th_factor", level=0)
    g.variant("local", "local", 1.0)
    g.variant("local_th", "local", 1.0001)
    return g


ARB_N = 40000


def arb_group():
    g = Group("arb", 9)
    g.filler(ARB_N)
    todo = []  # (position, function that adds the query)

    claim_kinds = ("local", "last", "keyframe", "sim3")

    def at(pos, name, x, y, D, expect, best, level=1, **kw):
        if isinstance(expect, str):  # (the Fuse calls on this frame claim nothing: only equality there)
            expect = {k: expect for k in claim_kinds}
        if isinstance(best, str):
            best = {k: best for k in claim_kinds}
        todo.append((pos, lambda: g.q(name, x, y, D, expect, best=best, level=level, **kw)))

    def pair(name, pc, pl, ia, ib):
        """claimer at position pc and loser at pl share their best feature A (level 1); the loser then takes B
        (level 0: the local variant's ratio test does not apply)"""
        x, y = g.slot()
        D = g.desc()
        g.feat(name + "_A", x, y, g.flip(D, 10), octave=1, at=ia)
        g.feat(name + "_B", x + 1.0, y, g.flip(D, 30), octave=0, at=ib)
        at(pc, name + "_claimer", x, y, D, "accepted", name + "_A")
        at(pl, name + "_loser", x, y, D, "accepted", name + "_B")
        g.pairs.append((name + "_loser", name + "_claimer", 0))

    pair("far", 5, 200, 7, 20000)
    pair("adjacent", 10, 11, 100, 101)
    pair("chunk_edge", 63, 64, 200, 201)
    pair("idx_last", 12, 14, ARB_N - 1, ARB_N - 2)  # the last index, claimed; its neighbour taken by the loser
    pair("idx_32768", 16, 17, 32768, 32767)
    # six equal MapPoints over six features of one window, levels alternating: each takes the next best; the scan keeps
    # four keys, so the fifth and sixth need the whole-wave rescan
    x, y = g.slot()
    D = g.desc()
    for i in range(6):
        g.feat("six_%d" % i, x + 0.25 * i, y, g.flip(D, 10 + i), octave=i % 2, at=300 + 7 * i)
    for i in range(6):
        at(20 + i, "six_obs_%d" % i, x, y, D, "accepted", "six_%d" % i)
    g.rescan += ["six_obs_4", "six_obs_5"]
    # the same without observations: nothing is claimed in the local and last-frame variants, all six write the first
    # feature, the last writer stays and the count is 6; the keyframe and Sim3 variants claim regardless
    x, y = g.slot()
    D = g.desc()
    for i in range(6):
        g.feat("noobs_%d" % i, x + 0.25 * i, y, g.flip(D, 10 + i), octave=i % 2, at=400 + 7 * i)
    for i in range(6):
        soft = "overwritten" if i < 5 else "accepted"
        at(30 + i, "six_noobs_%d" % i, x, y, D, {"local": soft, "last": soft, "keyframe": "accepted", "sim3": "accepted"},
           {"local": "noobs_0", "last": "noobs_0", "keyframe": "noobs_%d" % i, "sim3": "noobs_%d" % i}, has_obs=0)
    g.rescan_claiming = ["six_noobs_4", "six_noobs_5"]  # (keyframe, Sim3)
    # claim-table collisions: the bests of two queries of one round are features a and a + 2048 / a + 4096
    for name, p0, a, b in (("collide_2048", 40, 1000, 3048), ("collide_4096", 44, 5000, 9096)):
        for k, idx in enumerate((a, b)):
            x, y = g.slot()
            D = g.desc()
            g.feat("%s_%d" % (name, k), x, y, g.flip(D, 10), octave=1, at=idx)
            at(p0 + k, "%s_%d" % (name, k), x, y, D, "accepted", "%s_%d" % (name, k))
    # a feature occupied on entry that is the best of three queries: each takes its own second
    x, y = g.slot()
    D = g.desc()
    g.feat("occupied_best", x, y, g.flip(D, 5), octave=1, occ=1, at=35000)
    for k in range(3):
        g.feat("occupied_alt_%d" % k, x + 1.0 + k, y, g.flip(D, 20 + k), octave=k % 2, at=36000 + k)
        at(50 + k, "occupied_%d" % k, x, y, D, "accepted", "occupied_alt_%d" % k)
    # the local variant's ratio test after a claim (the loser's candidates share level 1). second_claimed: A 50, B 55,
    # C 90 -> 50 > 0.8 * 55 rejects, but B is claimed first, and 50 <= 0.8 * 90 accepts. best_claimed: A 40, B 50,
    # C 55 -> accepted on A unless A is claimed: then B against C fails
    x, y = g.slot()
    D = g.desc()
    B = g.flip(D, 55)
    E = g.flip(B, 5)  # the claimer's descriptor: 5 from B, some 80 from A and C
    g.feat("sc_A", x, y, g.flip(D, 50), octave=1, at=15000)
    g.feat("sc_B", x + 0.5, y, B, octave=1, at=15001)
    g.feat("sc_C", x + 1.0, y, g.flip(D, 90), octave=1, at=15002)
    at(210, "second_claimer", x, y, E, {"local": "accepted"}, {"local": "sc_B"})
    at(212, "second_claimed_loser", x, y, D, {"local": "accepted"}, {"local": "sc_A"})
    g.pairs.append(("second_claimed_loser", "second_claimer", 1))
    x, y = g.slot()
    D = g.desc()
    A = g.flip(D, 40)
    E = g.flip(A, 5)
    g.feat("bc_A", x, y, A, octave=1, at=16000)
    g.feat("bc_B", x + 0.5, y, g.flip(D, 50), octave=1, at=16001)
    g.feat("bc_C", x + 1.0, y, g.flip(D, 55), octave=1, at=16002)
    at(214, "best_claimer", x, y, E, {"local": "accepted"}, {"local": "bc_A"})
    at(215, "best_claimed_loser", x, y, D, {"local": "ratio_reject"}, None)
    g.pairs.append(("best_claimed_loser", "best_claimer", 0))
    for pos, add in sorted(todo, key=lambda t: t[0]):
        g.idle(pos)
        assert len(g.qs) == pos
        add()
    g.idle(220)
    for kind in ("local", "last", "keyframe", "sim3"):
        th = 1.0 if kind == "local" else 4
        g.variant(kind, kind, th)
        for nq in (0, 1, 63, 64, 65):
            g.variant("%s_nq%d" % (kind, nq), kind, th, nq=nq)
    g.variant("fuse", "fuse", 4.0)
    g.variant("fuse_sim3", "fuse_sim3", 4.0)
    return g


def rot_group():
    """the rotation-consistency filter of the last-frame and keyframe variants. Query i sits on its own feature
    (angle 20) with angle 20 + rot; the calls truncate the list (nq), so one list gives several histograms:
    (The bin is round(rot / 30) with rot in [0, 360], 0 to 12: `bin == HISTO_LENGTH` cannot happen, no case for it.)
    20 x bin 0 | 2 x bin 5 | 2 x bin 9 | 2 x bin 12 (rot slightly negative) | 2 x rot * (1/30) == 0.5 | the shared feature"""
    g = Group("rot", 10)
    base = f32(20.0)
    tiny = f32(down(base) - base)  # the smallest negative rot at 20
    half = f32(15.0)
    assert f32(half * (f32(1) / f32(30))) == f32(0.5) and f32(tiny + f32(360)) == f32(360)
    rots = [0.0] * 20 + [150.0] * 2 + [270.0] * 2 + [tiny] * 2 + [half] * 2
    for i, r in enumerate(rots):
        x, y = g.slot()
        D = g.desc()
        a2 = base
        a1 = f32(base + f32(r))
        if i == 0:
            a1, a2 = f32(-0.0), f32(0.0)  # rot = -0.0: not < 0
        elif i == 1:
            a1, a2 = f32(0.0), f32(0.0)
        assert i < 2 or f32(a1 - a2) == f32(r)
        g.feat("rot_%d" % i, x, y, g.flip(D, 10), angle=a2)
        # exits per call are set by expect_rot below
        g.q("rot_%d" % i, x, y, D, lambda c, i=i: expect_rot(c, i), best="rot_%d" % i, angle=a1)
    # one feature, two queries without observations (last-frame: no claim): the first in a discarded bin, the second in
    # bin 0. The reference resets the feature once and subtracts one; the keyframe variant claims, so the second misses
    x, y = g.slot()
    D = g.desc()
    g.feat("shared", x, y, g.flip(D, 10), angle=base)
    g.q("shared_discarded", x, y, D, lambda c: expect_rot(c, 28), best="shared", angle=f32(base + f32(200.0)), has_obs=0)
    g.q("shared_kept", x, y, D, lambda c: expect_rot(c, 29), best={"last": "shared"}, angle=base, has_obs=0)
    for kind in ("last", "keyframe"):
        for nq in (20, 21, 22, 23, 24, 26, 28, 30):
            g.variant("%s_nq%d" % (kind, nq), kind, 4.0, nq=nq, check_ori=True)
        g.variant("%s_noori" % kind, kind, 4.0, nq=30, check_ori=False)
    return g


def expect_rot(c, i):
    """exit of query i of rot_group in call c, worked out by hand from ComputeThreeMaxima"""
    nq, kind = c["nq"], c["kind"]
    bins = [0] * 20 + [5] * 2 + [9] * 2 + [12] * 2 + [1] * 2 + [7, 0]
    if not c["check_ori"]:
        if i == 28:
            return "overwritten" if kind == "last" else "accepted"
        if i == 29:
            return "accepted" if kind == "last" else "th_reject"
        return "accepted"
    if kind == "keyframe" and i == 29:
        return "th_reject"  # the feature is claimed by query 28
    size = {}
    for b in bins[:nq]:
        size[b] = size.get(b, 0) + 1
    if kind == "keyframe" and nq == 30:
        size[0] -= 1  # query 29 found its feature claimed
    # bin 0 is the largest (20 or 21). ComputeThreeMaxima keeps the next two by size, the lower bin index first among
    # equals, if they pass `max < 0.1f * max1`: 0.1f * 20 = 2.0f, so a bin of 2 stays and a bin of 1 goes, and when the
    # second goes the third goes with it; 0.1f * 21 = 2.1f drops a bin of 2
    others = sorted((-n, b) for b, n in size.items() if b != 0)[:2]
    limit = 2 if size[0] == 20 else 3
    kept = {0}
    if others and -others[0][0] >= limit:
        kept.add(others[0][1])
        if len(others) > 1 and -others[1][0] >= limit:
            kept.add(others[1][1])
    if bins[i] not in kept:
        return "rot_removed"
    if i == 29:
        return "overwritten"  # counted, but the feature was reset by query 28's bin
    return "accepted"


def raw_scale(max_dist, dist):
    """MapPoint::PredictScale before its clamps (MapPoint.cc:385-417; log of a float = logf)"""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    ratio = f32(f32(max_dist) / f32(dist))
    return int(np.ceil(f32(f32(libm.logf(float(ratio))) / f32(np.log(f32(1.2))))))


def front_group():
    """the projection front half (host code): image bounds, depth, the distance and viewing-angle tests, PredictScale,
    the flags. Radius 3."""
    g = Group("front", 11)

    def one(name, u, v, expect, fx=None, fy=None, level=0, foct=0, **kw):
        D = g.desc()
        if fx is not None:
            g.feat(name, fx, fy, g.flip(D, 10), octave=foct)
        return g.q(name, u, v, D, expect, best=name, level=level, **kw)

    # u == mnMaxX, v == mnMaxY: `u > mnMaxX` keeps it (last-frame, keyframe), IsInImage's `u < mnMaxX` drops it. (Level 7,
    # radius 10.7: a feature within 3 px of the edge rounds to column 64 and is in no cell)
    one("u_eq_maxx", 640.0, 100.0, {"sim3": "out_of_image", "fuse": "out_of_image", "fuse_sim3": "out_of_image",
                                    "*": "accepted"}, 632.0, 100.0, level=7, foct=7)
    one("v_eq_maxy", 100.0, 480.0, {"sim3": "out_of_image", "fuse": "out_of_image", "fuse_sim3": "out_of_image",
                                    "*": "accepted"}, 100.0, 472.0, level=7, foct=7)
    one("u_below_0", down(0.0), 140.0, {"local": "accepted", "*": "out_of_image"}, 1.0, 140.0)
    one("v_below_0", 140.0, down(0.0), {"local": "accepted", "*": "out_of_image"}, 140.0, 1.0)
    one("u_eq_0", 0.0, 180.0, "accepted", 1.0, 180.0)
    # behind the camera, projecting into the image: only the keyframe variant has no depth test
    one("behind", 300.0, 100.0, {"local": "accepted", "keyframe": "accepted", "*": "depth"}, 300.0, 100.0, z=-1.0)
    one("depth_2", 340.0, 100.0, "accepted", 340.0, 100.0, z=2.0)

    def edge(mult, target, over):
        """a float m with (float)(mult * m) == target, or the next one, whose product is above / below it"""
        m = f32(float(target) / float(mult))
        while f32(f32(mult) * m) > target:
            m = down(m)
        while f32(f32(mult) * m) < target:
            m = up(m)
        assert f32(f32(mult) * m) == target
        if over > 0:
            while f32(f32(mult) * m) <= target:
                m = up(m)
        if over < 0:
            while f32(f32(mult) * m) >= target:
                m = down(m)
        return m

    # dist3D == 0.8f * min_dist and == 1.2f * max_dist pass (`<`, `>`); one float further fails. |(4, 8, 1)| = 9 etc.
    dr = {"local": "accepted", "last": "accepted", "*": "dist_range"}
    one("dist_eq_min", 4.0, 8.0, "accepted", 4.0, 8.0, min_dist=edge(0.8, 9.0, 0), max_dist=f32(9.0))
    one("dist_below_min", 8.0, 4.0, dr, 8.0, 4.0, min_dist=edge(0.8, 9.0, 1), max_dist=f32(9.0))
    one("dist_eq_max", 12.0, 12.0, "accepted", 12.0, 12.0, max_dist=edge(1.2, 17.0, 0))
    one("dist_above_max", 6.0, 18.0, dr, 6.0, 18.0, max_dist=edge(1.2, 19.0, -1))
    # PO . n == 0.5 * dist passes (`<`); |(18, 6, 1)| = 19, |(2, 2, 1)| = 3
    va = {"sim3": "view_angle", "fuse": "view_angle", "fuse_sim3": "view_angle", "*": "accepted"}
    one("normal_eq_half", 18.0, 6.0, "accepted", 18.0, 6.0, normal=np.array([0, 0, 9.5], f32))
    one("normal_below_half", 2.0, 2.0, va, 2.0, 2.0, normal=np.array([0, 0, down(1.5)], f32))
    # PredictScale's lower clamp: nScale = -1 needs max_dist / dist <= 1 / 1.2 in float while `dist > 1.2f * max_dist` is
    # still false. That holds where 1.2f * max_dist is rounded up to dist: the smallest max_dist that passes the test,
    # at the first point of the row for which logf(ratio) / logf(1.2f) comes out below -1
    for u in range(300, 340):
        dist = f32(np.sqrt(float(u) ** 2 + 300.0 ** 2 + 1.0))
        m = f32(float(dist) / 1.2)
        while f32(f32(1.2) * m) < dist:
            m = up(m)
        while f32(f32(1.2) * down(m)) >= dist:
            m = down(m)
        if raw_scale(m, dist) == -1:
            break
    else:
        raise AssertionError("no point of the row reaches PredictScale's lower clamp")
    i = one("scale_low", float(u), 300.0, "accepted", float(u), 300.0)
    assert g.qs[i]["dist"] == dist
    g.qs[i]["max_dist"] = m
    g.qs[i]["min_dist"] = f32(1.0)
    # and the upper one: log ratio / log 1.2 about 12.6 is clamped to the last level
    i = one("scale_high", 400.0, 300.0, "accepted", 400.0, 300.0, level=7, foct=7)
    g.qs[i]["max_dist"] = f32(float(g.qs[i]["dist"]) * 10.0)
    g.qs[i]["min_dist"] = f32(1.0)
    # flags: each variant reads its own
    one("flag_skip", 200.0, 380.0, {"local": "accepted", "*": "skipped"}, 200.0, 380.0, skip=1)
    one("flag_bad", 240.0, 380.0, {"last": "accepted", "*": "skipped"}, 240.0, 380.0, bad=1)
    one("flag_not_in_view", 280.0, 380.0, {"local": "skipped", "*": "accepted"}, 280.0, 380.0, in_view=0)
    g.all_kinds(3)
    return g


def empty_group():
    """a frame without features"""
    g = Group("empty", 12)
    for i in range(3):
        g.q("nothing_%d" % i, 100.0 + i, 100.0, g.desc(), "no_candidates")
    g.all_kinds(4)
    g.variant("last_ori", "last", 4.0, check_ori=True)
    return g


def real_group():
    """ordinary arithmetic: the calibration of proj_scenes.py, a rotated pose, MapPoints back-projected from
    hand-placed features that include the border cells; no expectations, only equality"""
    import proj_scenes as ps
    g = Group("real", 13, calib=(ps.FX, ps.FY, ps.CX, ps.CY))
    rng = g.rng
    g.Tcw = ps.pose(ps.rot(rng, 3.0), rng.normal(0, 0.05, 3))
    xs = [1.0, 4.0, 9.0, 14.0, 626.0, 631.0, 636.0, 639.0] + list(np.arange(40.0, 600.0, 47.0))
    ys = [1.0, 4.0, 9.0, 14.0, 466.0, 471.0, 476.0, 479.0] + list(np.arange(40.0, 440.0, 53.0))
    pts = [(x, y) for x in xs for y in ys]
    k = np.zeros(len(pts), [("x", "<f4"), ("y", "<f4"), ("octave", "<i4")])
    k["x"], k["y"] = [p[0] for p in pts], [p[1] for p in pts]
    k["octave"] = rng.integers(0, 4, len(pts))
    Xw = ps.backproject(rng, k, np.arange(len(pts)), g.Tcw)
    R, t = g.Tcw[:3, :3].astype(np.float64), g.Tcw[:3, 3].astype(np.float64)
    Ow = -(R.T @ t)
    for i, (x, y) in enumerate(pts):
        D = g.desc()
        ang = float(rng.uniform(0, 360))
        g.feat("f%d" % i, x, y, g.flip(D, int(rng.integers(0, 60))), octave=int(k["octave"][i]), angle=ang)
        lvl = int(k["octave"][i])
        qi = g.q("p%d" % i, x, y, D, None, level=lvl, angle=f32((ang + rng.normal(0, 20)) % 360),
                 has_obs=int(rng.random() < 0.8))
        r = g.qs[qi]
        r["pos"] = Xw[i]
        po = Xw[i].astype(np.float64) - Ow
        r["dist"] = f32(np.linalg.norm(po))
        r["max_dist"] = f32(r["dist"] * 1.2 ** (lvl - 0.5))
        r["min_dist"] = f32(r["max_dist"] / 1.2 ** 7)
        r["normal"] = (po / np.linalg.norm(po)).astype(f32)
    g.all_kinds(8)
    g.variant("last_ori", "last", 8.0, check_ori=True)
    g.variant("keyframe_ori", "keyframe", 8.0, check_ori=True)
    return g


_BUILDERS = {"grid": grid_group, "clamp": clamp_group, "wide": wide_group, "boundary": boundary_group,
             "lanes": lanes_group, "levels": levels_group, "cand": cand_group, "ratio": ratio_group, "arb": arb_group,
             "rot": rot_group, "front": front_group, "empty": empty_group, "real": real_group}
# large then small, so that a context reused across consecutive groups would show stale scratch
GROUPS = ["arb", "grid", "wide", "cand", "clamp", "boundary", "lanes", "levels", "ratio", "rot", "front", "empty", "real"]
FUSE_GROUPS = [n for n in GROUPS if n not in ("clamp", "ratio", "rot", "empty")]  # a Fuse call on a frame with features
_cache = {}


def group(name):
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


# ====================================================================================================== running a call
def run_oracle(c, F, mps):
    """(count, match[F.n]) or for the Fuse kinds (count, best_idx[mps.n]) from the CPU oracle"""
    import oracle_py as o
    k = c["kind"]
    if k == "local":
        return o.search_by_projection_local(F, mps, c["th"], c["nnratio"])
    if k == "last":
        return o.search_by_projection_last_frame(F, c["Tcw"], mps, c["Tl"], c["th"], c["bmono"], c["check_ori"])
    if k == "keyframe":
        return o.search_by_projection_keyframe(F, c["Tcw"], mps, c["th"], c["orb_dist"], c["check_ori"])
    if k == "sim3":
        return o.search_by_projection_sim3(F, c["Tcw"], mps, c["th"])
    if k == "fuse":
        return o.fuse(F, c["Tcw"], c["Ow"], mps, c["th"], c["inv"])
    return o.fuse_sim3(F, c["Tcw"], mps, c["th"])


def run_gpu(mt, c, F, mps, cache=None, key=0):
    """the same through an orbamd.ORBmatcher (one matcher, hence one device context, for every call); with a
    KeyFrameCache the Fuse kind goes through FuseCached"""
    k = c["kind"]
    mt.mfNNratio, mt.mbCheckOrientation = float(c["nnratio"]), bool(c["check_ori"])
    if k == "local":
        return mt.SearchByProjectionLocal(F, mps, c["th"])
    if k == "last":
        return mt.SearchByProjectionLastFrame(F, c["Tcw"], mps, c["Tl"], c["th"], c["bmono"])
    if k == "keyframe":
        return mt.SearchByProjectionKeyFrame(F, c["Tcw"], mps, c["th"], c["orb_dist"])
    if k == "sim3":
        return mt.SearchByProjectionSim3(F, c["Tcw"], mps, c["th"])
    if k == "fuse":
        if cache is not None:
            return mt.FuseCached(cache, key, F, c["Tcw"], c["Ow"], mps, c["th"], c["inv"])
        return mt.Fuse(F, c["Tcw"], c["Ow"], mps, c["th"], c["inv"])
    return mt.FuseSim3(F, c["Tcw"], mps, c["th"])

"""Hand-made inputs for ORBextractor::operator(), one named case per edge of the extractor (no GPU, no oracle).

Pure numpy and integer arithmetic, so every machine builds the same bytes. A case is (name, image, extractor
parameters, expect): `expect(r)` asserts, from the result and the `stats` of tests/extract_py.py (r.kps, r.desc,
r.stages, r.stats), that the image reached the branch its name claims; tests/test_oracle_extract.py runs it for every
case, so a case that misses its branch fails on the CPU. Cases that share a size and a parameter set form one group:
the GPU tests batch a group's images into one tensor.

Geometry of the common 120x100 level (ORBextractor.cc:773-806): borders 16, two cell columns x in [16,66) and [60,104),
two cell rows y in [16,56) and [50,84) (the second ones clamped to maxBorder); cv::FAST leaves a 3-px inset, so the
columns detect x in 19..62 and 63..100 and the rows y in 19..52 and 53..80: no pixel is detected by two cells."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name image params expect")
# params: (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
        (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
W0, H0 = 120, 100
FAST_PARAMS = [(20, 7), (21, 8), (7, 7), (7, 20), (1, 0), (255, 254)]
# Geometry::build's LDS key limit at 256 octree nodes (extract.cpp key_lds, restated in key_limit below). The product has
# no getter for it: key_limit and the constants of resize_fits must move together with extract.cpp / orb_device.h, or
# octree/global_scratch and the pyramid/scale_* cases stop reaching the instantiations their names claim.
KL_256 = 1888


def key_limit(nfeat0, nIni=1):
    """Geometry::build: keys of a level stay in LDS up to KL (node tables of NC = pow2 >= node_cap entries, 76 B
    each)"""
    cap = max(nfeat0 + 3, 4 * nIni)
    nc = 1
    while nc < cap:
        nc <<= 1
    nb = 76 * nc
    kl32 = ((32 * 1024 - nb - 64) // 7) & ~15
    return min(2048, kl32) if kl32 >= 1024 else min(2048, ((160 * 1024 - nb) // 7) & ~15)


def resize_fits(sw, sh, dw, dh):
    """Geometry::build's tables for the resize of a (sw, sh) level to (dw, dh), and its two checks restated:
    returns (xmax, resize_tile_fits, build_pyr_tables). xmax < dw: the last columns' second tap is past the row.
    Tile: a 64 x 32 output tile's source window within 144 x 48 (extract_kernels.hip kRsW / kRsH). Tables: at most
    2048 rows and 1024 four-column groups, and each group's taps inside an 8-byte source window."""
    scale_x, scale_y = 1.0 / (dw / sw), 1.0 / (dh / sh)
    xofs, xmax = [], dw
    for dx in range(dw):
        sx = int(np.floor(np.float32((dx + 0.5) * scale_x - 0.5)))
        sx = max(sx, 0)
        if sx + 1 >= sw:
            xmax = min(xmax, dx)
            sx = min(sx, sw - 1)
        xofs.append(sx)
    yofs = [int(np.floor(np.float32((dy + 0.5) * scale_y - 0.5))) for dy in range(dh)]
    tile = True
    for c0 in range(0, dw, 64):
        c1 = min(c0 + 64, dw)
        hi = min(xofs[c1 - 1] + 1, sw - 1)
        tile &= hi - xofs[c0] + 1 + 3 + 4 <= 144
    for r0 in range(0, dh, 32):
        r1 = min(r0 + 32, dh)
        lo, hi = min(max(yofs[r0], 0), sh - 1), min(max(yofs[r1 - 1] + 1, 0), sh - 1)
        tile &= hi - lo + 1 <= 48
    tables = dh <= 2048 and (dw + 3) // 4 <= 1024 and sw >= 12
    au = (sw + 3) // 4 * 4
    for gi in range((dw + 3) // 4):
        win = min(xofs[4 * gi], au - 8)
        for i in range(4):
            x = min(4 * gi + i, dw - 1)
            o = xofs[x] - win
            if o < 0 or o > 7 or (x < xmax and o + 1 > 7):
                tables = False
    return xmax, bool(tile), bool(tables)


def flat(v=100, w=W0, h=H0):
    return np.full((h, w), v, np.uint8)


def noise(w, h, seed, lo=0, hi=255):
    """integer hash noise (splitmix64 finaliser), the same bytes everywhere"""
    x = np.arange(w * h, dtype=np.uint64) + np.uint64(seed * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return (np.uint64(lo) + (x >> np.uint64(33)) % np.uint64(hi - lo + 1)).astype(np.uint8).reshape(h, w)


def dots(img, pts):
    """pts: (x, y, value)"""
    for x, y, v in pts:
        img[y, x] = v
    return img


def lattice(img, dx, dy, value, x0=19, y0=19):
    h, w = img.shape
    img[y0:h - 19:dy, x0:w - 19:dx] = value
    return img


def textured_frame(img, seed):
    """full-range noise on the outer 4 px: outside every FAST ring and every IC_Angle patch, inside what
    GaussianBlur's REFLECT_101 mirrors for a descriptor read 1 px from the edge (a flat border would make a clamped
    border indistinguishable from the reflected one)"""
    h, w = img.shape
    n = noise(w, h, seed)
    for sl in ((slice(0, 4), slice(None)), (slice(h - 4, h), slice(None)), (slice(None), slice(0, 4)),
               (slice(None), slice(w - 4, w))):
        img[sl] = n[sl]
    return img


def arc(img, cx, cy, start, n, value):
    for k in range(n):
        dx, dy = RING[(start + k) % 16]
        img[cy + dy, cx + dx] = value
    return img


# ------------------------------------------------------------------------------ result helpers ---
def cand(r, l=0):
    """{(x, y): [responses]} of level l's vToDistributeKeys in level coordinates"""
    out = {}
    for x, y, s in r.stages[l]["candidates"]:
        out.setdefault((int(x) + 16, int(y) + 16), []).append(int(s))
    return out


def cell(r, i, j, l=0):
    for c in r.stats["levels"][l]["cells"]:
        if c["i"] == i and c["j"] == j:
            return c
    raise KeyError((i, j))


def kstat(r, x, y, l=0):
    for k in r.stats["keypoints"]:
        if (k["level"], k["x"], k["y"]) == (l, x, y):
            return k
    raise KeyError((l, x, y))


def kp_of(r, x, y, l=0):
    for n, k in enumerate(r.stats["keypoints"]):
        if (k["level"], k["x"], k["y"]) == (l, x, y):
            return r.kps[n]
    raise KeyError((l, x, y))


def _exactly(pts, l=0):
    """level l's candidates are exactly pts: {(x, y): response}"""
    def f(r):
        got = {k: v for k, v in cand(r, l).items()}
        assert got == {k: [v] for k, v in pts.items()}, got
    return f


# ------------------------------------------------------------------------------- FAST definition ---
def _base(c, bright):
    if bright:
        return 100 if 100 + c <= 255 else 0
    return 100 if 100 - c >= 0 else 255


def fast_cases(ini, mn):
    P = (500, 1.2, 1, ini, mn)
    pre = "fast_%d_%d/" % (ini, mn)
    out = []
    seen = set()
    for which, t in (("ini", ini), ("min", mn)):
        for step in (0, 1):
            c = t + step
            if c > 255 or c < 1 or c in seen:
                continue
            seen.add(c)
            for bright in (True, False):
                b = _base(c, bright)
                img = dots(flat(b), [(40, 40, b + c if bright else b - c)])
                # a score of 0 is no keypoint (the NMS compares it with the zeros around it)
                hit = (c > ini or c > mn) and c - 1 > 0
                th = ini if c > ini else mn

                def exp(r, hit=hit, c=c, th=th):
                    _exactly({(40, 40): c - 1} if hit else {})(r)
                    assert len(r.kps) == int(hit)
                    assert cell(r, 0, 0)["threshold"] == (th if hit else None)
                    if hit:
                        assert r.kps[0]["response"] == c - 1
                out.append(Case("%sdot_%s_t%s_%s" % (pre, which, "+1" if step else "", "bright" if bright else "dark"),
                                img, P, exp))
    centres = [(24 + 12 * (k % 6), 25 + 12 * (k // 6)) for k in range(16)]
    c = min(max(ini, mn) + 10, 255)
    for n in (8, 9):
        for bright in (True, False):
            b = _base(c, bright)
            img = flat(b)
            for s, (cx, cy) in enumerate(centres):
                arc(img, cx, cy, s, n, b + c if bright else b - c)

            def exp(r, n=n, c=c):
                got = cand(r)
                if n == 9:  # every start position, the arcs that wrap 15 -> 0 included
                    assert all(got.get(p) == [c - 1] for p in centres), [got.get(p) for p in centres]
                else:
                    assert not any(p in got for p in centres)
            out.append(Case("%sarc%d_%s" % (pre, n, "bright" if bright else "dark"), img, P, exp))
    for bright in (True, False):  # ring 0..4 and 8..12: two adjacent cardinals pass the pretest, longest arc is 5
        b = _base(c, bright)
        img = flat(b)
        arc(img, 40, 40, 0, 5, b + c if bright else b - c)
        arc(img, 40, 40, 8, 5, b + c if bright else b - c)

        def exp(r):
            assert (40, 40) not in cand(r)
            st = cell(r, 0, 0)
            assert st["ini"]["pretest"] >= 1 or st["min"]["pretest"] >= 1
        out.append(Case("%spretest_only_%s" % (pre, "bright" if bright else "dark"), img, P, exp))
    for centre, ring in ((0, 255), (255, 0)):  # S = 255, response 254
        img = arc(flat(centre), 40, 40, 0, 16, ring)

        def exp(r):
            assert cand(r).get((40, 40)) == [254]
        out.append(Case("%scentre%d_ring%d" % (pre, centre, ring), img, P, exp))
    return out


# ------------------------------------------------------------------------------ fallback and NMS ---
P1 = (500, 1.2, 1, 20, 7)


def fallback_cases():
    out = []
    out.append(Case("fallback/weak_only", dots(flat(), [(30, 30, 110), (45, 40, 110)]), P1,
                    lambda r: (_exactly({(30, 30): 9, (45, 40): 9})(r),
                               _eq(cell(r, 0, 0)["threshold"], 7), _eq(cell(r, 0, 0)["ini"]["corners"], 0))))
    out.append(Case("fallback/weak_beside_ini", dots(flat(), [(30, 30, 110), (45, 40, 110), (50, 25, 130),
                                                              (80, 30, 110)]), P1,
                    lambda r: (_exactly({(50, 25): 29, (80, 30): 9})(r), _eq(cell(r, 0, 0)["threshold"], 20),
                               _eq(cell(r, 0, 1)["threshold"], 7))))

    def exp(r):  # the ini pass finds two corners that suppress each other: empty, so the min pass runs (:812)
        st = cell(r, 0, 0)
        assert st["ini"]["corners"] == 2 and st["ini"]["survivors"] == 0 and st["threshold"] == 7
        assert st["min"]["corners"] == 3 and st["min"]["survivors"] == 1
        _exactly({(45, 40): 9})(r)
    out.append(Case("fallback/ini_all_tied", dots(flat(), [(30, 30, 130), (31, 30, 130), (45, 40, 110)]), P1, exp))
    return out


def _eq(a, b):
    assert a == b, (a, b)


def nms_cases():
    out = []
    for name, d in (("h", (1, 0)), ("v", (0, 1)), ("d", (1, 1)), ("anti", (-1, 1))):
        def exp(r):
            assert cell(r, 0, 0)["ini"]["corners"] == 2 and not cand(r) and len(r.kps) == 0
        out.append(Case("nms/equal_" + name, dots(flat(), [(40, 40, 150), (40 + d[0], 40 + d[1], 150)]), P1, exp))
    out.append(Case("nms/differ_by_1", dots(flat(), [(40, 40, 150), (41, 40, 151), (30, 30, 151), (30, 31, 150)]), P1,
                    _exactly({(41, 40): 50, (30, 30): 50})))
    out.append(Case("nms/plateau3", dots(flat(), [(40, 40, 150), (41, 40, 150), (42, 40, 150)]), P1,
                    lambda r: (_eq(cell(r, 0, 0)["ini"]["corners"], 3), _exactly({})(r))))
    # equal pairs with a cell's band boundary between them: each cell's score map is zero outside its band
    out.append(Case("nms/equal_across_columns",
                    dots(flat(), [(62, 30, 150), (63, 30, 150), (62, 70, 150), (63, 71, 150)]), P1,
                    _exactly({(62, 30): 49, (63, 30): 49, (62, 70): 49, (63, 71): 49})))
    out.append(Case("nms/equal_across_rows", dots(flat(), [(30, 52, 150), (30, 53, 150), (80, 52, 150), (81, 53, 150)]),
                    P1, _exactly({(30, 52): 49, (30, 53): 49, (80, 52): 49, (81, 53): 49})))
    out.append(Case("nms/equal_across_cell_corner", dots(flat(), [(62, 52, 150), (63, 53, 150)]), P1,
                    _exactly({(62, 52): 49, (63, 53): 49})))
    pts = [(19, 25), (62, 35), (63, 45), (100, 30), (30, 19), (40, 52), (50, 53), (70, 80), (19, 19), (100, 80),
           (62, 60), (75, 52)]
    out.append(Case("nms/first_last_band_row_col", dots(flat(), [(x, y, 150) for x, y in pts]), P1,
                    _exactly({p: 49 for p in pts})))
    return out


# --------------------------------------------------------------------------------- cell geometry ---
def geometry_cases():
    out = []
    out.append(Case("geo/edges_detectable", dots(flat(), [(19, 40, 150), (100, 45, 150), (40, 19, 150), (50, 80, 150)]),
                    P1, _exactly({(19, 40): 49, (100, 45): 49, (40, 19): 49, (50, 80): 49})))
    out.append(Case("geo/edges_one_outside",
                    dots(flat(), [(18, 40, 150), (101, 45, 150), (40, 18, 150), (50, 81, 150)]), P1,
                    lambda r: (_exactly({})(r), _eq(len(r.kps), 0))))

    def exp(r):
        st = cell(r, 1, 1)
        assert st["clamped_x"] and st["clamped_y"] and st["rect"] == (60, 50, 104, 84)
        _exactly({(95, 75): 49, (100, 80): 39})(r)
    out.append(Case("geo/clamped_last_cell", dots(flat(), [(95, 75, 150), (100, 80, 140)]), P1, exp))
    return out


SWEEP_PARAMS = (40, 1.2, 1, 20, 7)


def sweep_sizes():
    """one level, W = 62..140, three heights each: the smallest, the square and a portrait one that still has
    round((W-32)/(H-32)) >= 1"""
    return [(w, h) for w in range(62, 141) for h in sorted({62, w, w + 17})]


def sweep_image(w, h):
    img = noise(w, h, w * 1000 + h, 92, 108)
    pts = [(19, 19, 160), (w - 20, h - 20, 165), (w - 20, 19, 170), (19, h - 20, 175), (w // 2, h // 2, 180),
           (w - 26, h // 2 + 3, 30)]
    return dots(img, pts)


def zero_capacity_case():
    """a cell row 4..6 px high (band height 0, no key slot) needs 26 cell rows: the smallest level height is 813,
    and round((W-32)/781) >= 1 needs W >= 423. The last row starts at y = 16 + 25 * 31 = 791, maxBorderY = 797."""
    w, h = 423, 813
    img = noise(w, h, 5, 96, 104)
    pts = [(19 + 37 * k, 19 + 70 * k, 160) for k in range(11)] + [(200, 789, 160), (210, 793, 160), (100, 788, 150)]
    dots(img, pts)

    def exp(r):
        lv = r.stats["levels"][0]
        assert lv["nRows"] == 26 and lv["hCell"] == 31
        st = cell(r, 25, 0)
        assert st["rect"][1] == 791 and st["rect"][3] == 797 and st["clamped_y"]
        assert st["ini"]["corners"] == 0 and st["min"]["corners"] == 0  # 6 rows: cv::FAST scores none
        assert (200, 789) in cand(r) and (210, 793) in cand(r)  # both through row 24, which detects up to y = 793
    return Case("geo/zero_capacity_row", img, (300, 1.2, 1, 20, 7), exp)


def one_band_cases():
    """cells whose detection band is one row or one column: 7 px high or wide. Geometry::build gives such a cell a
    key capacity of ceil(1 / 2) = 1; rounded down it would be 0 and the corner the reference emits would be lost.
    423 x 814: 26 cell rows of 31, the last one y in [791, 798), and row 24 detects up to y = 793 only, so the dot at
    y = 794 is found through the 7-row cell alone. 814 x 62 is the same in x (and has 26 octree roots)."""
    out = []
    w, h = 423, 814
    img = dots(noise(w, h, 8, 96, 104), [(19 + 37 * k, 19 + 70 * k, 160) for k in range(11)] +
               [(200, 794, 160), (300, 794, 150), (100, 793, 170)])

    def expr(r):
        lv = r.stats["levels"][0]
        assert lv["nRows"] == 26
        for j, x in ((5, 200), (9, 300)):
            st = cell(r, 25, j)
            assert st["rect"][1] == 791 and st["rect"][3] == 798 and st["clamped_y"]
            assert st["ini"]["survivors"] == 1 and len(cand(r)[(x, 794)]) == 1
        assert len(cand(r)[(100, 793)]) == 1  # through row 24
    out.append(Case("geo/one_band_row", img, (300, 1.2, 1, 20, 7), expr))
    w, h = 814, 62
    img = dots(noise(w, h, 9, 96, 104), [(19 + 31 * k, 19 + (7 * k) % 24, 160 + k) for k in range(25)] +
               [(794, 25, 150), (794, 38, 170), (793, 31, 140)])

    def expc(r):
        lv = r.stats["levels"][0]
        st = cell(r, 0, 25)
        assert lv["nCols"] == 26 and lv["nIni"] == 26 and st["rect"] == (791, 16, 798, 46) and st["clamped_x"]
        assert st["ini"]["survivors"] == 2 and len(cand(r)[(794, 25)]) == 1 and len(cand(r)[(794, 38)]) == 1
        assert len(cand(r)[(793, 31)]) == 1  # through column 24
    out.append(Case("geo/one_band_column", img, (40, 1.2, 1, 20, 7), expc))
    return out


def dropped_cell_cases():
    """the skips of :794 and :803. A last cell column starting at or past maxBorderX - 6 needs 26 columns (width 781
    after the borders, W = 813: the column would start at x = 791 = maxBorderX - 6); a last row starting at or past
    maxBorderY - 3 needs 29 rows (H = 903). The cell before is clamped and covers the same pixels, so nothing is lost.
    No level of 140 px or less has such a cell. The wide image also has 26 octree roots."""
    out = []
    w, h = 813, 62
    img = dots(noise(w, h, 6, 96, 104), [(19 + 31 * k, 19 + (7 * k) % 24, 160 + k) for k in range(26)] +
               [(790, 25, 150), (793, 40, 170)])

    def expc(r):
        lv = r.stats["levels"][0]
        assert lv["nCols"] == 26 and lv["nIni"] == 26 and cell(r, 0, 25)["skipped"] == "col"
        assert cell(r, 0, 24)["rect"] == (760, 16, 797, 46) and (793, 40) in cand(r)
    out.append(Case("geo/dropped_last_column", img, (40, 1.2, 1, 20, 7), expc))
    w, h = 468, 903
    img = dots(noise(w, h, 7, 96, 104), [(19 + 40 * k, 19 + 78 * k, 160 + k) for k in range(11)] +
               [(100, 880, 150), (200, 883, 170)])

    def expr(r):
        lv = r.stats["levels"][0]
        rows = [c for c in lv["cells"] if c["i"] == 28]
        assert lv["nRows"] == 29 and len(rows) == 1 and rows[0]["skipped"] == "row"
        assert cell(r, 27, 0)["rect"][3] == 887 and (200, 883) in cand(r)
    out.append(Case("geo/dropped_last_row", img, (300, 1.2, 1, 20, 7), expr))
    return out


# ------------------------------------------------------------- dense cells, octree storage, launches ---
P2 = (500, 1.2, 2, 20, 7)  # nfeat 273 / 227: node_cap 276 on level 0 only, so a >= 64-frame batch splits the octree


def dense_cases():
    out = []

    def exp(r):
        st = cell(r, 0, 0)["ini"]
        assert st["pretest"] > 64 and st["corners"] > 64 and st["survivors"] > 64
        lv = r.stats["levels"]
        assert lv[0]["N"] + 3 > 256 >= lv[1]["N"] + 3
    out.append(Case("dense/lattice4", lattice(flat(), 4, 4, 150), P2, exp))

    def exp2(r):
        st = cell(r, 0, 0)["ini"]
        assert st["pretest"] > 64 and st["survivors"] > 20
    out.append(Case("dense/noise", noise(W0, H0, 11), P2, exp2))
    out.append(Case("dense/flat", flat(), P2, lambda r: _eq(len(r.kps), 0)))
    return out


def octree_cases():
    out = []
    PN = (12, 1.2, 1, 20, 7)
    grid = [(24 + 9 * (k % 9), 24 + 9 * (k // 9)) for k in range(54)]  # 9-px spacing: isolated dots

    def ndots(n):
        return dots(flat(), [(x, y, 130 + (37 * k) % 90) for k, (x, y) in enumerate(grid[:n])])
    for n, name in ((5, "n_below_N"), (12, "n_equals_N"), (13, "n_is_N_plus_1"), (54, "n_far_above_N")):
        def exp(r, n=n):
            lv = r.stats["levels"][0]
            assert lv["candidates"] == n and lv["N"] == 12
            assert lv["octree_out"] == (n if n <= 12 else lv["octree_out"]) and (n <= 12 or lv["octree_out"] >= 12)
            if n == 54:
                assert lv["stop_at_n"]
        out.append(Case("octree/" + name, ndots(n), PN, exp))
    # N = 1: the root holds 5 keys and is divided once (:596-640 divides before it looks at N); two children are
    # occupied, so two keypoints come out
    out.append(Case("octree/N_is_1", ndots(5), (1, 1.2, 1, 20, 7),
                    lambda r: (_eq(r.stats["levels"][0]["N"], 1), _eq(r.stats["levels"][0]["divisions"], 1),
                               _eq(len(r.kps), 2))))

    def exp_tie(r):  # equal responses in one node: the first key in the node's order stays (strict > at :748-757)
        lv = r.stats["levels"][0]
        assert lv["nodes_with_tied_best"] == 2 and lv["octree_out"] == 3 and lv["candidates"] == 7
        # of the four equal keys of the upper-left node the first in cell order stays, of the two lower-right ones too
        assert [(int(x), int(y)) for x, y, _ in r.stages[0]["octree"]] == [(90, 70), (90, 30), (30, 30)]
    out.append(Case("octree/equal_responses", dots(flat(), [(30, 30, 150), (38, 30, 150), (30, 38, 150), (38, 38, 150),
                                                            (90, 70, 150), (95, 75, 150), (90, 30, 140)]),
                    (3, 1.2, 1, 20, 7), exp_tie))

    def exp_split(r):  # the root is 88 x 68: its children split at x = 44, y = 34 (level x = 60, y = 50)
        c = cand(r)
        assert {(60, 50), (60, 30), (30, 50), (59, 45)} <= set(c)
        assert r.stats["levels"][0]["divisions"] == 1
        # `<` at :515-524: x = 44 goes right, y = 34 goes down, so (60, 50) is in the lower-right child (where it beats
        # (80, 70)), (60, 30) alone upper-right, (30, 50) alone lower-left, and (59, 45) loses to (25, 25) upper-left;
        # children are pushed to the front, so the output runs n4, n3, n2, n1
        assert [(int(x), int(y)) for x, y, _ in r.stages[0]["octree"]] == [(60, 50), (30, 50), (60, 30), (25, 25)]
    out.append(Case("octree/keys_on_split", dots(flat(), [(60, 50, 156), (60, 30, 151), (30, 50, 152), (59, 45, 153),
                                                          (80, 70, 150), (25, 25, 155)]), (4, 1.2, 1, 20, 7),
                    exp_split))
    return out


def nini_cases():
    """(W-32)/(H-32) of exactly 1.5 and 2.5 (:543 rounds half away from zero: 2 and 3 roots), and 3.4"""
    out = []
    for w, h, n in ((77, 62, 2), (107, 62, 3), (134, 62, 3)):
        xs = list(range(19, w - 19, 7)) + [w - 20]
        hx = (w - 32) / n
        edge = sorted({16 + int(hx * i) for i in range(1, n)} | {16 + int(hx * i) - 1 for i in range(1, n)})
        pts = [(x, 19 + (5 * k) % 22, 130 + (29 * k) % 100) for k, x in enumerate(xs)]
        pts += [(x, 42, 150 + k) for k, x in enumerate(edge)
                if all(abs(x - p[0]) > 1 or abs(42 - p[1]) > 1 for p in pts)]

        def exp(r, n=n, edge=edge):
            lv = r.stats["levels"][0]
            assert lv["nIni"] == n and lv["candidates"] >= 8
            assert any(x in edge for x, _ in cand(r))  # keys on a root's boundary column
        out.append(Case("octree/nIni%d_%dx%d" % (n, w, h), dots(flat(100, w, h), pts), (8, 1.2, 1, 20, 7), exp))
    return out


def scratch_case():
    """more level-0 candidates than the LDS key limit, so the octree's global-scratch instantiation runs: 126 features
    on one level is the smallest count with 256-entry node tables (KL 1888, the smallest limit); dots every 2 px in
    x and 4 px in y are the densest lattice whose dots have no other dot on their ring"""
    w = h = 162
    img = lattice(flat(100, w, h), 2, 4, 150)

    def exp(r):
        lv = r.stats["levels"][0]
        assert key_limit(lv["N"], lv["nIni"]) == KL_256 and lv["candidates"] > KL_256, lv["candidates"]
    return Case("octree/global_scratch", img, (126, 1.2, 1, 20, 7), exp)


def empty_level_case():
    """a level with no candidates between levels that have some: a single-pixel dot of contrast 9 is a corner on level
    0 only (min threshold); the two equal pixels of a 1 x 2 bar suppress each other on level 0, are resampled below
    the min threshold on level 1 and to one corner on level 2"""
    img = dots(flat(), [(40, 40, 109), (72, 58, 115), (72, 59, 115)])

    def exp(r):
        assert [v["candidates"] for v in r.stats["levels"]] == [1, 0, 1]
        assert sorted(set(r.kps["octave"])) == [0, 2]
    return Case("octree/empty_middle_level", img, (500, 1.2, 3, 20, 7), exp)


# ------------------------------------------------------------------ orientation and descriptor ---
def _blur_outside(k):
    """the blur's taps for this keypoint's descriptor reads leave the level: REFLECT_101 engaged"""
    return (k["blur_x"][0] < 0 or k["blur_y"][0] < 0 or k["blur_x"][1] >= k["width"] or k["blur_y"][1] >= k["height"])


def orientation_cases():
    out = []
    for name, (dx, dy), ang in (("0", (5, 0), 0.0), ("90", (0, 5), 90.0), ("180", (-5, 0), 180.0),
                                ("270", (0, -5), 270.0)):
        img = dots(flat(), [(60, 45, 150), (60 + dx, 45 + dy, 103)])

        def exp(r, ang=ang):
            assert kp_of(r, 60, 45)["angle"] == ang
        out.append(Case("orient/angle_" + name, img, P2, exp))

    def exp0(r):
        k = kstat(r, 60, 45)
        assert k["m01"] == 0 and k["m10"] == 0 and kp_of(r, 60, 45)["angle"] == 0.0
        assert k["equal_pairs"] > 64  # the blurred patch is flat away from the dot
    out.append(Case("orient/symmetric_patch", dots(flat(), [(60, 45, 150)]), P2, exp0))
    for v, d in ((0, 255), (255, 0)):
        def exps(r):
            assert kstat(r, 60, 45)["equal_pairs"] > 64
        out.append(Case("orient/saturated_%d" % v, dots(flat(v), [(60, 45, d), (64, 47, d)]), P2, exps))
    # the four extreme positions of level 0, a weak pixel in each of 8 directions setting the angle
    for k, (dx, dy) in enumerate(((5, 0), (4, 4), (0, 5), (-4, 4), (-5, 0), (-4, -4), (0, -5), (4, -4))):
        pts = []
        for x, y in ((19, 19), (100, 19), (19, 80), (100, 80)):
            pts += [(x, y, 150), (x + dx, y + dy, 104)]

        def expx(r, diagonal=k % 2 == 1):
            for x, y in ((19, 19), (100, 19), (19, 80), (100, 80)):
                assert _blur_outside(kstat(r, x, y)) == diagonal  # +-13 px at 0 / 90 degrees, 18 px at 45
        out.append(Case("orient/extremes_dir%d" % k, textured_frame(dots(flat(), pts), 40 + k), P2, expx))
    # the same on level 1 (100 x 83): dots that the resize puts on its extreme positions (19 | 80, 19 | 63)
    pts = []
    for x, sx in ((23, 1), (96, -1)):
        for y, sy in ((23, 1), (76, -1)):
            pts += [(x, y, 255), (x + 5 * sx, y + 5 * sy, 112)]

    def expl1(r):
        for x, y in ((19, 19), (80, 19), (19, 63), (80, 63)):
            assert _blur_outside(kstat(r, x, y, 1))
    out.append(Case("orient/extremes_level1", textured_frame(dots(flat(), pts), 50), P2, expl1))
    return out


def tail_cases():
    """level widths with w mod 4 = 1, 2, 3 and a keypoint on the last detectable column whose pattern, rotated by 45
    degrees steps, reads up to column w - 2 (the pattern reaches 18 px at most): GaussianBlur's scalar tail columns
    [w & ~3, w) are read for w mod 4 = 2 and 3; for w mod 4 = 1 the tail is column w - 1, which no descriptor reads"""
    out = []
    for w in (121, 122, 123):
        pts = []
        for k, (dx, dy) in enumerate(((5, 0), (4, 4), (0, 5), (-4, 4), (-5, 0), (-4, -4), (0, -5), (4, -4))):
            x, y = w - 20, 21 + 8 * k
            pts += [(x, y, 150), (x + dx, y + dy, 104)]

        def exp(r, w=w):
            ks = [k for k in r.stats["keypoints"] if k["level"] == 0 and k["x"] == w - 20]
            assert len(ks) == 8
            reach = max(k["read_x"][1] for k in ks)
            assert reach == w - 2
            assert (reach >= (w & ~3)) == (w % 4 != 1)
        out.append(Case("blur/tail_w%d" % w, dots(flat(100, w, H0), pts), (500, 1.2, 1, 20, 7), exp))
    return out


def tail_rounding_case():
    """GaussianBlur's scalar tail rounds half up where its vector part rounds half to even: they differ only where the
    7 x 7 sum is exactly k + 1/2 with k even. Here the sum at (120, 49), a tail column of the 122-px level, is
    102.5 * 2^16, and comparison 99 of the keypoint at (102, 50) reads 102 against that pixel: 103 (half up) sets
    the bit, 102 would not. The two extra pixels are outside the keypoint's FAST ring and IC_Angle patch."""
    img = dots(flat(101, 122, H0), [(102, 50, 151), (106, 54, 105), (118, 46, 9), (120, 49, 122)])

    def exp(r):
        K = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)
        pad = np.pad(r.stages[0]["pyramid"].astype(np.int64), 3, mode="reflect")
        rows = sum(K[i] * pad[:, i:i + 122] for i in range(7))
        assert int(sum(K[i] * rows[i:i + H0, :] for i in range(7))[49, 120]) == 205 * 32768
        k = kstat(r, 102, 50)
        assert k["read_x"][1] >= 120 and (r.desc[r.stats["keypoints"].index(k)][99 // 8] >> (99 % 8)) & 1
    return Case("blur/tail_half_up", img, (500, 1.2, 1, 20, 7), exp)


# ----------------------------------------------------------------------------------- pyramid ---
def pyramid_cases():
    out = []
    img = dots(noise(W0, H0, 21, 60, 140), [(30, 30, 250), (90, 70, 5)])

    def exp_copy(r):  # scale_x = 1: the last column's second tap is past the row (xmax < dw: the right-edge clamp)
        assert r.stats["levels"][1]["size"] == (W0, H0) and resize_fits(W0, H0, W0, H0) == (W0 - 1, True, True)
        assert np.array_equal(r.stages[1]["pyramid"], r.stages[0]["pyramid"])
    out.append(Case("pyramid/right_edge_clamp", img, (500, 1.004, 2, 20, 7), exp_copy))
    # 1.6: a 32-row output tile needs more than 48 source rows (resize_tile_fits fails; at 1.5 it still fits);
    # 2.5: four outputs span more than an 8-byte source window (build_pyr_tables fails as well)
    out.append(Case("pyramid/scale_1_6", img, (500, 1.6, 2, 20, 7),
                    lambda r: (_eq(r.stats["levels"][1]["size"], (75, 62)),
                               _eq(resize_fits(W0, H0, 75, 62), (75, False, True)))))
    big = dots(noise(160, 160, 22, 60, 140), [(30, 30, 250), (120, 110, 5)])
    out.append(Case("pyramid/scale_2_5", big, (500, 2.5, 2, 20, 7),
                    lambda r: (_eq(r.stats["levels"][1]["size"], (64, 64)),
                               _eq(resize_fits(160, 160, 64, 64), (64, False, False)))))
    # eight levels: 222 px is the smallest side whose level 7 is 62 px
    img8 = dots(noise(222, 222, 23, 80, 120),
                [(40 + 17 * k, 30 + 19 * ((3 * k) % 9), 250 if k % 2 else 0) for k in range(9)])
    for y, x in ((60, 150), (150, 60), (111, 111)):
        img8[y:y + 9, x:x + 9] = 230

    def exp8(r):
        lv = r.stats["levels"]
        assert len(lv) == 8 and lv[7]["size"] == (62, 62) and all(v["candidates"] > 0 for v in lv)
        for a, b in zip(lv, lv[1:]):  # the common scale: every level takes the tiled and the whole-frame kernels
            assert resize_fits(*a["size"], *b["size"]) == (b["size"][0], True, True)
    out.append(Case("pyramid/eight_levels", img8, (300, 1.2, 8, 20, 7), exp8))
    return out


def all_cases():
    out = []
    for ini, mn in FAST_PARAMS:
        out += fast_cases(ini, mn)
    out += fallback_cases() + nms_cases() + geometry_cases() + dense_cases() + octree_cases() + nini_cases()
    out += [scratch_case(), empty_level_case(), zero_capacity_case()] + one_band_cases() + dropped_cell_cases()
    out += orientation_cases() + tail_cases() + [tail_rounding_case()] + pyramid_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def groups(cases):
    """{(W, H, params): [cases]} in first-seen order"""
    g = {}
    for c in cases:
        g.setdefault((c.image.shape[1], c.image.shape[0]) + tuple(c.params), []).append(c)
    return g


FAST_GROUP_PREFIXES = ("fast_", "fallback/", "nms/")  # the groups run with the oracle's vector and scalar FAST

# rejected inputs (product only; the oracle is not called on them): (W, H, params)
REJECTED = [
    ("level_under_62", 61, 80, (100, 1.2, 1, 20, 7)),
    ("level1_under_62", 73, 100, (100, 1.2, 2, 20, 7)),       # 73 / 1.2 = 60.8: level 1 is 61 px wide
    ("zero_roots_62x93", 62, 93, (100, 1.2, 1, 20, 7)),       # round(30 / 61) == 0 initial nodes
    ("scale_exactly_2", 160, 160, (100, 2.0, 2, 20, 7)),      # OpenCV switches to INTER_AREA
]

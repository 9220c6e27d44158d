"""Deterministic stereo pairs for the Frame::ComputeStereoMatches parity tests (Frame.cc:470-641).

Pure numpy and integer arithmetic (float32 only where the reference itself multiplies floats), so every
machine builds the same bytes.

* band_scene: a textured pair whose disparity differs per row band (zero, whole and fractional pixels),
  with independent noise and occluded blocks in the right image: non-zero SADs, a real median, sub-pixel
  fits, end-of-range and negative-disparity rejections.
* directed_cases: flat grey images with hand-placed 11x11 patches and hand-made keypoints and descriptors,
  one named left keypoint per edge of the algorithm. Every input is valid (octaves in [0, nlevels),
  coordinates inside the image): the point is wrong answers, never out-of-range indices.
* throw_cases: the two inputs on which the reference would throw (a left window outside its level).
"""
import numpy as np

f32 = np.float32
NLEVELS, SCALE_FACTOR = 8, 1.2
KP_FIELDS = [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")]
kp_dtype = np.dtype(KP_FIELDS)

# band disparities in 1/16 px: 3 5/16, 9 8/16, 0 and 17 13/16 px
BANDS = (53, 152, 0, 285)
BANDS_ALT = (0, 40, 200, 119)  # a second right image for the same left one
# (W, seed, bands) at H = 240 and 500 features: the seeds whose scenes meet the coverage conditions that
# test_oracle_frame.py asserts on the CPU restatement (376 wide: dword rows; 375: the byte-wise kernel)
BAND_CASES = [(376, 2, BANDS), (376, 2, BANDS_ALT), (376, 4, BANDS), (375, 3, BANDS), (375, 3, BANDS_ALT),
              (375, 6, BANDS)]
BAND_SHARED_SEED = {376: 2, 375: 3}  # the seed whose left image comes with both right images

# directed cases: maxD = mbf / mb = 40 px, so both ends of the disparity range fit in a small image
MBF, MB = 4.0, 0.1
MAXD = 40
ZONE = 168  # directed images: rows below are flat grey + patches, rows from here on are textured (pyramid levels)
ZONE_DX = 6  # disparity of the textured zone


def tables(W, H):
    """mvScaleFactor, mvInvScaleFactor (ORBextractor.cc:417-431) and the level sizes (ComputePyramid)."""
    scale = [f32(1)]
    for _ in range(1, NLEVELS):
        scale.append(f32(scale[-1] * f32(SCALE_FACTOR)))
    inv = [f32(f32(1) / s) for s in scale]
    sizes = [(int(np.rint(f32(f32(W) * i))), int(np.rint(f32(f32(H) * i)))) for i in inv]
    return np.array(scale, f32), np.array(inv, f32), sizes


def _texture(rng, W, H, cell=24, rect_area=700):
    """smooth bilinear background (integer lerp of a coarse random grid), random rectangles, +-3 noise"""
    gw, gh = W // cell + 2, H // cell + 2
    g = rng.integers(40, 216, (gh, gw)).astype(np.int64)
    y, x = np.arange(H), np.arange(W)
    y0, fy, x0, fx = y // cell, (y % cell)[:, None], x // cell, (x % cell)[None, :]
    top = g[y0][:, x0] * (cell - fx) + g[y0][:, x0 + 1] * fx
    bot = g[y0 + 1][:, x0] * (cell - fx) + g[y0 + 1][:, x0 + 1] * fx
    img = (top * (cell - fy) + bot * fy + cell * cell // 2) // (cell * cell)
    for _ in range(W * H // rect_area):
        w, h = int(rng.integers(4, 29)), int(rng.integers(4, 29))
        rx, ry = int(rng.integers(0, W)), int(rng.integers(0, H))
        img[ry:ry + h, rx:rx + w] = int(rng.integers(0, 256))
    img = img + rng.integers(-3, 4, (H, W))
    return np.clip(img, 0, 255)


def band_scene(seed, W, H, bands=BANDS, noise=4, occlusions=12):
    """(left, right) uint8 [H, W]. The left image is a crop of a texture that depends on (seed, W, H) only; the
    right image is right[y, x] = tex[y, x + d] with d = bands[band of y] / 16 px (4-bit fixed-point lerp), plus
    independent +-noise per pixel and `occlusions` 48x48 blocks of another texture."""
    assert 0 <= min(bands) and max(bands) < 16 * 30
    tex = _texture(np.random.default_rng([seed, 0]), W + 32, H)
    left = tex[:, :W]
    right = np.empty((H, W), np.int64)
    bh = H // len(bands)
    for b, d in enumerate(bands):
        r0, r1 = b * bh, (H if b == len(bands) - 1 else (b + 1) * bh)
        i, f = d >> 4, d & 15
        right[r0:r1] = (tex[r0:r1, i:i + W] * (16 - f) + tex[r0:r1, i + 1:i + 1 + W] * f + 8) >> 4
    rng = np.random.default_rng([seed, 1] + [int(b) for b in bands])
    right = np.clip(right + rng.integers(-noise, noise + 1, (H, W)), 0, 255)
    other = _texture(np.random.default_rng([seed, 2]), W, H)
    for _ in range(occlusions):
        ox, oy = int(rng.integers(0, W - 48)), int(rng.integers(0, H - 48))
        right[oy:oy + 48, ox:ox + 48] = other[oy:oy + 48, ox:ox + 48]
    return left.astype(np.uint8), right.astype(np.uint8)


# ------------------------------------------------------------------------------------------ directed cases
PASSES = ("right_edge", "end_shift", "deltaR_range", "neg_disp", "maxD", "kept", "median_rej")  # got past Hamming
MISSES = ("no_cand", "hamming")


class _Directed:
    def __init__(self, W, H):
        assert W >= 320 and H == 240
        self.W, self.H = W, H
        self.rng = np.random.default_rng(470641)
        self.L = np.full((H, W), 128, np.int64)
        self.R = np.full((H, W), 128, np.int64)
        zone = _texture(self.rng, W + ZONE_DX, H - ZONE, cell=16, rect_area=500)
        self.L[ZONE:] = zone[:, :W]
        self.R[ZONE:] = zone[:, ZONE_DX:]
        self.scale, self.inv, self.sizes = tables(W, H)
        self.kl, self.dl, self.kr, self.dr, self.names, self.expect = [], [], [], [], [], {}
        self.slots = iter([(40 + 32 * i, 5 + 16 * j) for j in range(8) for i in range(8)])
        self.wide = iter([(70 + 70 * i, 133 + 16 * j) for j in range(2) for i in range(4)])

    # ---- primitives
    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def flip(self, d, h):
        """d with exactly h bits flipped: Hamming distance h"""
        d = d.copy()
        for p in self.rng.permutation(256)[:h]:
            d[p >> 3] ^= np.uint8(1 << (p & 7))
        return d

    def patch(self, symmetric=False):
        p = self.rng.integers(40, 200, (11, 11)).astype(np.int64)
        if symmetric:
            p[:, 6:] = p[:, :5][:, ::-1]
        return p

    @staticmethod
    def perturbed(p, sad):
        """p with `sad` grey levels added over its non-centre pixels: the L1 distance of the two centred windows"""
        idx = [i for i in range(121) if i != 60]
        base, rem = divmod(sad, 120)
        q = p.copy().reshape(-1)
        for n, i in enumerate(idx):
            q[i] += base + (1 if n < rem else 0)
        return q.reshape(11, 11)

    def put(self, img, x, y, p):
        img[y - 5:y + 6, x - 5:x + 6] = p

    def kp(self, x, y, octave):
        assert 0 <= x <= self.W - 1 and 0 <= y <= self.H - 1 and 0 <= octave < NLEVELS
        return (f32(x), f32(y), f32(31.0) * self.scale[octave], f32(0), f32(1), octave)

    def left(self, name, x, y, octave, d, expect):
        assert name not in self.expect
        self.kl.append(self.kp(x, y, octave))
        self.dl.append(d)
        self.names.append(name)
        self.expect[name] = (expect,) if isinstance(expect, str) else tuple(expect)

    def right(self, x, y, octave, d):
        self.kr.append(self.kp(x, y, octave))
        self.dr.append(d)

    def level_xy(self, su, sv, lev):
        """level-0 float32 coordinates that Frame.cc:563-565 rounds to (su, sv) at level lev"""
        out = []
        for s in (su, sv):
            for e in (0.0, 0.25, -0.25, 0.5, -0.5):
                v = f32(f32(s) * self.scale[lev] + f32(e))
                t = f32(v * self.inv[lev])
                if np.floor(t + f32(0.5)) == s and abs(float(t) - s) < 0.4:
                    break
            else:
                raise AssertionError("no level-0 coordinate for %d at level %d" % (s, lev))
            out.append(v)
        return out

    # ---- one level-0 case: the left patch at xL, its copy (+ sad grey levels) at xL - d in the right image, the
    # right keypoint k px off the copy (the best shift is 5 - k)
    def good(self, name, xL, y, d=6, k=0, sad=10, h=20, expect="kept", symmetric=False, roct=0):
        p = self.patch(symmetric)
        self.put(self.L, xL, y, p)
        self.put(self.R, xL - d, y, self.perturbed(p, sad))
        D = self.desc()
        self.left(name, xL, y, 0, D, expect)
        self.right(xL - d + k, y, roct, self.flip(D, h))

    def build(self):
        W, H = self.W, self.H
        slot, wide = lambda: next(self.slots), lambda: next(self.wide)
        # the 0.01 branch (Frame.cc:625-629): a mirror-symmetric patch at zero disparity, d1 == d3, deltaR == 0
        x0, y = slot()
        self.good("branch001", x0 + 5, y, d=0, sad=0, symmetric=True)
        # every (c0l & 3, c0r & 3) pair, the best shift moving with it; SAD 10 each (the median's population)
        for a in range(4):
            for b in range(4):
                x0, y = slot()
                k = (a + 2 * b) % 7 - 3
                xL = x0 + (a + 5 - x0) % 4
                d = 4 + (xL + k - 10 - 4 - b) % 4
                assert (xL - 5) & 3 == a and (xL - d + k - 10) & 3 == b
                self.good("align_%d_%d" % (a, b), xL, y, d=d, k=k)
        # the largest L1 distance there is: white with a black centre against black with a white centre, 120 * 510
        x0, y = slot()
        p = np.full((11, 11), 255, np.int64)
        p[5, 5] = 0
        self.put(self.L, x0, y, p)
        xr = x0 - 6
        self.R[y - 5:y + 6, xr - 10:xr + 1] = 0
        self.R[y, xr - 5] = 255
        D = self.desc()
        self.left("sad_max", x0, y, 0, D, "median_rej")
        self.right(xr, y, 0, self.flip(D, 20))
        # SAD tie between shifts 3, 5, 7, 9 (columns of period 2): the first one wins
        x0, y = slot()
        ca, cb = self.rng.integers(40, 110, 11), self.rng.integers(140, 200, 11)
        xr = x0 - 4
        for j in range(11):
            self.L[y - 5:y + 6, x0 - 5 + j] = ca if j % 2 == 0 else cb
        for c in range(3, 21):
            self.R[y - 5:y + 6, xr - 10 + c] = ca if (c - 3) % 2 == 0 else cb
        D = self.desc()
        self.left("sad_tie_first", x0, y, 0, D, "kept")
        self.right(xr, y, 0, self.flip(D, 20))
        # best shift next to an end (neighbours at 0 and 10), and at an end (rejected)
        for name, k, e in (("shift_1", 4, "kept"), ("shift_9", -4, "kept"), ("shift_0", 5, "end_shift"),
                           ("shift_10", -5, "end_shift")):
            x0, y = slot()
            self.good(name, x0, y, k=k, expect=e)
        # thOrbDist = 75 (Frame.cc:475, 553)
        x0, y = slot()
        self.good("hamming_74", x0, y, h=74)
        x0, y = slot()
        self.good("hamming_75", x0, y, h=75, expect="hamming")
        # the octave filter (Frame.cc:537)
        x0, y = slot()
        self.good("roct_plus1", x0, y, roct=1)
        x0, y = slot()
        self.good("roct_plus2", x0, y, roct=2, expect="hamming")
        # the copy one pixel to the right of the left patch: disparity -1
        x0, y = slot()
        self.good("neg_disp", x0, y, d=-1, k=-1, expect="neg_disp")
        # the median's population: 1.5f * 1.4f * 10 rounds to 21 in float and the test is `<`, so 21 is rejected and 20 kept
        x0, y = slot()
        self.good("sad_20", x0, y, sad=20)
        x0, y = slot()
        self.good("sad_21", x0, y, sad=21, expect="median_rej")
        for s in (255, 256, 511, 512):  # both sides of the radix select's bin boundaries, with duplicates
            for c in "abc":
                x0, y = slot()
                self.good("sad_%d_%s" % (s, c), x0, y, sad=s, expect="median_rej")
        for s in (536, 1074):  # between 1.5f * 1.4f * 255 and * 256, and between * 511 and * 512
            x0, y = slot()
            self.good("sad_%d" % s, x0, y, sad=s, expect="median_rej")
        for c in "abc":
            x0, y = slot()
            self.good("zero_%s" % c, x0, y, sad=0)
        # the columns next to the left and right borders (a dword past the level's last one is clamped)
        self.good("left_col_edge", 15, 37, d=5)
        self.good("border_right", W - 6, 53)
        D = self.desc()
        self.left("right_edge", W - 8, 69, 0, D, "right_edge")  # endu = uR0 + 11 >= cols
        self.right(W - 11, 69, 0, self.flip(D, 20))
        self.left("no_cand", 100, 160, 0, self.desc(), "no_cand")  # no right keypoint's band holds row 160
        # limits of the search: uR == minU and uR == maxU are inside, disparity == maxD is not
        x0, y = wide()
        self.good("uR_eq_minU", x0, y, d=MAXD - 1, k=-1)
        x0, y = wide()
        self.good("disp_gt_maxD", x0, y, d=MAXD + 1, k=1, expect="maxD")
        x0, y = wide()
        self.good("disp_eq_maxD", x0, y, d=MAXD, sad=0, symmetric=True, expect="maxD")
        x0, y = wide()
        self.good("uR_below_minU", x0, y, d=MAXD + 1, expect="hamming")
        x0, y = wide()
        self.good("uR_eq_maxU", x0, y, d=2, k=2)
        x0, y = wide()
        self.good("uR_above_maxU", x0, y, d=2, k=3, expect="hamming")
        # Hamming tie: two copies of the patch, 4 and 28 px to the left, at distance 20 both. The reference keeps
        # the lower iR (the first it meets); the other copy sits in an earlier row bucket
        x0, y = wide()
        p, D = self.patch(), self.desc()
        self.put(self.L, x0, y, p)
        self.put(self.R, x0 - 4, y, self.perturbed(p, 10))
        self.put(self.R, x0 - 28, y, self.perturbed(p, 10))
        self.left("hamming_tie", x0, y, 0, D, "kept")
        self.right(x0 - 4, y + 1, 0, self.flip(D, 20))
        self.right(x0 - 28, y - 1, 0, self.flip(D, 20))
        # the same behind 70 worse candidates in earlier buckets of the band (a second trip of 64 candidates)
        x0, y = wide()
        p, D = self.patch(), self.desc()
        self.put(self.L, x0, y, p)
        self.put(self.R, x0 - 4, y, self.perturbed(p, 10))
        self.put(self.R, x0 - 28, y, self.perturbed(p, 10))
        self.left("many_cands", x0, y, 0, D, "kept")
        for i in range(35):
            self.right(x0 - (i % MAXD), y - 2, 0, self.flip(D, 21 + i))
        self.right(x0 - 4, y + 2, 0, self.flip(D, 20))
        self.right(x0 - 28, y + 2, 0, self.flip(D, 20))
        for i in range(35, 70):
            self.right(x0 - (i % MAXD), y - 2, 0, self.flip(D, 21 + i))
        # rows 5 (every case of the first row of slots) and H - 6, the latter inside the textured zone
        D = self.desc()
        self.left("row_last", 100, H - 6, 0, D, "kept")
        self.right(100 - ZONE_DX, H - 6, 0, self.flip(D, 20))
        # octave 1 in the textured zone: inside, at the level's bottom right corner, at its right-edge `continue`
        lw1, lh1 = self.sizes[1]
        for name, su, sv, sur, e in (("o1_inside", 120, 160, 115, PASSES), ("o1_corner", lw1 - 6, lh1 - 6, lw1 - 12, PASSES),
                                     ("o1_right_edge", lw1 - 6, lh1 - 26, lw1 - 11, "right_edge")):
            D = self.desc()
            x, y = self.level_xy(su, sv, 1)
            xr, _ = self.level_xy(sur, sv, 1)
            self.left(name, x, y, 1, D, e)
            self.right(xr, y, 1, self.flip(D, 10))
        # one octave-7 right keypoint; left keypoints of octaves 6 and 7 on the first and last row of its band and
        # one row outside either end, and an octave-5 one that the octave filter drops
        D = self.desc()
        xr, yr = self.level_xy(40, 55, 7)
        self.right(xr, yr, 7, D)
        r = f32(f32(2.0) * self.scale[7])
        minr, maxr = int(np.floor(f32(yr - r))), int(np.ceil(f32(yr + r)))
        for lev, su in ((7, 42), (6, 50)):
            x, _ = self.level_xy(su, 10, lev)
            for name, v, e in (("above_band", minr - 1, MISSES), ("v_eq_minr", minr, PASSES), ("v_eq_maxr", maxr, PASSES),
                               ("below_band", maxr + 1, MISSES)):
                self.left("o%d_%s" % (lev, name), x, f32(v + 0.5), lev, self.flip(D, 10), e)
        x, _ = self.level_xy(60, 10, 5)
        self.left("o5_filtered", x, f32(minr + 3.5), 5, self.flip(D, 10), MISSES)
        return self


_cache = {}


def directed_cases(W, H):
    """dict: left, right (uint8 [H, W]), kl, dl, kr, dr (orbx_kp records and [n, 32] descriptors), mbf, mb, names (one
    per left keypoint) and expect (name -> the exits of Frame.cc:508-650 the case may end in)."""
    if (W, H) not in _cache:
        b = _Directed(W, H).build()
        assert b.L.min() >= 0 and b.L.max() <= 255 and b.R.min() >= 0 and b.R.max() <= 255
        _cache[(W, H)] = dict(left=b.L.astype(np.uint8), right=b.R.astype(np.uint8), kl=np.array(b.kl, kp_dtype),
                              dl=np.array(b.dl, np.uint8), kr=np.array(b.kr, kp_dtype), dr=np.array(b.dr, np.uint8),
                              mbf=MBF, mb=MB, names=list(b.names), expect=dict(b.expect))
    return _cache[(W, H)]


# subsets of the directed left keypoints (same images, same right keypoints): the median pass sees other populations
MEDIAN_SUBSETS = {
    # name: (left keypoint names, median, kept)
    "all_zero": (["branch001", "zero_a", "zero_b", "zero_c"], 0, 0),  # threshold 0: nothing is < 0
    "single_zero": (["zero_b"], 0, 0),
    "single": (["align_2_1"], 10, 1),
    # the n/2-th element on either side of a bin boundary of the radix select (255 | 256 and 511 | 512), duplicates
    # around it, n odd and even; sad_536 / sad_1074 lie between the two thresholds, so a median one off changes `kept`
    "odd_255": (["zero_a", "sad_536"] + ["sad_255_" + c for c in "abc"] + ["sad_256_" + c for c in "ab"], 255, 6),
    "even_256": (["zero_a", "sad_536"] + ["sad_255_" + c for c in "abc"] + ["sad_256_" + c for c in "abc"], 256, 8),
    "odd_511": (["align_0_0", "sad_1074"] + ["sad_511_" + c for c in "abc"] + ["sad_512_" + c for c in "ab"], 511, 6),
    "even_512": (["align_0_0", "sad_1074"] + ["sad_511_" + c for c in "abc"] + ["sad_512_" + c for c in "abc"], 512, 8),
    # sorted (0, 10, 255, 256): element n/2 = 2 keeps all four, element (n - 1)/2 would reject two
    "even_split": (["sad_256_b", "zero_c", "sad_255_b", "align_3_3"], 255, 4),
    "edge_21": (["align_1_1", "align_1_2", "align_3_0", "sad_20", "sad_21", "hamming_75", "no_cand"], 10, 4),
    "dup_at_median": (["zero_a", "sad_512_a"] + ["align_%d_%d" % (a, b) for a in range(4) for b in range(4)], 10, 17),
}


def subset(case, names):
    idx = np.array([case["names"].index(n) for n in names])
    return case["kl"][idx].copy(), case["dl"][idx].copy()


def throw_cases(W, H):
    """[(name, kl, dl, kr, dr)] on the directed images. The left keypoint's own window leaves level 0 on the right
    (cv::Mat::colRange asserts, Frame.cc:574); in `both` its best right keypoint also fails the iniu / endu test of
    Frame.cc:586, which the reference only reaches after the assert."""
    c = directed_cases(W, H)
    b = _Directed(W, H)
    D = b.desc()
    out = []
    for name, xr in (("left_window_only", W - 30), ("both", W - 5)):
        kl = np.array([b.kp(W - 3, 101, 0)], kp_dtype)
        kr = np.array([b.kp(xr, 101, 0)], kp_dtype)
        out.append((name, np.concatenate([c["kl"][:3], kl]), np.concatenate([c["dl"][:3], D[None]]),
                    np.concatenate([c["kr"][:3], kr]), np.concatenate([c["dr"][:3], b.flip(D, 20)[None]])))
    return out

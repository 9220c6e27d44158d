"""Independent numpy restatements of the OpenCV 3.x primitives vs the oracle (no GPU).

These check the oracle's literal C translation against definitions written from the
published algorithm in a different form (vectorised numpy, pure-Python loops for the
quadtree), so an error has to be made twice to slip through."""
import math

import numpy as np
import pytest

import oracle_py
import orbamd
from extract_py import distribute_octtree_py, fast_numpy, gauss_numpy, resize_numpy


@pytest.mark.parametrize("seed,t", [(0, 20), (1, 7), (2, 40), (3, 0)])
def test_fast_matches_definition(seed, t):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (40, 43), dtype=np.uint8)
    img[10:20, 5:30] = 200  # flat region + edges
    got = oracle_py.fast(img, t)
    exp = fast_numpy(img, t)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("t", [0, 7, 20, 60, 255])
def test_fast_vector_form_equals_scalar(t):
    """the oracle's AVX2 FAST step (32 pixels, OpenCV FAST_t's vector form) equals its scalar form: noise,
    flat areas, saturated pixels (v + t > 255, v - t < 0) and every row-tail width; and the whole extractor"""
    rng = np.random.default_rng(100 + t)
    imgs = [rng.integers(0, 256, (48, w), dtype=np.uint8) for w in (7, 35, 36, 37, 67, 68, 100)]
    sat = rng.integers(0, 256, (40, 90), dtype=np.uint8)
    sat[5:30, 10:80] = np.where(rng.random((25, 70)) < 0.5, 0, 255).astype(np.uint8)
    imgs.append(sat)
    try:
        for img in imgs:
            oracle_py.set_fast_simd(True)
            a = oracle_py.fast(img, t)
            oracle_py.set_fast_simd(False)
            b = oracle_py.fast(img, t)
            assert np.array_equal(a, b), img.shape
        if t == 20:
            orc = oracle_py.OracleExtractor(1000, 1.2, 8, 20, 7)
            for img in orbamd.synth_frames(1, 0, 2, 640, 480):
                oracle_py.set_fast_simd(True)
                ka, da = orc(img)
                oracle_py.set_fast_simd(False)
                kb, db = orc(img)
                assert np.array_equal(ka.view(np.uint8), kb.view(np.uint8)) and np.array_equal(da, db)
    finally:
        oracle_py.set_fast_simd(True)


def test_fast_pretest_lerp_exact():
    """k_fast_cells2's byte-SWAR pretest compares with v_lerp_u8 (per byte (a + b + r) >> 1):
    bright = bit 7 of lerp(lerp(c, 255 - v, r_b), 255 - M_b, 1) must equal c > v + t, and
    notdark = bit 7 of lerp(lerp(c, 255 - v, r_d), 255 - M_d, 1) must equal NOT c < v - t, for every
    (c, v, t) in [0, 255]^3 (t = 255: the bright bound is clamped, so only c > v + t => bright)."""
    c = np.arange(256, dtype=np.int32)[:, None]
    v = np.arange(256, dtype=np.int32)[None, :]

    def lerp(a, b, r):
        return (a + b + r) >> 1

    for t in range(256):
        rb, rd = t & 1, 1 - (t & 1)
        mb_c = min((t + 256 + rb) >> 1, 255)
        md_c = (256 - t - (t & 1)) >> 1
        bright = (lerp(lerp(c, 255 - v, rb), 255 - mb_c, 1) & 0x80) != 0
        notdark = (lerp(lerp(c, 255 - v, rd), 255 - md_c, 1) & 0x80) != 0
        assert lerp(lerp(c, 255 - v, rb), 255 - mb_c, 1).max() <= 255
        if t < 255:
            assert np.array_equal(bright, c > v + t), t
        else:
            assert not (c > v + t).any() or bright[c > v + t].all()
        assert np.array_equal(notdark, ~(c < v - t)), t


def test_fast_on_synthetic_cell_roi():
    frame = orbamd.synth_frames(0, 0, 1, 640, 480)[0]
    roi = frame[100:138, 200:237]
    for t in (20, 7):
        assert np.array_equal(oracle_py.fast(roi, t), fast_numpy(roi, t))


@pytest.mark.parametrize("sw,sh,dw,dh", [(640, 480, 533, 400), (533, 400, 444, 333), (257, 193, 214, 161),
                                         (1241, 376, 1034, 313), (214, 161, 179, 134)])
def test_resize_matches_definition(sw, sh, dw, dh):
    rng = np.random.default_rng(sw)
    src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    assert np.array_equal(oracle_py.resize_linear(src, dw, dh), resize_numpy(src, dw, dh))


@pytest.mark.parametrize("w,h", [(640, 480), (179, 134), (309, 231), (67, 70)])
def test_gauss_matches_definition(w, h):
    rng = np.random.default_rng(w * h)
    src = rng.integers(0, 256, (h, w), dtype=np.uint8)
    src[:20, :20] = 255  # saturation path
    assert np.array_equal(oracle_py.gauss7(src), gauss_numpy(src))


def test_fast_atan2_close_to_atan2():
    rng = np.random.default_rng(5)
    for y, x in rng.integers(-20000, 20000, (500, 2)):
        a = oracle_py.fast_atan2(float(y), float(x))
        e = math.degrees(math.atan2(y, x)) % 360
        assert abs((a - e + 180) % 360 - 180) < 0.3
    assert oracle_py.fast_atan2(0.0, 0.0) == 0.0


def test_descriptor_distance():
    rng = np.random.default_rng(9)
    for _ in range(200):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = rng.integers(0, 256, 32, dtype=np.uint8)
        assert oracle_py.descriptor_distance(a, b) == int(np.unpackbits(a ^ b).sum())


# ---------------------------------------------------------------- DistributeOctTree ---
@pytest.mark.parametrize("agent,t", [(0, 0), (3, 11)])
def test_octree_matches_python_restatement(agent, t):
    frame = orbamd.synth_frames(agent, t, 1, 640, 480)[0]
    orc = oracle_py.OracleExtractor()
    orc(frame)
    nfeat = orc.tables()["nfeat"]
    for l in (0, 3, 7):
        w, h = orc.level_size(l)
        cand = [tuple(r) for r in orc.candidates(l)]
        exp = distribute_octtree_py(cand, 16, w - 16, 16, h - 16, int(nfeat[l]))
        got = orc.octree(l)
        exp = np.array([(x + 16, y + 16, r) for x, y, r in exp], np.float32)
        assert np.array_equal(got, exp), "level %d" % l

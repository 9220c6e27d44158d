"""ORBextractor restated in plain Python / numpy from the reference text (no GPU, no oracle code).

Line numbers are those of ORB_SLAM2/src/ORBextractor.cc. The OpenCV primitives (FAST, resize, GaussianBlur) are written
from their definitions in another form than the oracle's C (vectorised numpy, Python lists for the quadtree), so an
error has to be made twice to slip through. `extract_py` returns the result of operator() and a `stats` structure that
says which branches the input reached; tests/test_oracle_extract.py asserts every directed case's exit from it.

Only cos/sin of the keypoint angle (computeOrbDescriptor, :113) and fastAtan2 (:103) come from elsewhere: the float
cosine is the double one rounded to float, fastAtan2 is oracle_py.fast_atan2 (pinned by its own test)."""
import math
import os
import re

import numpy as np

import oracle_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PATCH_SIZE, HALF_PATCH_SIZE, EDGE_THRESHOLD = 31, 15, 19  # :72-74

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
        (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

f32 = np.float32


def cv_round(v):
    """cvRound: round half to even (cvtss2si / cvtsd2si under the default rounding mode)"""
    return int(np.rint(v))


# ---------------------------------------------------------------------------------- cv::FAST ---
def fast_cell(img, t):
    """cv::FAST(img, kps, t, nonmax=true) from the definition: 9 contiguous of 16 ring pixels all > p+t or all < p-t;
    score = cornerScore<16>; 3x3 strict NMS against a score map that is zero outside the image's 3-px inset;
    row-major order. Returns ((n, 3) float32 of x, y, score; counts) with counts = pixels with two adjacent
    cardinal ring pixels both brighter or both darker (necessary for a 9-arc), corners before NMS, survivors."""
    img = img.astype(np.int32)
    h, w = img.shape
    sc = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return np.zeros((0, 3), np.float32), {"pretest": 0, "corners": 0, "survivors": 0}
    ys, xs = np.mgrid[3:h - 3, 3:w - 3]
    p = img[3:h - 3, 3:w - 3]
    d = np.stack([p - img[ys + dy, xs + dx] for dx, dy in RING], -1)  # v - ring
    best_dark = np.full(p.shape, -10**9)
    best_bright = np.full(p.shape, -10**9)
    for k in range(16):
        idx = [(k + j) % 16 for j in range(9)]
        best_dark = np.maximum(best_dark, d[..., idx].min(-1))
        best_bright = np.maximum(best_bright, (-d[..., idx]).min(-1))
    corner = (best_dark > t) | (best_bright > t)
    score = np.maximum(np.maximum(best_dark, best_bright), t) - 1
    sc[3:h - 3, 3:w - 3] = np.where(corner, score, 0)
    pre = np.zeros(p.shape, bool)
    for k in (0, 4, 8, 12):
        a, b = d[..., k], d[..., (k + 4) % 16]
        pre |= ((a > t) & (b > t)) | ((a < -t) & (b < -t))
    keep = sc > 0
    pad = np.pad(sc, 1)  # the 3-px inset is zero already, the pad is never the maximum
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            if a or b:
                keep &= sc > pad[1 + a:1 + a + h, 1 + b:1 + b + w]
    yy, xx = np.nonzero(keep)  # row-major
    out = np.stack([xx, yy, sc[yy, xx]], -1).astype(np.float32).reshape(-1, 3)
    return out, {"pretest": int(pre.sum()), "corners": int(corner.sum()), "survivors": len(out)}


def fast_numpy(img, t):
    return fast_cell(img, t)[0]


# -------------------------------------------------------------------------------- cv::resize ---
def resize_numpy(src, dw, dh):
    """INTER_LINEAR 8U fixed point (OpenCV 3.x resizeGeneric_, SSE2 vertical span)."""
    sh, sw = src.shape
    scale_x = 1.0 / (dw / sw)
    scale_y = 1.0 / (dh / sh)
    S = src.astype(np.int64)

    def coef(n, scale, limit, clamp_frac):
        f = np.array([np.float32((i + 0.5) * scale - 0.5) for i in range(n)], np.float32)
        si = np.floor(f).astype(np.int64)
        fr = (f - si.astype(np.float32)).astype(np.float32)
        if clamp_frac:
            neg = si < 0
            fr[neg] = 0
            si[neg] = 0
            hi = si >= limit - 1
            fr[hi] = 0
            si[hi] = limit - 1
        a0 = np.rint((np.float32(1) - fr) * np.float32(2048)).astype(np.int64)
        a1 = np.rint(fr * np.float32(2048)).astype(np.int64)
        return si, a0, a1

    sx, a0, a1 = coef(dw, scale_x, sw, True)
    sy, b0, b1 = coef(dh, scale_y, sh, False)
    r0 = np.clip(sy, 0, sh - 1)
    r1 = np.clip(sy + 1, 0, sh - 1)
    sx1 = np.minimum(sx + 1, sw - 1)
    h0 = S[r0][:, sx] * a0 + S[r0][:, sx1] * a1
    h1 = S[r1][:, sx] * a0 + S[r1][:, sx1] * a1
    simd_end = 0
    while simd_end <= dw - 16:
        simd_end += 16
    while simd_end < dw - 4:
        simd_end += 4
    B0, B1 = b0[:, None], b1[:, None]
    v_simd = (((h0 >> 4) * B0) >> 16) + (((h1 >> 4) * B1) >> 16) + 2 >> 2
    v_scal = (h0 * B0 + h1 * B1 + (1 << 21)) >> 22
    v = np.where(np.arange(dw)[None, :] < simd_end, v_simd, v_scal)
    return np.clip(v, 0, 255).astype(np.uint8)


# -------------------------------------------------------------------------- cv::GaussianBlur ---
def gauss_numpy(src):
    k = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)
    h, w = src.shape
    pad = np.pad(src.astype(np.int64), 3, mode="reflect")  # numpy "reflect" == REFLECT_101
    rows = sum(k[i] * pad[:, i:i + w] for i in range(7))
    s = sum(k[i] * rows[i:i + h, :] for i in range(7))
    rhe = (s + 0x7FFF + ((s >> 16) & 1)) >> 16
    half_up = (s + (1 << 15)) >> 16
    v = np.where(np.arange(w)[None, :] < (w & ~3), rhe, half_up)
    return np.clip(v, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------- DistributeOctTree ---
def distribute_octtree_py(keys, minX, maxX, minY, maxY, N, stats=None):
    """Pure-Python literal restatement of ORBextractor.cc:539-763 (std::list semantics,
    pointer tie-break pinned to creation order). stats (a dict, optional) receives nIni, the number of DivideNode
    calls, the node count after the first pass and whether the stop-at-N pass (:664-733) ran."""
    seq = [0]
    ndiv = [0]

    class Node:
        def __init__(self, ul, ur, bl, br, ks):
            self.UL, self.UR, self.BL, self.BR, self.k = ul, ur, bl, br, ks
            self.nomore = False
            self.seq = None

    def divide(n):
        ndiv[0] += 1
        hx = math.ceil((n.UR[0] - n.UL[0]) / 2)
        hy = math.ceil((n.BR[1] - n.UL[1]) / 2)
        n1 = Node(n.UL, (n.UL[0] + hx, n.UL[1]), (n.UL[0], n.UL[1] + hy), (n.UL[0] + hx, n.UL[1] + hy), [])
        n2 = Node(n1.UR, n.UR, n1.BR, (n.UR[0], n.UL[1] + hy), [])
        n3 = Node(n1.BL, n1.BR, n.BL, (n1.BR[0], n.BL[1]), [])
        n4 = Node(n3.UR, n2.BR, n3.BR, n.BR, [])
        for kp in n.k:
            if kp[0] < n1.UR[0]:
                (n1 if kp[1] < n1.BR[1] else n3).k.append(kp)
            elif kp[1] < n1.BR[1]:
                n2.k.append(kp)
            else:
                n4.k.append(kp)
        for c in (n1, n2, n3, n4):
            c.nomore = len(c.k) == 1
        return n1, n2, n3, n4

    def create(n):
        n.seq = seq[0]
        seq[0] += 1
        return n

    # :543 round(float): half away from zero (a 1.5 or 2.5 aspect ratio gives 2 or 3 roots)
    nIni = int(math.floor(np.float32(maxX - minX) / np.float32(maxY - minY) + np.float32(0.5)))
    hX = np.float32(maxX - minX) / np.float32(nIni)
    lst = []
    for i in range(nIni):
        ulx = int(np.float32(hX * np.float32(i)))
        urx = int(np.float32(hX * np.float32(i + 1)))
        lst.append(create(Node((ulx, 0), (urx, 0), (ulx, maxY - minY), (urx, maxY - minY), [])))
    roots = list(lst)
    for kp in keys:
        roots[int(np.float32(kp[0]) / hX)].k.append(kp)
    lst = [n for n in lst if len(n.k) > 0]
    for n in lst:
        n.nomore = len(n.k) == 1
    finish = False
    phase2 = False
    vsz = []
    while not finish:
        prev = len(lst)
        vsz = []
        nexp = 0
        i = 0
        while i < len(lst):
            n = lst[i]
            if n.nomore:
                i += 1
                continue
            front = []
            for c in divide(n):
                if c.k:
                    create(c)
                    front.insert(0, c)
                    if len(c.k) > 1:
                        nexp += 1
                        vsz.append(c)
            del lst[i]
            lst[:0] = front
            i += len(front)
        if len(lst) >= N or len(lst) == prev:
            finish = True
        elif len(lst) + nexp * 3 > N:
            phase2 = True
            while not finish:
                prev = len(lst)
                vprev = sorted(vsz, key=lambda n: (len(n.k), n.seq))
                vsz = []
                for n in reversed(vprev):
                    front = []
                    for c in divide(n):
                        if c.k:
                            create(c)
                            front.insert(0, c)
                            if len(c.k) > 1:
                                vsz.append(c)
                    lst.remove(n)
                    lst[:0] = front
                    if len(lst) >= N:
                        break
                if len(lst) >= N or len(lst) == prev:
                    finish = True
    out = []
    ties = 0
    for n in lst:
        best = n.k[0]
        for kp in n.k[1:]:
            if kp[2] > best[2]:
                best = kp
        ties += sum(1 for kp in n.k if kp[2] == best[2]) > 1
        out.append(best)
    if stats is not None:
        stats.update(nIni=nIni, divisions=ndiv[0], stop_at_n=phase2, nodes_with_tied_best=int(ties),
                     roots_used=sum(1 for r in roots if r.k))
    return out


# -------------------------------------------------------------------------- the pattern table ---
def _decode_header(path, name):
    txt = open(path).read()
    body = txt[txt.index(name):]
    body = body[body.index("{") + 1: body.index("}")]
    vals = [int(v, 16) for v in re.findall(r"0x[0-9a-f]{2}", body)]
    return np.array(vals, np.uint8).astype(np.int8)


_pattern = None


def pattern():
    """bit_pattern_31_ (:150-408) as (256, 4) int: x0, y0, x1, y1 of each comparison (the table whose hash
    tests/test_oracle_tables.py pins against the reference text)"""
    global _pattern
    if _pattern is None:
        _pattern = _decode_header(os.path.join(ROOT, "oracle", "orb_pattern_data.h"),
                                  "orb_oracle_pattern_u8").astype(np.int32).reshape(256, 4)
    return _pattern


# -------------------------------------------------------------------- constructor (:410-470) ---
def constructor_tables(nfeatures, scaleFactor, nlevels):
    sf = float(f32(scaleFactor))  # the float argument stored in a double member (ORBextractor.h:100)
    scale = [f32(1)]
    sigma2 = [f32(1)]
    for _ in range(1, nlevels):
        scale.append(f32(float(scale[-1]) * sf))  # :421
        sigma2.append(f32(scale[-1] * scale[-1]))
    inv_scale = [f32(1) / s for s in scale]
    inv_sigma2 = [f32(1) / s for s in sigma2]
    factor = f32(1.0 / sf)  # :436
    ndes = f32(f32(f32(nfeatures) * f32(f32(1) - factor)) / f32(f32(1) - f32(math.pow(float(factor), float(nlevels)))))
    nfeat, total = [], 0
    for _ in range(nlevels - 1):
        nfeat.append(cv_round(ndes))
        total += nfeat[-1]
        ndes = f32(ndes * factor)
    nfeat.append(max(nfeatures - total, 0))
    # :454-469
    r2 = f32(math.sqrt(2.0))
    vmax = int(math.floor(f32(f32(f32(HALF_PATCH_SIZE) * r2) / f32(2)) + f32(1)))
    vmin = int(math.ceil(f32(f32(HALF_PATCH_SIZE) * r2) / f32(2)))
    umax = [0] * (HALF_PATCH_SIZE + 1)
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(HALF_PATCH_SIZE * HALF_PATCH_SIZE - v * v))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return {"scale": np.array(scale, f32), "inv_scale": np.array(inv_scale, f32), "sigma2": np.array(sigma2, f32),
            "inv_sigma2": np.array(inv_sigma2, f32), "nfeat": nfeat, "umax": umax}


def level_sizes(W, H, inv_scale):
    """ComputePyramid's sizes (:1111-1112)"""
    return [(cv_round(f32(W) * s), cv_round(f32(H) * s)) for s in inv_scale]


# -------------------------------------------------------------------------- cell loop (:765-829) ---
def cell_loop(img, ini_th, min_th):
    """one level of ComputeKeyPointsOctTree up to vToDistributeKeys; returns (keys [(x, y, response)], cell stats)"""
    rows, cols = img.shape
    W = f32(30)
    minBX = minBY = EDGE_THRESHOLD - 3
    maxBX, maxBY = cols - EDGE_THRESHOLD + 3, rows - EDGE_THRESHOLD + 3
    width, height = f32(maxBX - minBX), f32(maxBY - minBY)
    nCols, nRows = int(width / W), int(height / W)
    wCell, hCell = int(math.ceil(width / f32(nCols))), int(math.ceil(height / f32(nRows)))
    keys, cells = [], []
    for i in range(nRows):
        iniY = minBY + i * hCell
        maxY = iniY + hCell + 6
        if iniY >= maxBY - 3:
            cells.append({"i": i, "j": None, "skipped": "row"})
            continue
        cy = maxY > maxBY
        if cy:
            maxY = maxBY
        for j in range(nCols):
            iniX = minBX + j * wCell
            maxX = iniX + wCell + 6
            if iniX >= maxBX - 6:
                cells.append({"i": i, "j": j, "skipped": "col"})
                continue
            cx = maxX > maxBX
            if cx:
                maxX = maxBX
            roi = img[iniY:maxY, iniX:maxX]
            k, c_ini = fast_cell(roi, ini_th)
            st = {"i": i, "j": j, "skipped": None, "rect": (iniX, iniY, maxX, maxY), "clamped_x": cx, "clamped_y": cy,
                  "ini": c_ini, "min": None, "threshold": ini_th if len(k) else None}
            if len(k) == 0:  # :812
                k, c_min = fast_cell(roi, min_th)
                st["min"] = c_min
                st["threshold"] = min_th if len(k) else None
            for x, y, r in k:
                keys.append((f32(x + f32(j * wCell)), f32(y + f32(i * hCell)), f32(r)))
            cells.append(st)
    return keys, {"nCols": nCols, "nRows": nRows, "wCell": wCell, "hCell": hCell, "cells": cells}


# --------------------------------------------------------------------- IC_Angle (:77-104) ---
def ic_moments(img, x, y, umax):
    m01 = m10 = 0
    c = img.astype(np.int64)
    for u in range(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1):
        m10 += u * int(c[y, x + u])
    for v in range(1, HALF_PATCH_SIZE + 1):
        d = umax[v]
        plus, minus = c[y + v, x - d:x + d + 1], c[y - v, x - d:x + d + 1]
        m01 += v * int((plus - minus).sum())
        m10 += int((np.arange(-d, d + 1) * (plus + minus)).sum())
    return m01, m10


# ---------------------------------------------------------- computeOrbDescriptor (:107-147) ---
def orb_descriptor(blur, x, y, angle_deg):
    """returns (32 bytes, stats): every product and the sum in float (no contraction), cvRound half to even"""
    factorPI = f32(math.pi / f32(180))  # :107
    angle = f32(f32(angle_deg) * factorPI)
    a, b = f32(math.cos(float(angle))), f32(math.sin(float(angle)))
    P = pattern().astype(f32)
    px = np.concatenate([P[:, 0], P[:, 2]])
    py = np.concatenate([P[:, 1], P[:, 3]])
    ry = np.rint((px * b).astype(f32) + (py * a).astype(f32)).astype(np.int64)
    rx = np.rint((px * a).astype(f32) - (py * b).astype(f32)).astype(np.int64)
    h, w = blur.shape
    yy, xx = y + ry, x + rx
    assert yy.min() >= 0 and xx.min() >= 0 and yy.max() < h and xx.max() < w  # the reference reads unchecked
    val = blur[yy, xx].astype(np.int32)
    t0, t1 = val[:256], val[256:]
    desc = np.packbits((t0 < t1).astype(np.uint8), bitorder="little")
    st = {"read_x": (int(xx.min()), int(xx.max())), "read_y": (int(yy.min()), int(yy.max())),
          # the source pixels of GaussianBlur's 7 taps at those reads: < 0 or >= size means REFLECT_101 engaged
          "blur_x": (int(xx.min()) - 3, int(xx.max()) + 3), "blur_y": (int(yy.min()) - 3, int(yy.max()) + 3),
          "equal_pairs": int((t0 == t1).sum())}
    return desc, st


# ----------------------------------------------------------------- operator() (:1043-1105) ---
KP_DTYPE = oracle_py.kp_dtype


def extract_py(image, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7):
    """Returns (keypoints, descriptors, stages, stats). stages: per level the pyramid image, the candidates
    (vToDistributeKeys) and the octree output with the borders added, as the oracle exposes them."""
    image = np.ascontiguousarray(image, np.uint8)
    H, W = image.shape
    T = constructor_tables(nfeatures, scaleFactor, nlevels)
    sizes = level_sizes(W, H, T["inv_scale"])
    pyr = [image]
    for l in range(1, nlevels):  # :1120 (the 19-px borders are never read)
        pyr.append(resize_numpy(pyr[-1], *sizes[l]))
    minB = EDGE_THRESHOLD - 3
    stages, lstats, per_level = [], [], []
    for l in range(nlevels):
        w, h = sizes[l]
        keys, cs = cell_loop(pyr[l], iniThFAST, minThFAST)
        ost = {}
        kept = distribute_octtree_py(keys, minB, w - minB, minB, h - minB, T["nfeat"][l], ost) if keys else []
        kept = [(f32(x + minB), f32(y + minB), r) for x, y, r in kept]  # :843-844
        per_level.append(kept)
        stages.append({"pyramid": pyr[l], "candidates": np.array(keys, f32).reshape(-1, 3),
                       "octree": np.array(kept, f32).reshape(-1, 3)})
        lstats.append(dict(cs, size=(w, h), N=T["nfeat"][l], candidates=len(keys), octree_in=len(keys),
                           octree_out=len(kept), nIni=ost.get("nIni"), divisions=ost.get("divisions", 0),
                           stop_at_n=ost.get("stop_at_n", False),
                           nodes_with_tied_best=ost.get("nodes_with_tied_best", 0)))
    n = sum(len(k) for k in per_level)
    kps = np.zeros(n, KP_DTYPE)
    desc = np.zeros((n, 32), np.uint8)
    kstats = []
    off = 0
    for l in range(nlevels):
        if not per_level[l]:
            continue  # :1081
        blur = gauss_numpy(pyr[l])  # :1085-1086 (a clone of the level: REFLECT_101 at the level's own edge)
        for x, y, r in per_level[l]:
            xi, yi = cv_round(x), cv_round(y)
            m01, m10 = ic_moments(pyr[l], xi, yi, T["umax"])
            ang = f32(oracle_py.fast_atan2(float(m01), float(m10)))
            d, st = orb_descriptor(blur, xi, yi, ang)
            desc[off] = d
            k = kps[off]
            k["x"], k["y"] = (x, y) if l == 0 else (f32(x * T["scale"][l]), f32(y * T["scale"][l]))  # :1095-1100
            k["size"] = f32(int(f32(PATCH_SIZE) * T["scale"][l]))  # :837
            k["angle"], k["response"], k["octave"] = ang, r, l
            kstats.append(dict(st, level=l, x=xi, y=yi, m01=m01, m10=m10, width=sizes[l][0], height=sizes[l][1]))
            off += 1
    return kps, desc, stages, {"tables": T, "levels": lstats, "keypoints": kstats}

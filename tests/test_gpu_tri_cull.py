"""GPU: the epipolar tile cull of the BF SearchForTriangulation batch calls (k_tri_order + k_tri_mfma over its
layout, csrc/orb_tri_cull.h) against the full scan of the same build (orbm_debug_tri_cull) and against the oracle:
match rows bit for bit, counts, and the rows the call must not touch. At most 8 pairs per launch; the pair lists are
never the identity (test_gpu_match_cases._Batch: q1 = 1, 3, .., q2 = 0, 2, ..).

The tile counters of hook mode 2 say which path ran: a launch past the ordering kernel's capacity leaves them at
zero (the fallback), F = 0 executes no tile at all, and on the C2 fixture the executed share is the CPU test's."""
import ctypes as C
import os

import numpy as np
import pytest

import match_cases as mc
import orbamd
from test_gpu_match_cases import _Batch, _launches, _tri_items

pytestmark = pytest.mark.gpu
f32 = np.float32
CAP = 4096  # kTriOrdCap (orb_tri_cull.h): features per frame the ordering kernel sorts
COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 257, 1007, 2000)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2_640x480_1000.npz")


@pytest.fixture(scope="module")
def mh():
    h = C.c_void_p()
    orbamd._lib.check(orbamd.load().orbm_create(0, C.byref(h)), "orbm_create")
    yield h
    orbamd.load().orbm_destroy(h)


# ------------------------------------------------------------------ geometries
def bench_geometry():
    return mc.default_f12()


def inside_geometry():
    """forward motion: the epipole lies in the image"""
    from orbamd.device import CX, CY, FX, FY
    from orbamd.matcher import compute_f12, epipole
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]], f32)
    R = np.eye(3, dtype=f32)
    t1, t2 = np.zeros(3, f32), np.array([0.004, -0.003, 0.05], f32)
    F12 = compute_f12(R, t1, R, t2, K, K)
    ex, ey = epipole(R, t2, -R.T @ t1, FX, FY, CX, CY)
    assert 0 < ex < 640 and 0 < ey < 480
    return F12, ex, ey


def near_line(F, x1, y1, off, rng):
    """a point at signed distance `off` from the epipolar line of (x1, y1), inside the image where the line crosses it"""
    a, b, c = F.astype(np.float64).T @ np.array([x1, y1, 1.0])
    n = np.hypot(a, b)
    if not n > 0:
        return rng.uniform(0, 640), rng.uniform(0, 480)
    if abs(b) >= abs(a):
        x = rng.uniform(0, 640)
        y = -(a * x + c) / b
    else:
        y = rng.uniform(0, 480)
        x = -(b * y + c) / a
    return x + off * a / n, y + off * b / n


def scene(name, seed, n1, n2, geom, stereo=False, ties=0, one_point=False, yspan=None):
    """n1 queries at random positions; candidate j belongs to query j mod n1: near its epipolar line (inside the band,
    on its edge or outside), its descriptor the query's with 0..70 bits flipped. `ties` queries get three candidates
    of one and the same descriptor at different offsets inside the band (the later original index must win). The
    candidates are added in a shuffled order, so original indices and positions are unrelated."""
    F12, ex, ey = geom
    c = mc.Case(name, seed, F12=F12, epipole=(ex, ey))
    c.stereo_form = stereo
    rng = c.rng
    band = np.sqrt(3.84 * c.sigma2.astype(np.float64))
    qd, qxy = [], []
    for i in range(n1):
        xy = (123.25, 77.5) if one_point else (rng.uniform(5, 635), rng.uniform(5, 475) if yspan is None else
                                               rng.uniform(*yspan))
        qd.append(c.desc())
        qxy.append(xy)
    cands = []
    for j in range(n2):
        o = int(rng.integers(0, len(c.scale)))
        if n1 == 0:
            cands.append((rng.uniform(0, 640), rng.uniform(0, 480), c.desc(), o))
            continue
        i = j % n1
        if one_point:
            x, y = 123.25, 77.5
        else:
            x, y = near_line(F12, qxy[i][0], qxy[i][1], rng.uniform(-1.3, 1.3) * band[o], rng)
        d = c.flip(qd[i], int(rng.integers(10 if i < ties else 0, 70)))
        if i < ties and j < 3 * n1:  # the three candidates of a tie query: one descriptor (D = 6), the widest band
            o = len(c.scale) - 1
            d = c.flip(qd[i], 6) if j < n1 else cands[i][2].copy()
            if not one_point:
                x, y = near_line(F12, qxy[i][0], qxy[i][1], (-0.8, 0.0, 0.8)[j // n1] * band[o], rng)
        cands.append((x, y, d, o))
    for j in rng.permutation(n2):
        x, y, d, o = cands[j]
        c.c(d, x=x, y=y, octave=o, ur=(rng.uniform(0, 30) if rng.random() < 0.6 else -1.0) if stereo else -1.0)
    for i in range(n1):
        c.q("q%d" % i, qd[i], None, None, x=qxy[i][0], y=qxy[i][1],
            ur=(rng.uniform(0, 30) if rng.random() < 0.6 else -1.0) if stereo else -1.0)
    c.tri()
    if stereo:
        c.tri("only", only_stereo=True)
    return c


_scenes = {}


def scenes(kind):
    """built once, shared (the oracle's results are memoised by match_cases.oracle_result)"""
    if kind not in _scenes:
        bench, inside, row = bench_geometry(), inside_geometry(), (mc.F_ROW, *mc.FAR)
        _scenes[kind] = {
            "counts": lambda: [scene("cull_n%d" % n, 1000 + n, n, n, bench) for n in COUNTS],
            "uneven": lambda: [scene("cull_33x1007", 2001, 33, 1007, bench), scene("cull_1007x65", 2002, 1007, 65, bench),
                               scene("cull_300x0", 2003, 300, 0, bench), scene("cull_0x300", 2004, 0, 300, bench)],
            "stereo": lambda: [scene("cull_s%d" % n, 3000 + n, n, n, bench, stereo=True) for n in (33, 257, 1007)]
            + [scene("cull_s_inside", 3500, 600, 600, inside, stereo=True)],
            "inside": lambda: [scene("cull_inside", 4000, 600, 700, inside)],
            # 2000 candidates within 100 rows: a tile spans ~1.6 px, the band of the top octave +-7 px, so the three
            # equal candidates of a tie query lie tiles and chunks apart
            "ties": lambda: [scene("cull_ties", 5000, 600, 2000, row, ties=200, yspan=(50, 150)),
                             scene("cull_ties_bench", 5001, 500, 1800, bench, ties=150)],
            "one_point": lambda: [scene("cull_one_point", 6000, 200, 640, row, ties=60, one_point=True),
                                  scene("cull_one_point_bench", 6001, 200, 260, bench, one_point=True)],
            "f_zero": lambda: [scene("cull_f_zero", 7000, 100, 100, (np.zeros((3, 3), f32), 0.0, 0.0))],
            "fallback": lambda: [scene("cull_over_capacity", 8000, CAP + 1, CAP + 1, bench)],
        }[kind]()
    return _scenes[kind]


# ------------------------------------------------------------------ running both scans
def run_both(torch, mh, items, stereo):
    """every launch (<= 8 pairs) with the full scan (hook 0) and with the cull and its counters (hook 2): both against
    the oracle, and against each other byte for byte (untouched rows included). Returns (matches, tiles executed,
    tiles in all)."""
    lib = orbamd.load()
    total, ex_all, all_all = 0, 0, 0
    try:
        for group in _launches(items):
            for k in range(0, len(group), 8):
                launch = group[k:k + 8]
                cases, calls = [c for c, _ in launch], [kk for _, kk in launch]
                b, c0, k0 = _Batch(torch, cases), cases[0], calls[0]
                F = np.ascontiguousarray(c0.F12.reshape(9))
                head = (mh, len(cases), b.q1.data_ptr(), b.q2.data_ptr(), b.kps.data_ptr(), b.desc.data_ptr(),
                        b.counts.data_ptr())
                geom = (b.S, F.ctypes.data, c0.ex, c0.ey, len(c0.scale), c0.scale.ctypes.data, c0.sigma2.ctypes.data)
                tail = (int(k0["check_ori"]), b.out.data_ptr(), b.nm.data_ptr(), b.stream())
                got = []
                for mode in (0, 2):
                    assert lib.orbm_debug_tri_cull(mh, mode) == 0
                    if stereo:
                        rc = lib.orbm_triangulation_bf_stereo_batch_device(*head, b.ur.data_ptr(), *geom,
                                                                           int(k0["only_stereo"]), *tail)
                    else:
                        rc = lib.orbm_triangulation_bf_batch_device(*head, *geom, *tail)
                    assert rc == 0
                    torch.cuda.synchronize()
                    got.append((b.out.cpu().numpy().copy(), b.nm.cpu().numpy().copy()))
                    total += b.check(calls, untouched=True)  # against the oracle; refills the sentinels
                np.testing.assert_array_equal(got[0][0], got[1][0])
                np.testing.assert_array_equal(got[0][1], got[1][1])
                cnt = (C.c_ulonglong * 2)()
                assert lib.orbm_debug_tri_cull_counts(mh, cnt) == 0
                assert cnt[0] <= cnt[1]
                if b.S > CAP:
                    assert cnt[1] == 0, "a launch past the ordering capacity must take the full scan"
                elif any(c.k1.n and c.k2.n for c in cases):
                    assert cnt[1] > 0, "the cull did not run"
                ex_all, all_all = ex_all + cnt[0], all_all + cnt[1]
    finally:
        lib.orbm_debug_tri_cull(mh, 1)
    return total // 2, ex_all, all_all


def items_of(cases, only=None):
    return [(c, call) for c in cases for call in c.calls if only is None or call["only_stereo"] == only]


@pytest.mark.parametrize("kind", ["counts", "uneven", "inside", "ties", "one_point"])
def test_cull_equals_full_scan_and_oracle(mh, kind):
    torch = pytest.importorskip("torch")
    n, ex, al = run_both(torch, mh, items_of(scenes(kind)), False)
    print("%s: %d matches, tiles executed %d of %d (%.1f %%)" % (kind, n, ex, al, 100.0 * ex / max(al, 1)))
    assert n > 0 and 0 < ex <= al


def test_ties_lie_tiles_and_chunks_apart_and_go_to_the_later_index(mh):
    """the premise of the `ties` scenes, from the oracle's rows: queries whose winner has equals (same distance, all
    passing) at least 64 original indices away, on both sides"""
    c = scenes("ties")[0]
    _, mo = mc.oracle_result(c, c.calls[0])
    d2 = c.k2.descriptors()
    far = 0
    assert c.k2.n >= 3 * c.k1.n
    for i in range(200):  # the tie queries
        j = mo[i]
        assert j >= 0
        same = [k for k in range(c.k2.n) if np.array_equal(d2[k], d2[j])]
        assert len(same) == 3 and j == max(same)
        far += max(same) - min(same) >= 64
    assert far > 100


@pytest.mark.parametrize("only", [False, True])
def test_stereo_form(mh, only):
    torch = pytest.importorskip("torch")
    n, ex, al = run_both(torch, mh, items_of(scenes("stereo"), only), True)
    print("stereo only_stereo=%d: %d matches, tiles executed %d of %d" % (only, n, ex, al))
    assert n > 0 and 0 < ex <= al


def test_f_zero_matches_nothing_and_executes_no_tile(mh):
    torch = pytest.importorskip("torch")
    c = scenes("f_zero")[0]
    assert (mc.oracle_result(c, c.calls[0])[1] == -1).all()
    n, ex, al = run_both(torch, mh, items_of([c]), False)
    assert n == 0 and ex == 0 and al > 0


def test_over_the_sort_capacity_takes_the_full_scan(mh):
    """kp_stride = 4100 > kTriOrdCap: the unculled kernel for that call (run_both asserts the counters stay zero)"""
    torch = pytest.importorskip("torch")
    n, ex, al = run_both(torch, mh, items_of(scenes("fallback")), False)
    assert n > 0 and ex == 0 and al == 0


@pytest.mark.parametrize("stereo", [False, True])
def test_match_cases(mh, stereo):
    """the hand-made cases of match_cases.py that the BF batch calls can express (test_gpu_match_cases' selection)"""
    torch = pytest.importorskip("torch")
    items = _tri_items("abcdh", lambda c, call: c.one_node and c.no_mp and (stereo or (c.mono and not call["only_stereo"])))
    items += _tri_items("e", lambda c, call: c.stereo_form == stereo)
    n, ex, al = run_both(torch, mh, items, stereo)
    print("match_cases stereo=%d: %d pairs, %d matches, tiles executed %d of %d" % (stereo, len(items), n, ex, al))
    assert n > 0 and 0 < ex <= al


def test_c2_fixture_rows_and_tile_share(mh):
    """the committed C2 pair (two consecutive bench frames): the golden match row, and the executed tile share the
    CPU test bounds (tests/test_tri_cull_bound.py: <= 20 % per wave)"""
    torch = pytest.importorskip("torch")
    lib = orbamd.load()
    d = np.load(GOLDEN)
    k1, k0 = d["kps1"], d["kps0"]
    n1, n0 = len(k1), len(k0)
    S = max(n1, n0) + 5
    kps, desc = np.zeros((2, S, 24), np.uint8), np.zeros((2, S, 32), np.uint8)
    kps[0, :n0], kps[1, :n1], desc[0, :n0], desc[1, :n1] = k0, k1, d["desc0"], d["desc1"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    kps_d, desc_d, cnt_d = dev(kps), dev(desc), dev(np.array([n0, n1], np.int32))
    q1, q2 = dev(np.array([1], np.int32)), dev(np.array([0], np.int32))
    out = torch.full((1, S), -7, dtype=torch.int32, device="cuda")
    nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    F = np.ascontiguousarray(d["F12"].reshape(9), f32)
    scale = mc.scale_table()
    sigma2 = (scale * scale).astype(f32)
    try:
        assert lib.orbm_debug_tri_cull(mh, 2) == 0
        assert lib.orbm_triangulation_bf_batch_device(
            mh, 1, q1.data_ptr(), q2.data_ptr(), kps_d.data_ptr(), desc_d.data_ptr(), cnt_d.data_ptr(), S,
            F.ctypes.data, float(d["ex"]), float(d["ey"]), 8, scale.ctypes.data, sigma2.ctypes.data, 0,
            out.data_ptr(), nm.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        cnt = (C.c_ulonglong * 2)()
        assert lib.orbm_debug_tri_cull_counts(mh, cnt) == 0
    finally:
        lib.orbm_debug_tri_cull(mh, 1)
    np.testing.assert_array_equal(out[0, :n1].cpu().numpy(), d["tri_match"])
    assert int(nm.item()) == int(d["tri_n"]) and (out[0, n1:] == -7).all()
    print("C2 fixture: tiles executed %d of %d = %.4f" % (cnt[0], cnt[1], cnt[0] / cnt[1]))
    assert cnt[0] / cnt[1] <= 0.20

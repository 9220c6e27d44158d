"""GPU: new MapPoints from triangulation matches on a device batch. orbm_create_new_map_points_batch_device against
the host unit (orbx_triangulate_matches, itself bit-equal to tests/triangulate_py.py in tests/test_triangulate.py) on
every output as raw bits; the device atan2f and cosParallaxStereo against the host libm; malformed input; and the chain
extract -> undistort -> stereo -> BF triangulation matcher -> new MapPoints -> SearchLocalPoints over the produced
table, against the yardstick's table and the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import orbamd
import triangulate_py as TP
from orbamd.frame import triangulate_matches

pytestmark = pytest.mark.gpu

f32 = np.float32
S = 320  # kp_stride: rows cross the 256-lane chunk and the wave boundary
SENT = 77


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx(torch):
    lib = orbamd.load()
    h = C.c_void_p()
    assert lib.orbm_create(0, C.byref(h)) == 0
    yield h
    lib.orbm_destroy(h)


def stream_of(torch):
    return torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream


def take_error(torch, ctx):
    return orbamd.load().orbm_check_error(ctx, stream_of(torch))


class Batch:
    """6 frames at kp_stride 320 with counts 300, 320, 64, 320, 1, 0 from two pairs of the CPU test's `my` scene
    (lateral/mixed: frames 0, 1; forward/stereo: frames 2, 3, the current keyframe cut to 64; frame 4 = frame 0's first
    keypoint; frame 5 empty), and 8 pairs over them"""

    def __init__(self):
        self.g, pairs = TP.camera_scene("my")
        by = dict((p.name, p) for p in pairs)
        A, B = by["lateral/mixed"], by["forward/stereo"]
        self.A, self.B = A, B
        nf = 6
        self.K = np.zeros((nf, S), TP.KP)
        self.UR = np.full((nf, S), -1, f32)
        self.D = np.full((nf, S), -1, f32)
        self.desc = np.random.default_rng(1).integers(0, 256, (nf, S, 32), dtype=np.uint8)
        self.T = np.stack([A.T1, A.T2, B.T1, B.T2, A.T1, np.eye(4, dtype=f32)]).astype(f32)
        self.cnt = np.array([300, 320, 64, 320, 1, 0], np.int32)
        for f, (k, ur, d) in enumerate(((A.kps1, A.ur1, A.d1), (A.kps2, A.ur2, A.d2), (B.kps1[:64], B.ur1[:64],
                                                                                      B.d1[:64]),
                                        (B.kps2, B.ur2, B.d2), (A.kps1[:1], A.ur1[:1], A.d1[:1]))):
            n = len(k)
            assert n == self.cnt[f]
            self.K[f, :n], self.UR[f, :n], self.D[f, :n] = k, ur, d
        self.desc[0, :300] = A.desc1
        self.desc[2, :64] = B.desc1[:64]
        self.desc[4, :1] = A.desc1[:1]
        last = A.match12.copy()
        last[:256] = -1  # matches only in the row's last chunk
        self.q1 = np.array([0, 2, 4, 5, 0, 0, 0, 2], np.int32)
        self.q2 = np.array([1, 3, 1, 1, 1, 1, 3, 3], np.int32)
        self.M = np.full((8, S), -1, np.int32)
        self.M[0, :300] = A.match12
        self.M[1, :64] = B.match12[:64]
        self.M[2, :1] = A.match12[:1]
        self.M[4, :300] = last
        self.M[6, :300] = A.match12  # frame 0 against frame 3: another pose and other keypoints
        self.M[7, :64] = B.match12[:64]
        self.M[:, 300:] = 5  # past every count: never read

    def host(self, p, K=None, M=None, T=None, monocular=0, med=1.0):
        K = self.K if K is None else K
        M = self.M if M is None else M
        T = self.T if T is None else T
        a, b = int(self.q1[p]), int(self.q2[p])
        n1, n2 = int(self.cnt[a]), int(self.cnt[b])
        return triangulate_matches(self.g.cstruct(), monocular, med, T[a], T[b], K[a, :n1], self.UR[a, :n1],
                                   self.D[a, :n1], self.desc[a, :n1], K[b, :n2], self.UR[b, :n2], self.D[b, :n2],
                                   M[p, :n1])


@pytest.fixture(scope="module")
def batch():
    return Batch()


def launch(torch, ctx, bt, q1=None, q2=None, K=None, M=None, T=None, monocular=0, med=None, stereo=True, nframes=6,
           g=None, cnt=None):
    """one launch over the batch's device arrays; every output pre-filled with a sentinel; numpy arrays back"""
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    q1 = bt.q1 if q1 is None else np.asarray(q1, np.int32)
    q2 = bt.q2 if q2 is None else np.asarray(q2, np.int32)
    K = bt.K if K is None else K
    M = bt.M if M is None else M
    T = bt.T if T is None else T
    P = len(q1)
    t = dict(q1=up(q1), q2=up(q2), K=up(K.view(f32).reshape(K.shape[0], S, 6)), cnt=up(bt.cnt if cnt is None else cnt),
             ur=up(bt.UR), d=up(bt.D), desc=up(bt.desc), T=up(T), M=up(M))
    if med is not None:
        t["med"] = up(np.asarray(med, f32))
    full = lambda sh, dt: torch.full(sh, SENT, dtype=dt, device=dev)  # noqa: E731
    o = dict(status=full((P, S), torch.int8), pos3=full((P, S, 3), torch.float32), pos=full((P * S, 3), torch.float32),
             normal=full((P * S, 3), torch.float32), mind=full((P * S,), torch.float32),
             maxd=full((P * S,), torch.float32), desc=full((P * S, 32), torch.uint8), flags=full((P * S,), torch.uint8),
             feat1=full((P * S,), torch.int32), feat2=full((P * S,), torch.int32), ranges=full((P, 2), torch.int32),
             nnew=full((P,), torch.int32))
    gs = (bt.g if g is None else g).cstruct()
    rc = orbamd.load().orbm_create_new_map_points_batch_device(
        ctx, P, t["q1"].data_ptr(), t["q2"].data_ptr(), nframes, t["K"].data_ptr(), t["cnt"].data_ptr(), S,
        t["ur"].data_ptr() if stereo else None, t["d"].data_ptr() if stereo else None, t["desc"].data_ptr(),
        t["T"].data_ptr(), t["M"].data_ptr(), C.byref(gs), monocular, t["med"].data_ptr() if med is not None else None,
        o["status"].data_ptr(), o["pos3"].data_ptr(), o["pos"].data_ptr(), o["normal"].data_ptr(),
        o["mind"].data_ptr(), o["maxd"].data_ptr(), o["desc"].data_ptr(), o["flags"].data_ptr(),
        o["feat1"].data_ptr(), o["feat2"].data_ptr(), o["ranges"].data_ptr(), o["nnew"].data_ptr(), stream_of(torch))
    assert rc == 0
    torch.cuda.synchronize()
    return dict((k, v.cpu().numpy()) for k, v in o.items())


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same_pair(got, p, n1, ref, what):
    """pair p of a launch against the host unit's result, every output as raw bits; nothing past the count or past
    nnew is written"""
    assert bits(got["status"][p, :n1]) == bits(ref.status), "%s: status %s" % (what, np.flatnonzero(
        got["status"][p, :n1] != ref.status)[:8])
    assert bits(got["pos3"][p, :n1]) == bits(ref.pos3), "%s: pos3" % what
    assert (got["status"][p, n1:] == SENT).all() and (got["pos3"][p, n1:] == SENT).all(), "%s: past the count" % what
    nn = ref.nnew
    assert int(got["nnew"][p]) == nn, "%s: nnew %d, host %d" % (what, int(got["nnew"][p]), nn)
    assert got["ranges"][p].tolist() == [p * S, p * S + nn], what
    sl = slice(p * S, p * S + nn)
    for k, r in (("pos", ref.tab_pos), ("normal", ref.tab_normal), ("mind", ref.tab_min), ("maxd", ref.tab_max),
                 ("desc", ref.tab_desc), ("flags", ref.tab_flags), ("feat1", ref.feat1), ("feat2", ref.feat2)):
        assert bits(got[k][sl]) == bits(r), "%s: table %s" % (what, k)
        assert (got[k][p * S + nn:(p + 1) * S] == SENT).all(), "%s: table %s past nnew" % (what, k)
    return nn


# ------------------------------------------------------------------------------------------------ kernel against host
def test_kernel_equals_host_unit_bitwise(torch, ctx, batch):
    got = launch(torch, ctx, batch)
    assert take_error(torch, ctx) != 0  # the scene's excluded rows raise the flag
    nn = [same_pair(got, p, int(batch.cnt[batch.q1[p]]), batch.host(p), "pair %d" % p) for p in range(8)]
    assert nn[0] > 150 and nn[1] > 30 and nn[3] == 0 and nn[5] == 0 and nn[4] > 10 and nn[6] < nn[0]
    st = got["status"]
    assert (st[4, :256] == TP.NO_MATCH).all() and (st[5, :300] == TP.NO_MATCH).all()
    # table row k is the k-th created idx1
    f1 = got["feat1"][:nn[0]]
    assert np.array_equal(f1, np.flatnonzero(np.isin(st[0, :300], TP.CREATED))) and f1[-1] >= 256
    seen = set(st[0, :300].tolist()) | set(st[1, :64].tolist())
    assert {TP.TRIANGULATED, TP.EXCLUDED, TP.NO_MATCH, TP.REPROJ1, TP.SCALE_RATIO, TP.Z1} <= seen


def test_every_scene_pair_of_one_camera(torch, ctx):
    """every pair of the `tum1` scene, two frames each, in one launch: all fourteen outcomes, both degenerate pairs"""
    g, pairs = TP.camera_scene("tum1")
    pairs = [p for p in pairs if not p.monocular]
    bt = Batch.__new__(Batch)
    nf = 2 * len(pairs)
    bt.g = g
    bt.K, bt.UR, bt.D = np.zeros((nf, S), TP.KP), np.full((nf, S), -1, f32), np.full((nf, S), -1, f32)
    bt.desc = np.zeros((nf, S, 32), np.uint8)
    bt.T = np.zeros((nf, 4, 4), f32)
    bt.cnt = np.zeros(nf, np.int32)
    bt.M = np.full((len(pairs), S), -1, np.int32)
    for i, p in enumerate(pairs):
        for f, k, ur, d, T in ((2 * i, p.kps1, p.ur1, p.d1, p.T1), (2 * i + 1, p.kps2, p.ur2, p.d2, p.T2)):
            n = len(k)
            bt.K[f, :n], bt.T[f], bt.cnt[f] = k, T, n
            if ur is not None:
                bt.UR[f, :n], bt.D[f, :n] = ur, d
        bt.desc[2 * i, :len(p.kps1)] = p.desc1
        bt.M[i, :len(p.kps1)] = p.match12
    bt.q1 = np.arange(0, nf, 2).astype(np.int32)
    bt.q2 = bt.q1 + 1
    got = launch(torch, ctx, bt, nframes=nf)
    take_error(torch, ctx)
    seen = set()
    for i, p in enumerate(pairs):
        same_pair(got, i, len(p.kps1), bt.host(i), p.name)
        seen |= set(got["status"][i, :len(p.kps1)].tolist())
    assert seen == set(range(14))


def test_monocular_baseline_and_pair_order(torch, ctx, batch):
    """monocular launches (no mvuRight arrays, the median-depth baseline test) and a permuted, duplicated pair list:
    the rows of a pair do not depend on where it stands in the list"""
    bt = batch
    mono = Batch()
    mono.UR[:], mono.D[:] = -1, -1
    med = np.array([1.0, 1.0, 1.0, 1.0, 1e3, 1.0, 1.0, 1e-3], f32)  # pair 4 falls below 0.01, pair 7 far above
    got = launch(torch, ctx, mono, monocular=1, med=med, stereo=False)
    take_error(torch, ctx)
    for p in range(8):
        same_pair(got, p, int(mono.cnt[mono.q1[p]]), mono.host(p, monocular=1, med=float(med[p])), "mono pair %d" % p)
    assert (got["status"][4, 256:300] == TP.BASELINE).sum() > 10 and int(got["nnew"][4]) == 0
    clean = launch(torch, ctx, bt)
    order = [7, 0, 3, 0, 6, 1, 2, 5, 4, 0]
    got = launch(torch, ctx, bt, q1=bt.q1[order], q2=bt.q2[order], M=bt.M[order])
    take_error(torch, ctx)
    for j, p in enumerate(order):
        n1 = int(bt.cnt[bt.q1[p]])
        nn = int(clean["nnew"][p])
        assert int(got["nnew"][j]) == nn
        assert bits(got["status"][j]) == bits(clean["status"][p]) and bits(got["pos3"][j]) == bits(clean["pos3"][p])
        for k in ("pos", "normal", "mind", "maxd", "desc", "flags", "feat1", "feat2"):
            assert bits(got[k][j * S:(j + 1) * S]) == bits(clean[k][p * S:(p + 1) * S]), (j, p, k)
        assert got["ranges"][j].tolist() == [j * S, j * S + nn] and n1 <= S


# ------------------------------------------------------------------------------------------------ atan2f, cosf
def test_device_atan2f_and_cos_parallax_equal_host_libm(torch):
    """orbx_selftest_atan2f on 2^20 random first-quadrant pairs over the whole exponent range, 2^18 pairs with
    quotients of ordinary size, and directed ratios (x == 1, the break points of atanf one ulp either side, exponent
    gaps around 60, 2^-29 and 2^25, (mb / 2, depth) of the stereo rigs), bit for bit; outside the domain NaN"""
    rng = np.random.default_rng(21)
    pos = lambda n: rng.integers(1, 0x7f800000, n, dtype=np.int64).astype(np.uint32).view(f32)  # noqa: E731
    y, x = [pos(1 << 20)], [pos(1 << 20)]
    xs = rng.uniform(0.01, 100.0, 1 << 18).astype(f32)
    y.append((xs * np.exp2(rng.uniform(-8, 8, 1 << 18))).astype(f32))
    x.append(xs)
    dy, dx = [], []
    for v in (0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -29, 2.0 ** 25, 2.0 ** 26, 1.0, 0.5, 3.0):
        for w in (f32(v), np.nextafter(f32(v), f32(0)), np.nextafter(f32(v), f32(np.inf))):
            dy += [w, w, f32(w * f32(3.0))]
            dx += [f32(1.0), f32(2.0), f32(3.0)]
    for gap in range(58, 64):
        dy += [f32(2.0 ** (gap - 40)), f32(1.5 * 2.0 ** (gap - 40)), f32(2.0 ** 20)]
        dx += [f32(2.0 ** -40), f32(1.25 * 2.0 ** -40), f32(2.0 ** (20 + gap - 126))]
    for mb in (0.110078, 0.537166, 0.08):
        for depth in (0.3, 1.0, 5.99, 40.0, 1e4, 1e-30):
            dy.append(f32(f32(mb) * f32(0.5)))
            dx.append(f32(depth))
    y = np.concatenate(y + [np.array(dy, f32)])
    x = np.concatenate(x + [np.array(dx, f32)])
    libm = C.CDLL("libm.so.6")
    libm.atan2f.restype, libm.atan2f.argtypes = C.c_float, [C.c_float, C.c_float]
    libm.cosf.restype, libm.cosf.argtypes = C.c_float, [C.c_float]
    want_a = np.array([libm.atan2f(float(a), float(b)) for a, b in zip(y, x)], f32)
    want_c = np.array([libm.cosf(float(f32(2.0) * a)) for a in want_a], f32)
    out_y = np.array([0.0, -1.0, np.inf, np.nan, 1.0, 1.0, 1.0], f32)
    out_x = np.array([1.0, 1.0, 1.0, 1.0, 0.0, -2.0, np.inf], f32)
    dev = torch.device("cuda", 0)
    ty = torch.from_numpy(np.concatenate([y, out_y])).to(dev)
    tx = torch.from_numpy(np.concatenate([x, out_x])).to(dev)
    ta, tc = torch.full_like(ty, 7.0), torch.full_like(ty, 7.0)
    assert orbamd.load().orbx_selftest_atan2f(ty.data_ptr(), tx.data_ptr(), ta.data_ptr(), tc.data_ptr(), ty.numel(),
                                              stream_of(torch)) == 0
    torch.cuda.synchronize()
    a, c = ta.cpu().numpy(), tc.cpu().numpy()
    n = len(y)
    bad = np.flatnonzero(a[:n].view(np.uint32) != want_a.view(np.uint32))
    assert bad.size == 0, (y[bad[:8]], x[bad[:8]], a[bad[:8]], want_a[bad[:8]])
    bad = np.flatnonzero(c[:n].view(np.uint32) != want_c.view(np.uint32))
    assert bad.size == 0, (y[bad[:8]], x[bad[:8]], c[bad[:8]], want_c[bad[:8]])
    assert np.isnan(a[n:]).all() and np.isnan(c[n:]).all()


# ------------------------------------------------------------------------------------------------ malformed input
def test_malformed_input_raises_the_flag_and_leaves_the_rest(torch, ctx, batch):
    bt = batch
    cleanK = bt.K.copy()
    for j in np.flatnonzero(np.isnan(cleanK["y"])):  # a clean batch: no row the contract excludes
        cleanK["y"].flat[j] = 100.0
    cleanK["octave"] = np.clip(cleanK["octave"], 0, 7)
    cleanM = np.where(bt.M >= 320, -1, bt.M)
    for f in range(6):
        cleanM[bt.q2 == f] = np.where(cleanM[bt.q2 == f] >= bt.cnt[f], -1, cleanM[bt.q2 == f])
    take_error(torch, ctx)
    clean = launch(torch, ctx, bt, K=cleanK, M=cleanM)
    assert take_error(torch, ctx) == 0
    assert not (clean["status"][:, :300] == TP.EXCLUDED).any()

    def others_same(got, touched):
        for p in range(8):
            if p in touched:
                continue
            for k in clean:
                lo, hi = (p, p + 1) if clean[k].shape[0] == 8 else (p * S, (p + 1) * S)
                assert bits(got[k][lo:hi]) == bits(clean[k][lo:hi]), (p, k)

    # a NaN pose entry of frame 3: every matched row of the pairs that use it is excluded
    T = bt.T.copy()
    T[3, 1, 2] = np.nan
    got = launch(torch, ctx, bt, K=cleanK, M=cleanM, T=T)
    assert take_error(torch, ctx) != 0
    others_same(got, {1, 6, 7})
    for p in (1, 6, 7):
        n1 = int(bt.cnt[bt.q1[p]])
        same_pair(got, p, n1, bt.host(p, K=cleanK, M=cleanM, T=T), "nan pose, pair %d" % p)
        assert set(got["status"][p, :n1].tolist()) <= {TP.NO_MATCH, TP.EXCLUDED} and int(got["nnew"][p]) == 0
    # an idx2 at and beyond the neighbour's count, a bad octave on either side
    for what, edit in (("idx2", lambda K, M: M.__setitem__((2, 0), 320)),
                       ("idx2 big", lambda K, M: M.__setitem__((2, 0), 2 ** 31 - 1)),
                       ("octave1", lambda K, M: K["octave"].__setitem__((4, 0), 8)),
                       ("octave2", lambda K, M: K["octave"].__setitem__((4, 0), -1))):
        K, M = cleanK.copy(), cleanM.copy()
        edit(K, M)
        got = launch(torch, ctx, bt, K=K, M=M)
        assert take_error(torch, ctx) != 0, what
        others_same(got, {2})
        assert got["status"][2, 0] == TP.EXCLUDED and int(got["nnew"][2]) == 0, what
        same_pair(got, 2, 1, bt.host(2, K=K, M=M), what)
    # a frame index outside the batch, a count above kp_stride
    for what, q1, q2, cnt in (("q1", 6, 1, None), ("q2", 0, -1, None), ("count", 0, 1, 321)):
        a, b = bt.q1.copy(), bt.q2.copy()
        a[4], b[4] = q1, q2
        c = bt.cnt.copy()
        touched = {4}
        if cnt is not None:
            c[4] = cnt  # frame 4 is pair 2's current keyframe
            a[4], touched = 4, {2, 4}
        got = launch(torch, ctx, bt, q1=a, q2=b, K=cleanK, M=cleanM, cnt=c)
        assert take_error(torch, ctx) != 0, what
        others_same(got, touched)
        for p in touched:
            assert int(got["nnew"][p]) == 0 and got["ranges"][p].tolist() == [p * S, p * S], what
            assert (got["status"][p] == TP.NO_MATCH).all() and not got["pos3"][p].any(), what
    assert take_error(torch, ctx) == 0


def test_empty_pair_list_is_a_no_op(torch, ctx, batch):
    g = batch.g.cstruct()
    fn = orbamd.load().orbm_create_new_map_points_batch_device
    assert fn(ctx, 0, None, None, 6, None, None, S, None, None, None, None, None, C.byref(g), 0, None,
              *([None] * 12), None) == 0


# ------------------------------------------------------------------------------------------------ the chain
def test_extract_to_new_map_points_to_track_local_chain(torch):
    """a 3-frame stereo batch at 640x480, the frames 14 steps of the synthetic pan apart (a 28 px shift: a baseline
    above the rig's): extraction, UndistortKeyPoints, ComputeStereoMatches, the stereo BF triangulation matcher, the
    new MapPoints and SearchLocalPoints over the produced table through its ranges, on one stream with no host step
    between them. Read back afterwards: the table equals the yardstick's and the host unit's on the same match rows,
    and the local-map search equals the CPU oracle fed the yardstick's table."""
    import frustum_py as FP
    import undistort_py as U
    from orbamd.device import STEREO_RIGS, BatchPipeline
    from orbamd.frame import image_bounds
    from orbamd.matcher import compute_f12, epipole
    from test_gpu_local import Expect, Frame, Table, same_frame
    W, H, B = 640, 480, 3
    cam = U.MY_YAML[0]
    rig = STEREO_RIGS["euroc"]
    pp = BatchPipeline(torch, W, H, B, nfeatures=500, stereo=rig, camera=cam.astuple())
    St = pp.stride
    ts = (7, 21, 35)  # the crop moves 2 px a step in x and stays at one y for t = 0 mod 7
    left = np.concatenate([orbamd.synth_frames(1, t, 1, W, H) for t in ts])
    right = np.concatenate([orbamd.synth_frames(1, t, 1, W, H, dx=8) for t in ts])
    imgs = torch.from_numpy(np.concatenate([left, right])).to(pp.dev)
    z = rig[0] / 8.0  # the fronto-parallel scene's depth at disparity 8
    step = np.array([-28.0 * z / cam.fx, 0.0, -0.002])  # the camera moves right: the image moves 28 px left
    poses = np.stack([TP.pose(np.eye(3), f * step) for f in range(B)])
    K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], f32)
    R, t1, t0 = np.eye(3, dtype=f32), poses[1, :3, 3].copy(), poses[0, :3, 3].copy()
    pp.F12 = compute_f12(R, t1, R, t0, K, K)
    pp.ex, pp.ey = epipole(R, t0, -t1, cam.fx, cam.fy, cam.cx, cam.cy)
    tposes = torch.from_numpy(poses).to(pp.dev)
    out = torch.full((B, St), -7, dtype=torch.int32, device=pp.dev)
    nm = torch.zeros(B, dtype=torch.int32, device=pp.dev)
    ntm = torch.zeros(B, dtype=torch.int32, device=pp.dev)
    inv = torch.zeros((B, B * St), dtype=torch.uint8, device=pp.dev)
    frame_mp = torch.full((B, St), -1, dtype=torch.int32, device=pp.dev)
    pp.extract(imgs)
    pp.match_pairs()
    t = pp.create_new_map_points(tposes)
    pp.track_local(tposes, t["pos"], t["normal"], t["min_dist"], t["max_dist"], t["desc"], t["flags"], frame_mp, 3.0,
                   out, nm, ntm, ranges=t["ranges"], in_view=inv)
    torch.cuda.synchronize()
    pp.check_error()
    pp.check_match_error()
    # the reference side, from the arrays read back
    g = TP.TriGeom(cam.fx, cam.fy, cam.cx, cam.cy, rig[0], b=rig[1])
    g.scale_factors[:8], g.level_sigma2[:8] = np.asarray(pp.scale, f32), np.asarray(pp.sigma2, f32)
    host = dict((k, v.cpu().numpy()) for k, v in t.items())
    frames = []
    for f in range(B):
        k = pp.host_keypoints_un(f)
        _, d = pp.host_keypoints(f)
        ur, dp, ns = pp.host_stereo(f)
        assert ns > 30
        frames.append((k, d, ur, dp))
    tab = dict(pos=np.zeros((B * St, 3), f32), normal=np.zeros((B * St, 3), f32), mind=np.zeros(B * St, f32),
               maxd=np.zeros(B * St, f32), desc=np.zeros((B * St, 32), np.uint8), flags=np.zeros(B * St, np.uint8))
    q1, q2 = pp.q1.cpu().numpy(), pp.q2.cpu().numpy()
    nnew = []
    for p in range(B):
        a, b = int(q1[p]), int(q2[p])
        (k1, d1, ur1, dp1), (k2, _, ur2, dp2) = frames[a], frames[b]
        m = pp.match[p, :len(k1)].cpu().numpy()
        ref = TP.triangulate_matches(g, 0, 1.0, poses[a], poses[b], k1, ur1, dp1, d1, k2, ur2, dp2, m)
        print("pair", p, "matches", int((m >= 0).sum()), dict((TP.NAMES[s], int(c)) for s, c in
                                                                enumerate(np.bincount(ref.status, minlength=14)) if c))
        hu = triangulate_matches(g.cstruct(), 0, 1.0, poses[a], poses[b], k1, ur1, dp1, d1, k2, ur2, dp2, m)
        assert ref.same_as(hu), "pair %d: host unit against yardstick" % p
        n1, nn = len(k1), ref.nnew
        assert bits(host["status"][p, :n1]) == bits(ref.status) and bits(host["pos3"][p, :n1]) == bits(ref.pos3), p
        assert int(host["nnew"][p]) == nn and host["ranges"][p].tolist() == [p * St, p * St + nn]
        sl = slice(p * St, p * St + nn)
        for kk, r in (("pos", ref.tab_pos), ("normal", ref.tab_normal), ("min_dist", ref.tab_min),
                      ("max_dist", ref.tab_max), ("desc", ref.tab_desc), ("flags", ref.tab_flags),
                      ("feat1", ref.feat1), ("feat2", ref.feat2)):
            assert bits(host[kk][sl]) == bits(r[:nn]), (p, kk)
        tab["pos"][sl], tab["normal"][sl], tab["mind"][sl], tab["maxd"][sl] = (ref.tab_pos[:nn], ref.tab_normal[:nn],
                                                                              ref.tab_min[:nn], ref.tab_max[:nn])
        tab["desc"][sl], tab["flags"][sl] = ref.tab_desc[:nn], ref.tab_flags[:nn]
        nnew.append(nn)
    assert min(nnew) > 0 and sum(nnew) > 30, nnew
    bnd, gw, gh = image_bounds(cam.astuple(), W, H)
    G = FP.Geom(cam.fx, cam.fy, cam.cx, cam.cy, rig[0], bnd, b=rig[1])
    G.scale_factors = np.asarray(pp.scale, f32)
    G.grid_w_inv, G.grid_h_inv = gw, gh
    table = Table(tab["pos"], tab["normal"], tab["mind"], tab["maxd"], tab["desc"], tab["flags"])
    got = (out.cpu().numpy(), nm.cpu().numpy(), ntm.cpu().numpy(), inv.cpu().numpy())
    ex = Expect(G)
    fmp = np.full((B, St), -1, np.int32)
    total = []
    for f in range(B):
        k, d, ur, _ = frames[f]
        fr = Frame(k, d, poses[f], ur)
        ref = ex.frame(f, fr, table, f * St, f * St + nnew[f], fmp[f], 3.0, True)
        total.append(same_frame(got, f, fr.n, ref, "chain frame %d" % f))
    print("nnew", nnew, "nmatches", total)
    assert max(total) > 0
    pp.close()

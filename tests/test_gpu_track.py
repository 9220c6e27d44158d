"""GPU: frame-to-frame tracking on a device batch. Frame::UnprojectStereo on the device against the host unit, bit for
bit, and orbm_search_by_projection_last_frame_batch_device against the CPU oracle
(oracle_py.search_by_projection_last_frame, never the per-call GPU entry): the whole d_match rows and d_nmatches of
every pair. Inputs are built by hand on the device with torch, except in the chain test, which extracts."""
import ctypes as C

import numpy as np
import pytest

import oracle_py
import orbamd
import proj_cases as pc
import proj_scenes as ps
import undistort_py as U
import unproject_py as UP
from orbamd.frame import make_camera, track_geom, unproject_stereo

pytestmark = pytest.mark.gpu

EDEVICE = -2


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx(torch):
    """one matcher context, hence one scratch buffer, for every launch of this module, large and small"""
    lib = orbamd.load()
    h = C.c_void_p()
    assert lib.orbm_create(0, C.byref(h)) == 0
    yield h
    lib.orbm_destroy(h)


# ------------------------------------------------------------------------------------------------ frames and geometry
class Fr:
    """one frame of a batch: what the entry reads of it as a current frame (kps, desc, uright, occ) and as a last
    frame (kps octave / angle, desc, pos, flags), and its pose"""

    def __init__(self, kps, desc, Tcw, uright=None, occ=None, pos=None, flags=None):
        n = len(kps)
        self.n = n
        self.kps = np.zeros(n, orbamd.kp_dtype)
        for f in ("x", "y", "octave", "angle"):
            self.kps[f] = kps[f]
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        self.Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(4, 4)
        self.uright = np.full(n, -1, np.float32) if uright is None else np.asarray(uright, np.float32)
        self.occ = np.zeros(n, np.uint8) if occ is None else np.asarray(occ, np.uint8)
        self.pos = np.zeros((n, 3), np.float32) if pos is None else np.asarray(pos, np.float32).reshape(n, 3)
        self.flags = np.zeros(n, np.uint8) if flags is None else np.asarray(flags, np.uint8)


class Geo:
    """the launch's orbm_track_geom, taken from a FrameView (the oracle's Frame side)"""
    NAMES = ("fx", "fy", "cx", "cy", "bf", "b", "min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv")

    def __init__(self, F, **over):
        for k in self.NAMES:
            setattr(self, k, np.float32(over.get(k, getattr(F, k))))
        self.scale = self.scale_factors = np.asarray(F.scale_factors, np.float32)

    def cstruct(self):
        return track_geom(self.fx, self.fy, self.cx, self.cy, self.bf, self.b,
                          (self.min_x, self.max_x, self.min_y, self.max_y), self.grid_w_inv, self.grid_h_inv,
                          self.scale)


def view_of(fr, G, use_uright=True, use_occ=True):
    """the oracle's Frame side of `fr` as a current frame under the launch geometry"""
    F = orbamd.FrameView(fr.kps, fr.desc, G.scale, 640, 480, G.fx, G.fy, G.cx, G.cy, bf=G.bf,
                         uright=fr.uright if use_uright else None, occupied=fr.occ if use_occ else None)
    for k in Geo.NAMES:
        setattr(F, k, getattr(G, k))
    return F


def mps_of(fr):
    """the oracle's MapPoint side of `fr` as a last frame: the documented meaning of the d_mp_flags bits"""
    fl = fr.flags
    return orbamd.MapPoints(fr.n, desc=fr.desc, pos=fr.pos, has_obs=(fl & 8) != 0,
                            skip=((fl & 1) == 0) | ((fl & 4) != 0), octave=fr.kps["octave"], angle=fr.kps["angle"])


def frame_of_view(F, Tcw):
    k = np.zeros(F.n, orbamd.kp_dtype)
    k["x"], k["y"], k["octave"], k["angle"] = F.x, F.y, F.octave, F.angle
    return Fr(k, F.desc, Tcw, F.uright, F.occupied)


def frame_of_mps(mps, Tl):
    """a last frame carrying the MapPoints of a per-call scene: a skipped entry is, alternately, a feature without a
    MapPoint (bit 0 clear) or an outlier (bit 2); bit 1 (bad) is set on every third and must be ignored"""
    n = mps.n
    k = np.zeros(n, orbamd.kp_dtype)
    k["x"], k["y"] = 1.0, 1.0
    k["octave"] = mps.octave
    if mps.angle is not None:
        k["angle"] = mps.angle
    i = np.arange(n)
    skip = np.zeros(n, bool) if mps.skip is None else mps.skip != 0
    has_obs = np.zeros(n, bool) if mps.has_obs is None else mps.has_obs != 0
    fl = np.where(skip, np.where(i % 2 == 0, 0, 1 | 4), 1) | np.where(has_obs, 8, 0) | np.where(i % 3 == 0, 2, 0)
    return Fr(k, mps.desc, Tl, pos=mps.pos, flags=fl)


def full_frame(seed, stereo=True, all_skipped=False):
    """a frame that can take both roles: real keypoints, and MapPoints back-projected from its own keypoints under its
    own pose, so that a nearby frame of the same stream finds them"""
    rng = np.random.default_rng(1000 + seed)
    F, k, d, scale = ps.make_frame(rng, 2, 40 + seed, stereo)
    Tcw = ps.pose(ps.rot(rng, 1.0), rng.normal(0, 0.02, 3))
    n = F.n
    pos = ps.backproject(rng, k, np.arange(n), Tcw)
    r = rng.random((4, n))
    fl = ((r[0] < 0.9) * 1) | ((r[1] < 0.3) * 2) | ((r[2] < 0.1) * 4) | ((r[3] < 0.85) * 8)
    if all_skipped:
        fl = np.where(np.arange(n) % 2 == 0, fl & ~1, fl | 4)
    return F, Fr(k, d, Tcw, F.uright, F.occupied, pos, fl)


def launch(torch, ctx, frames, pairs, G, th, mono, ori, use_uright=True, use_occ=True, S=None, counts=None):
    """one orbm_search_by_projection_last_frame_batch_device launch over hand-built device arrays: (match [npairs, S],
    nmatches [npairs]) as numpy, rows pre-filled with a sentinel"""
    nf = len(frames)
    S = max([fr.n for fr in frames] + [1]) if S is None else S
    K = np.zeros((nf, S), orbamd.kp_dtype)
    D = np.zeros((nf, S, 32), np.uint8)
    UR = np.full((nf, S), -1, np.float32)
    OC = np.zeros((nf, S), np.uint8)
    PO = np.zeros((nf, S, 3), np.float32)
    FL = np.zeros((nf, S), np.uint8)
    T = np.zeros((nf, 4, 4), np.float32)
    for f, fr in enumerate(frames):
        n = fr.n
        K[f, :n], D[f, :n], UR[f, :n], OC[f, :n], PO[f, :n], FL[f, :n], T[f] = (fr.kps, fr.desc, fr.uright, fr.occ,
                                                                                fr.pos, fr.flags, fr.Tcw)
    cnt = np.array([fr.n for fr in frames] if counts is None else counts, np.int32)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t = dict(k=up(K.view(np.float32).reshape(nf, S, 6)), d=up(D), ur=up(UR), oc=up(OC), po=up(PO), fl=up(FL), T=up(T),
             cnt=up(cnt), cur=up(np.array([p[0] for p in pairs], np.int32)),
             last=up(np.array([p[1] for p in pairs], np.int32)))
    out = torch.full((len(pairs), S), -7, dtype=torch.int32, device=dev)
    nm = torch.full((len(pairs),), -7, dtype=torch.int32, device=dev)
    g = G.cstruct()
    st = torch.cuda.current_stream(dev).cuda_stream
    rc = orbamd.load().orbm_search_by_projection_last_frame_batch_device(
        ctx, len(pairs), t["cur"].data_ptr(), t["last"].data_ptr(), nf, t["k"].data_ptr(), t["d"].data_ptr(),
        t["cnt"].data_ptr(), S, t["ur"].data_ptr() if use_uright else None,
        t["oc"].data_ptr() if use_occ else None, t["po"].data_ptr(), t["fl"].data_ptr(), t["T"].data_ptr(),
        C.byref(g), float(th), int(mono), int(ori), out.data_ptr(), nm.data_ptr(), st)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), nm.cpu().numpy()


def expect(frames, pair, G, th, mono, ori, use_uright=True, use_occ=True):
    cur, last = frames[pair[0]], frames[pair[1]]
    return oracle_py.search_by_projection_last_frame(view_of(cur, G, use_uright, use_occ), cur.Tcw, mps_of(last),
                                                     last.Tcw, th, mono, ori)


def same_pair(out_row, nm, ref, what):
    no, mo = ref
    n = len(mo)
    bad = np.nonzero(out_row[:n] != mo)[0]
    assert bad.size == 0, "%s: rows %s: gpu %s oracle %s" % (what, bad[:8], out_row[bad[:8]], mo[bad[:8]])
    assert int(nm) == no, "%s: nmatches %d, oracle %d" % (what, int(nm), no)
    assert (out_row[n:] == -7).all(), "%s: rows past the current frame's count were written" % what
    return no


def no_error(torch, ctx):
    st = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
    return orbamd.load().orbm_check_error(ctx, st)


# ------------------------------------------------------------------------------------------------ UnprojectStereo
def test_unproject_device_equals_host_bitwise(torch):
    S, counts = 128, [0, 1, 63, 64, 65, 128]
    cam, cols, rows = U.MY_YAML
    rng = np.random.default_rng(77)
    poses = UP.poses() + [ps.pose(ps.rot(rng, 30.0), rng.normal(0, 1.0, 3)) for _ in range(3)]
    kps, depth = UP.test_inputs(cols, rows, cam, 6 * S, seed=31)
    K = kps[:6 * S].reshape(6, S).copy()
    Z = depth[:6 * S].reshape(6, S).copy()
    Z[:, 0] = 2.5  # the one keypoint of the count-1 frame has a depth
    Z[5, 1:1 + len(UP.EDGE_DEPTHS)] = np.array(UP.EDGE_DEPTHS, np.float32)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tk, tz, tc = up(K.view(np.float32).reshape(6, S, 6)), up(Z), up(np.array(counts, np.int32))
    tT = up(np.stack(poses).astype(np.float32))
    lib = orbamd.load()
    ext = orbamd.ORBextractor(500, 1.2, 8, 20, 7, device=0, max_width=320, max_height=240, max_batch=1)
    st = torch.cuda.current_stream(dev).cuda_stream
    c = make_camera(cam.astuple())
    for with_flags in (True, False):
        pos = torch.full((6, S, 3), 123.0, dtype=torch.float32, device=dev)
        fl = torch.full((6, S), 0xEE, dtype=torch.uint8, device=dev)
        assert lib.orbx_unproject_stereo_batch_device(
            ext._h, C.byref(c), 6, tk.data_ptr(), tz.data_ptr(), tc.data_ptr(), S, tT.data_ptr(), pos.data_ptr(),
            fl.data_ptr() if with_flags else None, 9, st) == 0
        torch.cuda.synchronize()
        pos, fl = pos.cpu().numpy(), fl.cpu().numpy()
        for f, n in enumerate(counts):
            ref, valid = unproject_stereo(c, poses[f], K[f, :n], Z[f, :n])
            assert np.array_equal(pos[f, :n].view(np.uint32), ref.view(np.uint32)), f
            assert (pos[f, n:] == 123.0).all(), f
            assert (fl[f, n:] == 0xEE).all()
            assert np.array_equal(fl[f, :n], valid * 9 if with_flags else np.full(n, 0xEE, np.uint8)), f
    assert 0 < int(valid.sum()) < 128 and not np.array_equal(ref[valid != 0], np.zeros_like(ref[valid != 0]))
    ext.close()


# ------------------------------------------------------------------------------------------------ against the oracle
LAST_FRAME_CONFIGS = [(4, False, 0, True, 7.0), (5, True, 0, True, 15.0), (6, False, 1, False, 7.0),
                      (7, False, -1, True, 7.0)]  # test_gpu_projection.py::test_projection_last_frame


@pytest.fixture(scope="module")
def four_scenes():
    """the four scenes as eight frames (current 2 s, last 2 s + 1) and the stereo geometry they share"""
    frames, G = [], None
    for seed, bmono, forward, ori, th in LAST_FRAME_CONFIGS:
        F, Tcw, mps, Tl = ps.last_frame_scene(seed, bmono, not bmono, forward)
        frames += [frame_of_view(F, Tcw), frame_of_mps(mps, Tl)]
        if not bmono and G is None:
            G = Geo(F)
    return frames, G


def test_four_configurations_in_one_launch(torch, ctx, four_scenes):
    """every configuration's (th, bMono, check_ori) over all four scenes as one launch of four pairs: stereo and mono,
    forward, backward and neither, check_ori on and off; then the pair list permuted with one pair duplicated"""
    frames, G = four_scenes
    pairs = [(2 * s, 2 * s + 1) for s in range(4)]
    perm = [2, 0, 3, 1, 2]
    for ci, (seed, bmono, forward, ori, th) in enumerate(LAST_FRAME_CONFIGS):
        Gc = Geo(G, bf=0.0, b=0.0) if bmono else G  # a monocular Frame has mbf = 0 (proj_scenes.make_frame)
        out, nm = launch(torch, ctx, frames, pairs, Gc, th, bmono, ori)
        for s, p in enumerate(pairs):
            n = same_pair(out[s], nm[s], expect(frames, p, Gc, th, bmono, ori), "config %d scene %d" % (ci, s))
            if s == ci:
                assert n > frames[p[0]].n // 4
        out2, nm2 = launch(torch, ctx, frames, [pairs[i] for i in perm], Gc, th, bmono, ori)
        for j, i in enumerate(perm):
            assert np.array_equal(out2[j], out[i]) and nm2[j] == nm[i], (ci, j, i)
    assert no_error(torch, ctx) == 0


def last_calls(g):
    return [t for t in g.calls() if t[0]["kind"] == "last"]


@pytest.mark.parametrize("gname", pc.GROUPS)
def test_projection_cases_last(torch, ctx, gname):
    """every "last" call of the group: its Frame view is the current frame, a last frame carries its MapPoints; calls
    that share th, bMono and check_ori run as one launch (the geometry is the group's), the whole match array and the
    count equal pc.run_oracle's"""
    g = pc.group(gname)
    calls = last_calls(g)
    want = sorted(c["key"] for c in g.variants if c["kind"] == "last")
    assert len(calls) == len(want)
    if not want:  # the group has no SearchByProjection(CurrentFrame, LastFrame) call (GROUPS_WITHOUT_LAST below)
        return
    ran = []
    by_key = {}
    for c, F, mps in calls:
        by_key.setdefault((c["th"], c["bmono"], c["check_ori"]), []).append((c, F, mps))
    for (th, bmono, ori), grp in by_key.items():
        F = grp[0][1]
        frames = [frame_of_view(F, grp[0][0]["Tcw"])] + [frame_of_mps(mps, c["Tl"]) for c, _, mps in grp]
        pairs = [(0, 1 + i) for i in range(len(grp))]
        out, nm = launch(torch, ctx, frames, pairs, Geo(F), th, bmono, ori, use_uright=F.uright is not None)
        for i, (c, F, mps) in enumerate(grp):
            ref = pc.run_oracle(c, F, mps)
            bad = np.nonzero(out[i, :F.n] != ref[1])[0]
            where = g.describe(c, feats=bad, queries=[v for v in list(out[i, bad]) + list(ref[1][bad]) if v >= 0])
            same_pair(out[i], nm[i], ref, where)
            ran.append(c["key"])
    assert sorted(ran) == want
    assert no_error(torch, ctx) == 0


GROUPS_WITHOUT_LAST = ["ratio"]  # the second-best ratio test belongs to SearchByProjection(F, vpMapPoints) alone


def test_no_last_case_is_left_out():
    """the parametrisation above covers pc.GROUPS and each group asserts that it ran every one of its "last" variants;
    here: which groups have none, and how many cases that makes"""
    n = {name: sum(1 for c in pc.group(name).variants if c["kind"] == "last") for name in pc.GROUPS}
    assert sorted(k for k, v in n.items() if v == 0) == GROUPS_WITHOUT_LAST
    assert sum(n.values()) == sum(len(last_calls(pc.group(name))) for name in pc.GROUPS) >= 12


# ------------------------------------------------------------------------------------------------ degenerate shapes
@pytest.fixture(scope="module")
def degenerate():
    FA, A = full_frame(1)
    FB, B = full_frame(2)
    _, Cs = full_frame(3, all_skipped=True)
    empty = Fr(np.zeros(0, orbamd.kp_dtype), np.zeros((0, 32), np.uint8), np.eye(4))
    return [A, B, empty, Cs], Geo(FA)


@pytest.mark.parametrize("arrays", [True, False])
def test_degenerate_shapes_in_one_launch(torch, ctx, degenerate, arrays):
    """cur == last, an empty current frame, an empty last frame, a last frame whose features are all skipped, a frame
    whose count is kp_stride; with d_uright and d_occupied both given and both NULL"""
    frames, G = degenerate
    S = max(fr.n for fr in frames)
    pairs = [(0, 0), (2, 0), (0, 2), (0, 3), (0, 1), (1, 0), (2, 2), (1, 1)]
    assert any(frames[c].n == S for c, _ in pairs) and frames[2].n == 0
    assert not ((frames[3].flags & 1) != 0)[(frames[3].flags & 4) == 0].any()
    out, nm = launch(torch, ctx, frames, pairs, G, 7.0, False, True, use_uright=arrays, use_occ=arrays, S=S)
    got = [same_pair(out[i], nm[i], expect(frames, p, G, 7.0, False, True, arrays, arrays), "pair %s" % (p,))
           for i, p in enumerate(pairs)]
    assert got[0] > frames[0].n // 4 and got[1] == got[2] == got[3] == got[6] == 0 and got[4] > 0
    assert no_error(torch, ctx) == 0


# ------------------------------------------------------------------------------------------------ validation
def test_malformed_pairs_raise_the_flag_and_leave_the_rest(torch, ctx, degenerate):
    """run once: a frame index out of range (both sides), an octave-31 keypoint among the accepted features, a
    last-frame count above kp_stride; beside them a valid pair, and a current frame whose count above kp_stride is
    clamped"""
    frames, G = degenerate
    A, B = frames[0], frames[1]
    S = max(A.n, B.n)
    big = A if A.n == S else B  # the frame that fills kp_stride: its count is overstated below
    th, mono, ori = 7.0, False, True
    ref_ab = oracle_py.search_by_projection_last_frame(view_of(A, G), A.Tcw, mps_of(B), B.Tcw, th, mono, ori)
    j = int(ref_ab[1][ref_ab[1] >= 0][0])  # a feature of B that is an accepted query
    Bv = Fr(B.kps, B.desc, B.Tcw, B.uright, B.occ, B.pos, B.flags)
    jskip = int(np.nonzero((B.flags & 1) == 0)[0][0])
    Bv.kps["octave"][jskip] = 31  # a skipped feature's octave is never read
    Cbad = Fr(B.kps, B.desc, B.Tcw, B.uright, B.occ, B.pos, B.flags)
    Cbad.kps["octave"][j] = 31
    fs = [A, Bv, Cbad, big]
    counts = [A.n, Bv.n, Cbad.n, S + 5]
    pairs = [(0, 1), (7, 1), (0, -1), (0, 2), (0, 3), (3, 1)]
    assert no_error(torch, ctx) == 0
    out, nm = launch(torch, ctx, fs, pairs, G, th, mono, ori, S=S, counts=counts)
    assert no_error(torch, ctx) == EDEVICE
    assert no_error(torch, ctx) == 0
    same_pair(out[0], nm[0], ref_ab, "valid pair")
    assert ref_ab[0] > 0
    for i in (1, 2, 3, 4):
        assert nm[i] == 0 and (out[i] == -1).all(), i
    ref_clamped = oracle_py.search_by_projection_last_frame(view_of(big, G), big.Tcw, mps_of(Bv), Bv.Tcw, th, mono, ori)
    same_pair(out[5], nm[5], ref_clamped, "clamped current count")


def test_npairs_zero_is_a_no_op(torch, ctx, degenerate):
    frames, G = degenerate
    out, nm = launch(torch, ctx, frames[:2], [], G, 7.0, False, True)
    assert out.shape[0] == 0 and nm.shape[0] == 0


def test_more_pairs_than_one_search_launch_takes(torch, ctx):
    """the search kernels take at most 32768 calls per launch (a grid dimension): 32770 pairs of an 8-feature frame go
    out as two rounds of launches, and the pairs of the second round equal the oracle like those of the first"""
    g = pc.group("boundary")
    c, F, mps = last_calls(g)[0]
    frames = [frame_of_view(F, c["Tcw"]), frame_of_mps(mps, c["Tl"])]
    ref = pc.run_oracle(c, F, mps)
    npairs = 32770
    out, nm = launch(torch, ctx, frames, [(0, 1)] * npairs, Geo(F), c["th"], c["bmono"], c["check_ori"],
                     use_uright=F.uright is not None)
    assert ref[0] > 0 and (nm == ref[0]).all() and (out[:, :F.n] == ref[1][None, :]).all()
    assert no_error(torch, ctx) == 0


# ------------------------------------------------------------------------------------------------ the chain
def test_extract_undistort_stereo_unproject_track_chain(torch):
    """a 4-frame stereo batch at 640x480 / 1000 features: extraction, UndistortKeyPoints, ComputeStereoMatches,
    UnprojectStereo and SearchByProjection(frame f + 1, frame f) on one stream with no host step between them; read
    back afterwards, the positions equal the host unit on the read-back mvKeysUn / mvDepth and the matches equal the
    oracle on those positions"""
    from orbamd.device import STEREO_RIGS, BatchPipeline
    from orbamd.frame import image_bounds
    W, H, B = 640, 480, 4
    cam = U.MY_YAML[0]
    rig = STEREO_RIGS["euroc"]
    pp = BatchPipeline(torch, W, H, B, nfeatures=1000, stereo=rig, camera=cam.astuple())
    left = orbamd.synth_frames(1, 5, B, W, H)
    right = orbamd.synth_frames(1, 5, B, W, H, dx=8)
    imgs = torch.from_numpy(np.concatenate([left, right])).to(pp.dev)
    rng = np.random.default_rng(3)
    poses = np.stack([ps.pose(ps.rot(rng, 0.2), rng.normal(0, 0.01, 3)) for _ in range(B)]).astype(np.float32)
    tposes = torch.from_numpy(poses).to(pp.dev)
    flags = torch.zeros((B, pp.stride), dtype=torch.uint8, device=pp.dev)
    cur = torch.arange(1, B, dtype=torch.int32, device=pp.dev)
    last = torch.arange(0, B - 1, dtype=torch.int32, device=pp.dev)
    out = torch.full((B - 1, pp.stride), -7, dtype=torch.int32, device=pp.dev)
    nm = torch.zeros(B - 1, dtype=torch.int32, device=pp.dev)
    th, mono, ori = 15.0, False, True
    pp.extract(imgs)  # extraction, undistortion and stereo matching
    pos = pp.unproject(tposes, mp_flags=flags)
    pp.track_pairs(cur, last, pos, flags, tposes, th, mono, ori, out, nm)
    torch.cuda.synchronize()
    pp.check_error()
    pp.check_match_error()
    out, nm, pos, flags = out.cpu().numpy(), nm.cpu().numpy(), pos.cpu().numpy(), flags.cpu().numpy()
    b, gw, gh = image_bounds(cam.astuple(), W, H)
    frames = []
    for f in range(B):
        k = pp.host_keypoints_un(f)
        _, d = pp.host_keypoints(f)
        ur, dp, ns = pp.host_stereo(f)
        n = len(k)
        ref, valid = unproject_stereo(cam.astuple(), poses[f], k, dp)
        assert ns > 50 and np.array_equal(pos[f, :n].view(np.uint32), ref.view(np.uint32)), f
        assert np.array_equal(flags[f, :n], valid * 9), f
        frames.append(Fr(k, d, poses[f], ur, None, pos[f, :n], flags[f, :n]))
    F0 = orbamd.FrameView(frames[0].kps, frames[0].desc, pp.scale, W, H, cam.fx, cam.fy, cam.cx, cam.cy, bf=rig[0])
    G = Geo(F0, b=rig[1], min_x=b[0], max_x=b[1], min_y=b[2], max_y=b[3], grid_w_inv=gw, grid_h_inv=gh)
    got = []
    for p in range(B - 1):
        ref = expect(frames, (p + 1, p), G, th, mono, ori, True, False)
        n = frames[p + 1].n
        assert np.array_equal(out[p, :n], ref[1]) and nm[p] == ref[0], p
        got.append(ref[0])
    assert max(got) > 0
    pp.close()

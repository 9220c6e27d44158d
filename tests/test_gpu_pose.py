"""GPU: Optimizer::PoseOptimization on a device batch. orbm_pose_optimization_batch_device (k_pose_optimize) against
the host unit csrc/pose_optimize.c on every output as raw bits: the CPU test's scenes packed into batches, the sizes
around the lane and chunk boundaries of the ordered walk, repeated and permuted jobs, in-place poses, malformed jobs,
the optional outputs against a numpy statement of Tracking's discard loop, the device so3_sincos / sqrt / division
against the host, and the tracking chain on one stream."""
import ctypes as C
import math

import numpy as np
import pytest

import orbamd
import pose_py as P
import undistort_py as U
from orbamd.frame import pose_optimization, track_geom

pytestmark = pytest.mark.gpu

f32 = np.float32
SENT = 0x77
EDEVICE = -2


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


def geom_of(s):
    return track_geom(s.cam[0], s.cam[1], s.cam[2], s.cam[3], s.cam[4], 0.08, (0, 640, 0, 480), 0.1, 0.1,
                      [1.2 ** i for i in range(P.NLEVELS)])


class Batch:
    """scenes of one camera as frames of one device batch at kp_stride S: keypoints, counts, uright (-1 where a scene
    is monocular), the poses, one position table (the scenes' tables back to back) and one job per scene"""

    def __init__(self, scenes, S):
        self.scenes, self.S = scenes, S
        nf = len(scenes)
        self.kps = np.zeros((nf, S), orbamd.kp_dtype)
        self.ur = np.full((nf, S), -1.0, f32)
        self.counts = np.zeros(nf, np.int32)
        self.T = np.zeros((nf, 16), f32)
        self.mp = np.full((nf, S), -1, np.int32)
        pos, base = [], 0
        for f, s in enumerate(scenes):
            assert s.n <= S and s.cam == scenes[0].cam
            self.kps[f, :s.n] = s.kps
            if s.uright is not None:
                self.ur[f, :s.n] = s.uright
            self.counts[f] = s.n
            self.T[f] = s.T0.reshape(16)
            self.mp[f, :s.n] = np.where(s.mp_index >= 0, s.mp_index + base, -1)
            # beyond the count: garbage that must not be read as edges
            self.mp[f, s.n:] = 0
            pos.append(s.pos)
            base += len(s.pos)
        self.pos = np.concatenate(pos).astype(f32)
        self.frames = np.arange(nf, dtype=np.int32)

    def host(self, f, mp_row=None, T=None, pos=None):
        """the host unit on frame f: (Tcw [16], outlier [S] from a SENT-filled row, ninliers, status)"""
        s = self.scenes[f]
        n = int(self.counts[f])
        mp = self.mp[f] if mp_row is None else mp_row
        r = pose_optimization(geom_of(s), s.inv, self.T[f] if T is None else T, self.kps[f, :n], self.ur[f, :n],
                              mp[:n], self.pos if pos is None else pos, outlier=np.full(n, SENT, np.uint8))
        out = np.full(self.S, SENT, np.uint8)
        out[:n] = r.outlier
        return r.Tcw.reshape(16), out, r.ninliers, r.status


def launch(torch, ctx, bt, frames=None, mp=None, T=None, pos=None, counts=None, mrows=None, alias=False, flags=None,
           frame_mp=None, with_nmm=True, nframes=None):
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    frames = bt.frames if frames is None else np.asarray(frames, np.int32)
    mp = bt.mp[np.clip(frames, 0, len(bt.scenes) - 1)] if mp is None else mp
    J, S = len(frames), bt.S
    pos = bt.pos if pos is None else pos
    t_kps = up(bt.kps.view(np.uint8).reshape(len(bt.scenes), S, 24))
    t_ur, t_cnt = up(bt.ur), up(bt.counts if counts is None else counts)
    t_fr, t_mp, t_pos = up(frames), up(mp), up(pos)
    t_Tin = up(bt.T if T is None else T)
    t_Tout = t_Tin if alias else torch.full((J, 16), 7.0, dtype=torch.float32, device=dev)
    t_out = torch.full((J, S), SENT, dtype=torch.uint8, device=dev)
    t_ninl = torch.full((J,), -7, dtype=torch.int32, device=dev)
    t_nmm = torch.full((J,), -7, dtype=torch.int32, device=dev)
    t_st = torch.full((J,), -7, dtype=torch.int8, device=dev)
    t_fl = None if flags is None else up(flags)
    t_fmp = None if frame_mp is None else up(frame_mp)
    s0 = bt.scenes[0]
    g = geom_of(s0)
    inv = np.zeros(16, f32)
    inv[:P.NLEVELS] = s0.inv
    rc = orbamd.load().orbm_pose_optimization_batch_device(
        ctx, J, t_fr.data_ptr(), len(bt.scenes) if nframes is None else nframes, t_kps.data_ptr(), t_cnt.data_ptr(), S,
        t_ur.data_ptr(), C.byref(g), inv.ctypes.data, t_mp.data_ptr(), t_pos.data_ptr(),
        len(pos) if mrows is None else mrows, t_Tin.data_ptr(), t_Tout.data_ptr(), t_out.data_ptr(),
        None if t_fl is None else t_fl.data_ptr(), None if t_fmp is None else t_fmp.data_ptr(), t_ninl.data_ptr(),
        t_nmm.data_ptr() if with_nmm else None, t_st.data_ptr(), stream_of(torch))
    assert rc == 0
    torch.cuda.synchronize()
    r = dict(T=t_Tout.cpu().numpy(), outlier=t_out.cpu().numpy(), ninl=t_ninl.cpu().numpy(), nmm=t_nmm.cpu().numpy(),
             st=t_st.cpu().numpy())
    if t_fl is not None:
        r["flags"] = t_fl.cpu().numpy()
    if t_fmp is not None:
        r["frame_mp"] = t_fmp.cpu().numpy()
    return r


def same_job(got, j, ref, what):
    T, out, ninl, st = ref
    assert got["T"][j].tobytes() == T.tobytes(), what + ": pose"
    assert np.array_equal(got["outlier"][j], out), what + ": outlier"
    assert got["ninl"][j] == ninl and got["st"][j] == st, (what, got["ninl"][j], ninl, got["st"][j], st)


def directed_scenes(cam):
    ax = np.array([0.01, 1.01, 0.01])
    return [P.make_scene(cam, 50, "stereo", 0.0, outliers=0.0, seed=21, perturb=(0.0, 0.0)),        # at the optimum
            P.make_scene(cam, 60, "mixed", 0.5, seed=13, perturb=(0.3, math.radians(8.0))),        # rejected trials
            P.make_scene(cam, 40, "mixed", 0.5, seed=31, T_true=P.pose(P.rot(ax, math.radians(179.5)), [0, 0, 0.5])),
            P.make_scene(cam, 9, "mono", 0.3, seed=17), P.make_scene(cam, 2, "stereo", 0.0, seed=18)]


@pytest.mark.parametrize("cam", sorted(U.CAMERAS))
def test_kernel_equals_host_unit_bitwise(torch, ctx, cam):
    """the CPU test's scenes of one camera and the directed ones as one batch at stride 1024, 1000 features included"""
    scenes = P.camera_scenes(cam) + directed_scenes(cam)
    scenes.append(P.make_scene(cam, 1000, "mixed", 0.5, seed=5, unmatched=0.024, stride=1024))
    bt = Batch(scenes, 1024)
    assert take_error(torch, ctx) == 0
    got = launch(torch, ctx, bt)
    assert take_error(torch, ctx) == 0
    for j, s in enumerate(scenes):
        same_job(got, j, bt.host(j), s.name)
    assert (got["st"] == 0).sum() >= len(scenes) - 1 and (got["st"] == P.TOO_FEW).sum() == 1


@pytest.mark.parametrize("S,sizes", [(64, (0, 1, 2, 3, 9, 10, 63, 64)), (320, (255, 256, 257))])
def test_sizes_across_lane_and_chunk_boundaries(torch, ctx, S, sizes):
    scenes = [P.make_scene("my", n, "mixed", 0.3, seed=100 + n, unmatched=0.0) for n in sizes]
    assert [s.n for s in scenes] == list(sizes)
    bt = Batch(scenes, S)
    got = launch(torch, ctx, bt)
    assert take_error(torch, ctx) == 0
    for j, s in enumerate(scenes):
        same_job(got, j, bt.host(j), "n = %d" % s.n)


def test_chi2_exactly_at_the_float_threshold(torch, ctx):
    """the CPU test's threshold vectors through the kernel: (float)chi2 on the threshold from either side in double,
    one float above, one float below, mono and stereo; flags 0 0 1 0 each, and every output equal to the host unit"""
    s, want, _ = P.threshold_scene()
    bt = Batch([s], 64)
    got = launch(torch, ctx, bt)
    assert take_error(torch, ctx) == 0
    assert got["outlier"][0, :8].tolist() == [0, 0, 1, 0, 0, 0, 1, 0] == want.tolist()
    assert got["ninl"][0] == 6 and got["st"][0] == P.OK
    same_job(got, 0, bt.host(0), "threshold")


@pytest.fixture(scope="module")
def small():
    return Batch(P.camera_scenes("my", n=70)[:4] + [P.make_scene("my", 2, "stereo", 0.0, seed=18)], 128)


def test_one_frame_in_three_jobs_and_permuted_jobs(torch, ctx, small):
    """frame 1 in three jobs with different MapPoint rows (all, every other one, a block), and a permuted job list"""
    bt = small
    rows = [bt.mp[1].copy() for _ in range(3)]
    rows[1][::2] = -1
    rows[2][40:] = -1
    frames = [1, 0, 1, 3, 1, 2, 4]
    mp = np.stack([rows[0], bt.mp[0], rows[1], bt.mp[3], rows[2], bt.mp[2], bt.mp[4]])
    got = launch(torch, ctx, bt, frames=frames, mp=mp)
    for j, f in enumerate(frames):
        same_job(got, j, bt.host(f, mp_row=mp[j]), "job %d" % j)
    assert len({got["T"][j].tobytes() for j in (0, 2, 4)}) == 3
    perm = [6, 2, 5, 0, 3, 1, 4]
    got2 = launch(torch, ctx, bt, frames=[frames[p] for p in perm], mp=mp[perm])
    for k in ("T", "outlier", "ninl", "st", "nmm"):
        assert np.array_equal(got2[k].view(np.uint8), got[k][perm].view(np.uint8)), k
    assert take_error(torch, ctx) == 0


def test_poses_in_place(torch, ctx, small):
    sep = launch(torch, ctx, small)
    inp = launch(torch, ctx, small, alias=True)
    for k in ("T", "outlier", "ninl", "st"):
        assert np.array_equal(sep[k].view(np.uint8), inp[k].view(np.uint8)), k


def test_malformed_jobs_raise_the_flag_and_leave_the_rest(torch, ctx, small):
    bt = small
    clean = launch(torch, ctx, bt)
    assert take_error(torch, ctx) == 0

    def others_same(got, touched):
        for j in range(len(bt.scenes)):
            if j not in touched:
                for k in ("T", "outlier", "ninl", "st", "nmm"):
                    assert got[k][j].tobytes() == clean[k][j].tobytes(), (j, k)

    def excluded(got, j, T):
        assert got["st"][j] == P.EXCLUDED and got["ninl"][j] == 0 and (got["outlier"][j] == SENT).all()
        assert got["T"][j].tobytes() == T.tobytes()
    edge = int(np.flatnonzero(bt.mp[1, :bt.counts[1]] >= 0)[3])
    # a count above kp_stride is clamped: the rows beyond the count are features like any other
    cnt = bt.counts.copy()
    cnt[0] = bt.S + 5
    mp = bt.mp.copy()
    mp[0, bt.counts[0]:] = -1
    got = launch(torch, ctx, bt, counts=cnt, mp=mp)
    assert take_error(torch, ctx) == EDEVICE
    others_same(got, ())
    # an mp_index >= mrows counts as no MapPoint
    mp = bt.mp.copy()
    mp[1, edge] = len(bt.pos)
    got = launch(torch, ctx, bt, mp=mp)
    assert take_error(torch, ctx) == EDEVICE
    others_same(got, (1,))
    ref_row = bt.mp[1].copy()
    ref_row[edge] = -1
    same_job(got, 1, bt.host(1, mp_row=ref_row), "mp_index >= mrows")
    # a frame index outside the batch: nothing but the status, the counts and the flag
    for bad in (-1, len(bt.scenes)):
        fr = bt.frames.copy()
        fr[2] = bad
        got = launch(torch, ctx, bt, frames=fr, mp=bt.mp)
        assert take_error(torch, ctx) == EDEVICE
        others_same(got, (2,))
        excluded(got, 2, np.full(16, 7.0, f32))
    # the rows the contract excludes
    def with_kp(field, v):
        k = bt.kps.copy()
        k[field][1, edge] = v
        return dict(kps=k)
    T = bt.T.copy()
    T[1, 6] = np.inf
    pos = bt.pos.copy()
    pos[bt.mp[1, edge], 2] = np.nan
    ur = bt.ur.copy()
    ur[1, edge] = np.nan
    zpos = bt.pos.copy()  # a point in the camera's plane under the identity: chi2 is not finite
    zpos[bt.mp[1, edge]] = (0.5, 0.5, 0.0)
    zT = bt.T.copy()
    zT[1] = np.eye(4, dtype=f32).reshape(16)
    saved = bt.kps, bt.ur
    for what, kw in (("octave", with_kp("octave", 8)), ("octave < 0", with_kp("octave", -3)),
                     ("x", with_kp("x", np.inf)),
                     ("pose", dict(T=T)), ("pos", dict(pos=pos)), ("uright", dict(ur=ur)),
                     ("chi2", dict(pos=zpos, T=zT))):
        bt.kps = kw.pop("kps", saved[0])
        bt.ur = kw.pop("ur", saved[1])
        try:
            got = launch(torch, ctx, bt, **kw)
        finally:
            bt.kps, bt.ur = saved
        assert take_error(torch, ctx) == EDEVICE, what
        others_same(got, (1,))
        excluded(got, 1, kw.get("T", bt.T)[1])
    assert take_error(torch, ctx) == 0


def test_optional_outputs_are_the_discard_loop(torch, ctx, small):
    """d_mp_flags bit 2 := outlier with the other bits kept, d_frame_mp := -1 on outliers, d_nmatches_map = the kept
    features with bit 3, against numpy; rows beyond the count and features without a MapPoint untouched"""
    bt = small
    rng = np.random.default_rng(6)
    J, S = len(bt.scenes), bt.S
    flags = rng.integers(0, 256, (J, S)).astype(np.uint8)
    fmp = rng.integers(0, 1000, (J, S)).astype(np.int32)
    got = launch(torch, ctx, bt, flags=flags, frame_mp=fmp)
    plain = launch(torch, ctx, bt, with_nmm=False)
    assert take_error(torch, ctx) == 0
    for k in ("T", "outlier", "ninl", "st"):
        assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k
    assert (plain["nmm"] == -7).all()
    for j in range(J):
        n = int(bt.counts[j])
        has = np.zeros(S, bool)
        has[:n] = bt.mp[j, :n] >= 0
        o = got["outlier"][j]
        assert (o[has] <= 1).all() and (o[~has] == SENT).all()
        want_fl = np.where(has, (flags[j] & ~np.uint8(4)) | (np.where(has, o, 0) << 2).astype(np.uint8), flags[j])
        want_mp = np.where(has & (o == 1), -1, fmp[j])
        assert np.array_equal(got["flags"][j], want_fl) and np.array_equal(got["frame_mp"][j], want_mp), j
        assert got["nmm"][j] == int((has & (o == 0) & ((flags[j] & 8) != 0)).sum()), j
    assert (got["outlier"] == 1).sum() > 10
    # without d_mp_flags every kept feature counts
    got = launch(torch, ctx, bt)
    for j in range(J):
        n = int(bt.counts[j])
        assert got["nmm"][j] == int(((bt.mp[j, :n] >= 0) & (got["outlier"][j, :n] == 0)).sum())


def test_empty_job_list_is_a_no_op(torch, ctx, small):
    g = geom_of(small.scenes[0])
    inv = np.zeros(16, f32)
    fn = orbamd.load().orbm_pose_optimization_batch_device
    assert fn(ctx, 0, None, 5, None, None, 128, None, C.byref(g), inv.ctypes.data, None, None, 0, *([None] * 8),
              None) == 0


def test_device_so3_sincos_sqrt_and_division_equal_host(torch):
    """the device so3_sincos against the host statement, and the device's double sqrt and 1 / x against the host's
    correctly rounded ones, on 2^16 values and the directed angles, bit for bit"""
    lib = orbamd.load()
    rng = np.random.default_rng(9)
    directed = [1e-5, 0.5, 1.0, 1048575.9, 1048576.0, 2e6]
    for k in range(1, 12):
        for base in (k * math.pi / 4, k * math.pi / 2):
            directed += [base, np.nextafter(base, 0), np.nextafter(base, 100)]
    v = np.concatenate([rng.uniform(1e-5, math.pi, 1 << 15), 10 ** rng.uniform(-12, 12, (1 << 15) - len(directed)),
                        directed])
    assert len(v) == 1 << 16
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(v).to(dev)
    outs = [torch.zeros_like(t) for _ in range(4)]
    assert lib.orbx_selftest_so3(t.data_ptr(), *[o.data_ptr() for o in outs], len(v), stream_of(torch)) == 0
    torch.cuda.synchronize()
    sn, cs, sq, rc = [o.cpu().numpy() for o in outs]
    hs, hc = np.zeros_like(v), np.zeros_like(v)
    assert lib.orbx_test_so3_sincos(v.ctypes.data, hs.ctypes.data, hc.ctypes.data, len(v)) == 0
    assert sn.tobytes() == hs.tobytes() and cs.tobytes() == hc.tobytes()
    assert sq.tobytes() == np.sqrt(v).tobytes() and rc.tobytes() == (1.0 / v).tobytes()


# ------------------------------------------------------------------------------------------------ the chain
def test_tracking_chain_on_one_stream(torch):
    """a 4-frame stereo batch at 640x480: extraction, UndistortKeyPoints, ComputeStereoMatches, UnprojectStereo,
    SearchByProjection(frame f, frame f - 1), PoseOptimization, SearchLocalPoints under the new poses over the pruned
    frame_mp, PoseOptimization again, on one stream with no host step between them. Read back afterwards: both
    optimisations equal the host unit on the read-back match rows, and the local search equals the CPU oracle under
    the first optimisation's poses and pruned frame_mp."""
    import frustum_py as FP
    from orbamd.device import STEREO_RIGS, BatchPipeline
    from orbamd.frame import image_bounds
    from test_gpu_local import Expect, Frame, Table, same_frame
    W, H, B = 640, 480, 4
    cam = U.MY_YAML[0]
    rig = STEREO_RIGS["euroc"]
    pp = BatchPipeline(torch, W, H, B, nfeatures=500, stereo=rig, camera=cam.astuple())
    St, dev = pp.stride, pp.dev
    ts = (7, 14, 21, 28)  # the crop moves 2 px a step in x and stays at one y for t = 0 mod 7
    left = np.concatenate([orbamd.synth_frames(1, t, 1, W, H) for t in ts])
    right = np.concatenate([orbamd.synth_frames(1, t, 1, W, H, dx=8) for t in ts])
    imgs = torch.from_numpy(np.concatenate([left, right])).to(dev)
    z = rig[0] / 8.0  # the fronto-parallel scene's depth at disparity 8
    step = np.array([-14.0 * z / cam.fx, 0.0, 0.0])  # the camera moves right: the image moves 14 px left a frame
    poses = np.stack([P.pose(np.eye(3), f * step) for f in range(B)]).astype(f32)
    tposes = torch.from_numpy(poses).to(dev)
    flags = torch.zeros((B, St), dtype=torch.uint8, device=dev)
    cur = torch.arange(B, dtype=torch.int32, device=dev)
    last = ((cur + B - 1) % B).to(torch.int32)
    m1 = torch.full((B, St), -7, dtype=torch.int32, device=dev)
    nm1 = torch.zeros(B, dtype=torch.int32, device=dev)
    m2 = torch.full((B, St), -7, dtype=torch.int32, device=dev)
    nm2, ntm2 = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    inview = torch.zeros((B, B * St), dtype=torch.uint8, device=dev)
    # ---- the chain: device work only ----
    pp.extract(imgs)
    pos = pp.unproject(tposes, mp_flags=flags)
    pp.track_pairs(cur, last, pos, flags, tposes, 15.0, False, True, m1, nm1)
    work = tposes.clone()
    r1 = pp.optimize_pose(work, pos, pairs=(m1, last), frame_mp=True)
    frame_mp = r1["frame_mp"]
    keep1 = r1  # every call returns buffers of its own
    table_pos = pos.view(-1, 3)
    R = work[:, :3, :3]
    Ow = -(R.transpose(1, 2) @ work[:, :3, 3:4]).squeeze(2)  # fabricated observations: a normal towards each frame
    nrm = torch.nn.functional.normalize(pos - Ow.view(B, 1, 3), dim=2).view(-1, 3).contiguous()
    mind = torch.full((B * St,), 0.05, dtype=torch.float32, device=dev)
    maxd = torch.full((B * St,), 500.0, dtype=torch.float32, device=dev)
    tflags = torch.where(flags.view(-1) == 0, torch.full_like(flags.view(-1), 2), flags.view(-1))  # no point: bad
    pp.track_local(work, table_pos, nrm, mind, maxd, pp.desc[:B].view(-1, 32), tflags, frame_mp, 3.0, m2, nm2, ntm2,
                   in_view=inview)
    merged = torch.where(m2 >= 0, m2, frame_mp)
    poses1 = work.clone()
    r2 = pp.optimize_pose(work, pos, local=merged)
    torch.cuda.synchronize()
    pp.check_error()
    pp.check_match_error()
    # ---- the reference side, from the arrays read back ----
    g = pp.track_geom()
    inv = pp.inv_level_sigma2()
    hpos, hflags = pos.cpu().numpy().reshape(-1, 3), tflags.cpu().numpy()
    hm1, hlast = m1.cpu().numpy(), last.cpu().numpy()
    frames = []
    for f in range(B):
        k = pp.host_keypoints_un(f)
        _, d = pp.host_keypoints(f)
        ur, _, ns = pp.host_stereo(f)
        assert ns > 30
        frames.append((k, d, ur))
    k1 = dict((k, v.cpu().numpy()) for k, v in keep1.items())
    hfmp, hposes1 = frame_mp.cpu().numpy(), poses1.cpu().numpy()
    nin = []
    for f in range(B):
        k, _, ur = frames[f]
        n = len(k)
        mp = np.where(hm1[f, :n] >= 0, hlast[f] * St + hm1[f, :n], -1).astype(np.int32)
        assert np.array_equal(k1["mp_index"][f, :n], mp) and (mp >= 0).sum() == int(nm1.cpu()[f])
        ref = pose_optimization(g, inv, poses[f], k, ur, mp, hpos)
        assert k1["status"][f] == ref.status and hposes1[f].tobytes() == ref.Tcw.tobytes(), f
        assert np.array_equal(k1["outlier"][f, :n][mp >= 0], ref.outlier[mp >= 0]) and k1["ninliers"][f] == ref.ninliers
        assert np.array_equal(hfmp[f, :n], np.where(ref.outlier == 1, -1, mp))
        assert k1["nmatches_map"][f] == int(((mp >= 0) & (ref.outlier == 0)).sum())
        nin.append(ref.ninliers)
    bnd, gw, gh = image_bounds(cam.astuple(), W, H)
    G = FP.Geom(cam.fx, cam.fy, cam.cx, cam.cy, rig[0], bnd, b=rig[1])
    G.scale_factors = np.asarray(pp.scale, f32)
    G.grid_w_inv, G.grid_h_inv = gw, gh
    table = Table(hpos, nrm.cpu().numpy(), mind.cpu().numpy(), maxd.cpu().numpy(),
                  pp.desc[:B].cpu().numpy().reshape(-1, 32), hflags)
    got = (m2.cpu().numpy(), nm2.cpu().numpy(), ntm2.cpu().numpy(), inview.cpu().numpy())
    ex = Expect(G)
    hm2, h2 = got[0], dict((k, v.cpu().numpy()) for k, v in r2.items() if v is not None)
    found = []
    for f in range(B):
        k, d, ur = frames[f]
        fr = Frame(k, d, hposes1[f], ur)
        ref = ex.frame(f, fr, table, 0, B * St, hfmp[f], 3.0, True)
        found.append(same_frame(got, f, fr.n, ref, "chain frame %d" % f))
        n = fr.n
        mp = np.where(hm2[f, :n] >= 0, hm2[f, :n], hfmp[f, :n]).astype(np.int32)
        ref = pose_optimization(g, inv, hposes1[f], k, ur, mp, hpos)
        assert h2["poses"][f].tobytes() == ref.Tcw.tobytes() and h2["status"][f] == ref.status, f
        assert np.array_equal(h2["outlier"][f, :n][mp >= 0], ref.outlier[mp >= 0]) and h2["ninliers"][f] == ref.ninliers
    assert max(nin) >= 10 and int(h2["ninliers"].max()) >= 10
    print("inliers after the first optimisation", nin, "local matches", found, "inliers after the second",
          h2["ninliers"].tolist())
    pp.close()

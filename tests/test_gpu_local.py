"""GPU: local-map tracking on a device batch. The device logf against the host's, Frame::isInFrustum on the device
against the host unit, bit for bit, and orbm_search_local_points_batch_device (Tracking::SearchLocalPoints) against the
CPU oracle (oracle_py.search_by_projection_local fed the Python restatement's isInFrustum fields, never the per-call GPU
entry): the whole d_match rows, d_nmatches and d_ntomatch of every frame. Inputs are built by hand on the device with
torch, except in the chain test, which extracts."""
import ctypes as C

import numpy as np
import pytest

import frustum_py as FP
import oracle_py
import orbamd
import proj_scenes as ps
import undistort_py as U
from orbamd.frame import is_in_frustum

pytestmark = pytest.mark.gpu

EDEVICE = -2
f32 = np.float32


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


def stream_of(torch):
    return torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream


def take_error(torch, ctx):
    return orbamd.load().orbm_check_error(ctx, stream_of(torch))


def uploader(torch):
    dev = torch.device("cuda", 0)
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ logf
def test_device_logf_equals_host_libm(torch):
    """orbx_selftest_logf on the directed ratios of the boundary rows (1.0f, the powers of 1.2f, one ulp either side),
    the ends of the domain and 2^20 random positive normal floats, bit for bit; outside the domain the hook gives NaN"""
    r = [f32(1.0), FP.up(1.0), FP.down(1.0), np.finfo(f32).tiny, np.finfo(f32).max]
    for v in FP.scale_ratios():
        r += [v, FP.up(v), FP.down(v)]
    rng = np.random.default_rng(12)
    rnd = rng.integers(0x00800000, 0x7f800000, 1 << 20, dtype=np.int64).astype(np.uint32).view(f32)
    x = np.concatenate([np.array(r, f32), rnd])
    libm = C.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = C.c_float, [C.c_float]
    want = np.array([libm.logf(float(v)) for v in x], f32)
    outside = np.array([0.0, -0.0, -1.0, np.inf, np.nan, 1e-40], f32)
    up = uploader(torch)
    dx = up(np.concatenate([x, outside]))
    dy = torch.full_like(dx, 7.0)
    assert orbamd.load().orbx_selftest_logf(dx.data_ptr(), dy.data_ptr(), dx.numel(), stream_of(torch)) == 0
    torch.cuda.synchronize()
    y = dy.cpu().numpy()
    bad = np.nonzero(y[:len(x)].view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (x[bad[:8]], y[bad[:8]], want[bad[:8]])
    assert np.isnan(y[len(x):]).all()


# ------------------------------------------------------------------------------------------------ isInFrustum
def frustum_device(torch, ctx, g, poses, cloud, limit=0.5):
    up = uploader(torch)
    pos, nrm, mind, maxd = cloud
    M, nf = len(pos), len(poses)
    t = [up(pos), up(nrm), up(mind), up(maxd), up(np.stack(poses).astype(f32))]
    outs = [torch.full((nf, M), 9, dtype=dt, device=t[0].device)
            for dt in (torch.uint8, torch.float32, torch.float32, torch.float32, torch.int32, torch.float32)]
    cg = g.cstruct()
    rc = orbamd.load().orbx_is_in_frustum_batch_device(
        ctx, C.byref(cg), float(g.log_scale_factor), limit, M, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
        t[3].data_ptr(), nf, t[4].data_ptr(), *[o.data_ptr() for o in outs], stream_of(torch))
    assert rc == 0
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def same_bits(a, b):
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))
    return np.array_equal(a, b)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_frustum_device_equals_host_bitwise(torch, ctx, M):
    """wave and workgroup edges, three frames (the identity, a small and a large rotation) in one launch"""
    g = FP.camera_geom("my")
    poses = FP.poses()
    cloud = FP.cloud(g, poses[1], 257, 7)
    cloud = tuple(a[257 - M:] for a in cloud)  # M = 1: the last point
    got = frustum_device(torch, ctx, g, poses, cloud)
    nin = 0
    for f, T in enumerate(poses):
        ref = is_in_frustum(g.cstruct(), g.log_scale_factor, T, *cloud)
        for a, b in zip(got, ref):
            assert same_bits(a[f], b), (M, f)
        nin += int(ref[0].sum())
    assert M < 63 or nin > M // 4
    assert take_error(torch, ctx) == 0


def test_frustum_device_directed_rows_and_error_flag(torch, ctx):
    """the boundary rows under the identity pose as one table: equal to the host unit bit for bit; the rows the
    contract excludes raise the ctx's error flag, the same table without them does not"""
    g = FP.EXACT
    rows = [r for r in FP.directed_rows() if r[1] is FP.IDENTITY]
    assert len(rows) > 80

    def table(rs):
        return (np.array([r[2] for r in rs], f32), np.array([r[3] for r in rs], f32), np.array([r[4] for r in rs], f32),
                np.array([r[5] for r in rs], f32))
    clean = [r for r in rows if r[6] != FP.EXCLUDED]
    assert take_error(torch, ctx) == 0
    for rs, err in ((clean, 0), (rows, EDEVICE)):
        cloud = table(rs)
        got = frustum_device(torch, ctx, g, [FP.IDENTITY], cloud)
        ref = is_in_frustum(g.cstruct(), g.log_scale_factor, FP.IDENTITY, *cloud)
        for a, b in zip(got, ref):
            assert same_bits(a[0], b)
        assert take_error(torch, ctx) == err
        assert take_error(torch, ctx) == 0
    assert 0 < int(ref[0].sum()) < len(rows)


def test_frustum_device_empty_is_a_no_op(torch, ctx):
    g = FP.EXACT.cstruct()
    fn = orbamd.load().orbx_is_in_frustum_batch_device
    assert fn(ctx, C.byref(g), 0.18, 0.5, 0, *([None] * 4), 3, *([None] * 7), None) == 0
    assert fn(ctx, C.byref(g), 0.18, 0.5, 5, *([None] * 4), 0, *([None] * 7), None) == 0


# ------------------------------------------------------------------------------------------------ SearchLocalPoints
class Frame:
    def __init__(self, kps, desc, Tcw, uright=None):
        self.n = len(kps)
        self.kps = np.zeros(self.n, orbamd.kp_dtype)
        for k in ("x", "y", "octave", "angle"):
            self.kps[k] = kps[k]
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(self.n, 32)
        self.Tcw = np.ascontiguousarray(Tcw, f32).reshape(4, 4)
        self.uright = uright  # None: a monocular frame


class Table:
    """the local map: pos / normal [M, 3], min_dist / max_dist [M], desc [M, 32], flags [M] (bit 1 bad, bit 3 obs)"""

    def __init__(self, pos, normal, mind, maxd, desc, flags):
        self.M = len(pos)
        self.pos = np.ascontiguousarray(pos, f32).reshape(self.M, 3)
        self.normal = np.ascontiguousarray(normal, f32).reshape(self.M, 3)
        self.mind, self.maxd = np.ascontiguousarray(mind, f32), np.ascontiguousarray(maxd, f32)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(self.M, 32)
        self.flags = np.ascontiguousarray(flags, np.uint8)


def scene_geom(scale):
    g = FP.Geom(ps.FX, ps.FY, ps.CX, ps.CY, 47.9, (0, ps.W, 0, ps.H))
    assert np.array_equal(g.scale_factors, np.asarray(scale, f32))
    return g


def build_scene(stereo=True, nframes=4, per_frame=250):
    """four frames built like test_gpu_track.full_frame (real keypoints, a pose within a degree of the identity) and a
    table of MapPoints back-projected from each frame's own keypoints under its own pose, so that every frame finds
    its own and its neighbours' points; then points placed to be rejected by each test of isInFrustum. Every frame
    holds part of its own points already (frame_mp): those are seen."""
    frames, parts, frame_src = [], [], []
    G = None
    for s in range(nframes):
        rng = np.random.default_rng(2000 + s)
        F, k, d, scale = ps.make_frame(rng, 2, 40 + s, stereo)
        G = scene_geom(scale) if G is None else G
        Tcw = ps.pose(ps.rot(rng, 1.0), rng.normal(0, 0.02, 3))
        frames.append(Frame(k, d, Tcw, F.uright))
        src = rng.choice(F.n, per_frame, replace=False)
        Xw = ps.backproject(rng, k, src, Tcw) + rng.normal(0, 0.003, (per_frame, 3)).astype(f32)
        mind, maxd = ps.dist_bounds(rng, Xw, Tcw, k["octave"][src])
        R, t = Tcw[:3, :3].astype(np.float64), Tcw[:3, 3].astype(np.float64)
        nrm = Xw - (-(R.T @ t))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm[rng.random(per_frame) < 0.05] *= -1
        parts.append((Xw, nrm, mind, maxd, ps.flip_bits(rng, d[src], 30)))
        frame_src.append(src)
    # placed rejections, in the camera frame of frame 0 (every pose is within a degree and 6 cm of it): behind the
    # camera, 150+ pixels left / right of the image, above / below it
    rng = np.random.default_rng(77)
    ne = 60
    u = np.concatenate([rng.uniform(50, 590, 20), rng.choice([-200.0, 840.0], 20), rng.uniform(50, 590, 20)])
    v = np.concatenate([rng.uniform(50, 430, 40), rng.choice([-160.0, 640.0], 20)])
    z = np.concatenate([rng.uniform(-8, -1, 20), rng.uniform(2, 8, 40)])
    xc = np.stack([(u - ps.CX) / ps.FX * z, (v - ps.CY) / ps.FY * z, z], 1)
    T0 = frames[0].Tcw.astype(np.float64)
    Xe = ((xc - T0[:3, 3]) @ T0[:3, :3]).astype(f32)
    ne_n = Xe / np.linalg.norm(Xe, axis=1, keepdims=True)
    de = np.linalg.norm(Xe, axis=1)
    parts.append((Xe, ne_n, (de / 3).astype(f32), (de * 2).astype(f32), rng.integers(0, 256, (ne, 32), dtype=np.uint8)))
    pos, nrm, mind, maxd, desc = (np.concatenate([p[i] for p in parts]) for i in range(5))
    M = len(pos)
    fl = rng.random((2, M))
    flags = ((fl[0] < 0.06) * 2 | (fl[1] < 0.85) * 8).astype(np.uint8)
    table = Table(pos, nrm, mind, maxd, desc, flags)
    frame_mp = []
    for s, fr in enumerate(frames):
        rng = np.random.default_rng(3000 + s)
        row = np.full(fr.n, -1, np.int32)
        hold = rng.random(per_frame) < 0.4  # the frame already holds these of its own points
        row[frame_src[s][hold]] = (s * per_frame + np.arange(per_frame))[hold]
        free = np.nonzero(row < 0)[0]
        other = rng.choice(free, 20, replace=False)  # and a few points of the other frames
        row[other] = rng.choice(np.setdiff1d(np.arange(M), np.arange(s * per_frame, (s + 1) * per_frame)), 20)
        frame_mp.append(row)
    return frames, table, frame_mp, G


class Expect:
    """what the reference gives for one frame over a slice of the table: the restatement's isInFrustum fields (computed
    once per frame and slice), then the CPU oracle's SearchByProjection(F, vpMapPoints, th)"""

    def __init__(self, G):
        self.G = G
        self.fields = {}

    def frustum(self, key, fr, table, begin, end):
        k = (key, begin, end)
        if k not in self.fields:
            sl = slice(begin, end)
            self.fields[k] = FP.is_in_frustum(self.G, fr.Tcw, 0.5, table.pos[sl], table.normal[sl], table.mind[sl],
                                              table.maxd[sl])
        return self.fields[k]

    def frame(self, key, fr, table, begin, end, fmp, th, stereo, nnratio=0.8):
        """(nmatches, match row [n] of table indices, ntomatch, in_view [M], why [end - begin] of the points that went
        through isInFrustum, -1 for the others)"""
        G, M = self.G, table.M
        fmp = np.asarray(fmp[:fr.n])
        valid = (fmp >= 0) & (fmp < M)
        idx = np.where(valid, fmp, 0)
        holds = valid & ((table.flags[idx] & 2) == 0)  # a bad MapPoint counts as none (Tracking.cc:1151-1154)
        seen = np.zeros(M, bool)
        seen[fmp[holds]] = True
        occ = holds & ((table.flags[idx] & 8) != 0)
        sl = slice(begin, end)
        bad = (table.flags[sl] & 2) != 0
        tested = ~seen[sl] & ~bad
        fld = self.frustum(key, fr, table, begin, end)
        in_view = (fld.in_view != 0) & tested
        mps = orbamd.MapPoints(end - begin, desc=table.desc[sl], bad=bad, has_obs=(table.flags[sl] & 8) != 0,
                               track_in_view=in_view, track_proj_x=fld.proj_x, track_proj_y=fld.proj_y,
                               track_proj_xr=fld.proj_xr, track_level=fld.level, track_view_cos=fld.view_cos)
        F = orbamd.FrameView(fr.kps, fr.desc, G.scale_factors, ps.W, ps.H, G.fx, G.fy, G.cx, G.cy, bf=G.bf,
                             uright=fr.uright if stereo else None, occupied=occ.astype(np.uint8))
        for k in ("min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv", "b"):
            setattr(F, k, getattr(G, k))
        nm, m = oracle_py.search_by_projection_local(F, mps, th, nnratio)
        full = np.zeros(M, np.uint8)
        full[sl] = in_view
        return nm, np.where(m >= 0, m + begin, m), int(in_view.sum()), full, np.where(tested, fld.why, -1)


def launch_local(torch, ctx, frames, table, frame_mp, G, th, stereo=True, ranges=None, S=None, counts=None,
                 nnratio=0.8, with_in_view=True):
    """one orbm_search_local_points_batch_device launch over hand-built device arrays: (match [nf, S], nmatches [nf],
    ntomatch [nf], in_view [nf, M]) as numpy, every output pre-filled with a sentinel"""
    nf, M = len(frames), table.M
    S = max([fr.n for fr in frames] + [1]) if S is None else S
    K = np.zeros((nf, S), orbamd.kp_dtype)
    D = np.zeros((nf, S, 32), np.uint8)
    UR = np.full((nf, S), -1, f32)
    FM = np.full((nf, S), -1, np.int32)
    T = np.zeros((nf, 4, 4), f32)
    for f, fr in enumerate(frames):
        n = fr.n
        K[f, :n], D[f, :n], T[f] = fr.kps, fr.desc, fr.Tcw
        if fr.uright is not None:
            UR[f, :n] = fr.uright
        FM[f, :len(frame_mp[f])] = frame_mp[f]
    cnt = np.array([fr.n for fr in frames] if counts is None else counts, np.int32)
    up = uploader(torch)
    dev = torch.device("cuda", 0)
    t = dict(k=up(K.view(f32).reshape(nf, S, 6)), d=up(D), ur=up(UR), fm=up(FM), T=up(T), cnt=up(cnt),
             pos=up(table.pos.reshape(-1)), nrm=up(table.normal.reshape(-1)), mind=up(table.mind), maxd=up(table.maxd),
             md=up(table.desc.reshape(-1)), fl=up(table.flags))
    if ranges is not None:
        t["rng"] = up(np.asarray(ranges, np.int32).reshape(nf, 2))
    out = torch.full((nf, S), -7, dtype=torch.int32, device=dev)
    nm = torch.full((nf,), -7, dtype=torch.int32, device=dev)
    ntm = torch.full((nf,), -7, dtype=torch.int32, device=dev)
    inv = torch.full((nf, max(M, 1)), 5, dtype=torch.uint8, device=dev)
    g = G.cstruct()
    p = lambda key: t[key].data_ptr() if t[key].numel() else None  # noqa: E731
    rc = orbamd.load().orbm_search_local_points_batch_device(
        ctx, nf, p("k"), p("d"), p("cnt"), S, p("ur") if stereo else None, p("T"), C.byref(g),
        float(G.log_scale_factor), M, p("pos"), p("nrm"), p("mind"), p("maxd"), p("md"), p("fl"),
        t["rng"].data_ptr() if ranges is not None else None, p("fm"), float(th), float(nnratio), 0.5, out.data_ptr(),
        nm.data_ptr(), ntm.data_ptr(), inv.data_ptr() if with_in_view else None, stream_of(torch))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), nm.cpu().numpy(), ntm.cpu().numpy(), inv.cpu().numpy()[:, :M]


def same_frame(got, f, n, ref, what):
    out, nm, ntm, inv = got
    no, mo, nto, ivo = ref[:4]
    bad = np.nonzero(out[f, :n] != mo)[0]
    assert bad.size == 0, "%s: rows %s: gpu %s oracle %s" % (what, bad[:8], out[f, bad[:8]], mo[bad[:8]])
    assert int(nm[f]) == no, "%s: nmatches %d, oracle %d" % (what, int(nm[f]), no)
    assert int(ntm[f]) == nto, "%s: ntomatch %d, restatement %d" % (what, int(ntm[f]), nto)
    assert (out[f, n:] == -7).all(), "%s: rows past the frame's count were written" % what
    assert np.array_equal(inv[f], ivo), "%s: in_view differs" % what
    return no


@pytest.fixture(scope="module")
def scene():
    frames, table, frame_mp, G = build_scene()
    return frames, table, frame_mp, G, Expect(G)


def test_scene_is_not_vacuous(scene):
    """asserted from the CPU restatement and oracle alone: every frame has each of the five rejection reasons, a seen
    and a bad point, a quarter of the table in view and 50 matches"""
    frames, table, frame_mp, G, ex = scene
    for f, fr in enumerate(frames):
        for th in (1.0, 3.0, 5.0):
            nm, m, nto, inv, why = ex.frame(f, fr, table, 0, table.M, frame_mp[f], th, True)
            assert nm >= 50 and nto >= table.M // 4, (f, th, nm, nto)
        for r in FP.REJECTIONS:
            assert (why == r).any(), (f, r)
        assert not (why == FP.EXCLUDED).any()
        fm = frame_mp[f]
        held = fm[fm >= 0]
        assert ((table.flags[held] & 2) == 0).any() and ((table.flags[held] & 2) != 0).any()
        assert (table.flags & 2).any() and ((why == -1).sum() > 50)
        assert ((table.flags[held] & 8) != 0).any() and ((table.flags[held] & 8) == 0).any()
        assert len(set(m[m >= 0] // 250)) >= 3  # matches to its own points and to the other frames'


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("th", [1.0, 3.0, 5.0])
def test_four_frames_in_one_launch(torch, ctx, scene, th, stereo):
    frames, table, frame_mp, G, ex = scene
    got = launch_local(torch, ctx, frames, table, frame_mp, G, th, stereo)
    for f, fr in enumerate(frames):
        ref = ex.frame(f, fr, table, 0, table.M, frame_mp[f], th, stereo)
        assert same_frame(got, f, fr.n, ref, "th %g stereo %d frame %d" % (th, stereo, f)) >= 50
    assert take_error(torch, ctx) == 0


def test_stereo_and_mono_differ(scene):
    """the mvuRight test takes part: the oracle's rows with and without d_uright are not the same"""
    frames, table, frame_mp, G, ex = scene
    a = ex.frame(0, frames[0], table, 0, table.M, frame_mp[0], 3.0, True)
    b = ex.frame(0, frames[0], table, 0, table.M, frame_mp[0], 3.0, False)
    assert not np.array_equal(a[1], b[1])


def test_two_slices_of_one_table_equal_two_launches(torch, ctx, scene):
    """frames 0, 1 take the first half of the table and frames 2, 3 the second: one launch with d_range equals the
    oracle on each slice and two separate launches over the two half tables"""
    frames, table, frame_mp, G, ex = scene
    M, h = table.M, table.M // 2 + 3  # an odd split
    ranges = [(0, h), (0, h), (h, M), (h, M)]
    # every feature holds a point of its frame's slice or none, so that the half tables can say the same
    fmp = [np.where((r >= ranges[f][0]) & (r < ranges[f][1]), r, -1) for f, r in enumerate(frame_mp)]
    got = launch_local(torch, ctx, frames, table, fmp, G, 3.0, True, ranges=ranges)
    nms = []
    for f, fr in enumerate(frames):
        ref = ex.frame(("half", f), fr, table, ranges[f][0], ranges[f][1], fmp[f], 3.0, True)
        nms.append(same_frame(got, f, fr.n, ref, "slice of frame %d" % f))
        assert (fmp[f] >= 0).sum() > 20
    assert min(nms) > 20
    for lo, hi, fs in ((0, h, (0, 1)), (h, M, (2, 3))):
        sub = Table(table.pos[lo:hi], table.normal[lo:hi], table.mind[lo:hi], table.maxd[lo:hi], table.desc[lo:hi],
                    table.flags[lo:hi])
        part = launch_local(torch, ctx, [frames[f] for f in fs], sub, [np.where(fmp[f] >= 0, fmp[f] - lo, -1) for f in fs],
                            G, 3.0, True)
        for j, f in enumerate(fs):
            n = frames[f].n
            assert np.array_equal(np.where(part[0][j, :n] >= 0, part[0][j, :n] + lo, part[0][j, :n]), got[0][f, :n])
            assert part[1][j] == got[1][f] and part[2][j] == got[2][f]
            assert np.array_equal(part[3][j], got[3][f, lo:hi]) and not got[3][f, :lo].any() and not got[3][f, hi:].any()
    assert take_error(torch, ctx) == 0


def test_degenerate_shapes(torch, ctx, scene):
    """an empty table; a frame with count 0 and a frame whose every point is seen (ntomatch = 0) beside a normal one;
    rows past a frame's count keep the sentinel; nframes = 0"""
    frames, table, frame_mp, G, ex = scene
    empty = Table(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), np.zeros((0, 32)), np.zeros(0))
    out, nm, ntm, inv = launch_local(torch, ctx, frames[:2], empty, [np.full(fr.n, -1, np.int32) for fr in frames[:2]],
                                     G, 3.0)
    for f in range(2):
        assert nm[f] == 0 and ntm[f] == 0 and (out[f, :frames[f].n] == -1).all() and (out[f, frames[f].n:] == -7).all()
    # frame 1 sees all of a 200-point table: its features 0..199 hold points 0..199, none of them bad
    small = Table(table.pos[:200], table.normal[:200], table.mind[:200], table.maxd[:200], table.desc[:200],
                  table.flags[:200] & ~np.uint8(2))
    nobody = Frame(np.zeros(0, orbamd.kp_dtype), np.zeros((0, 32), np.uint8), np.eye(4), np.zeros(0, f32))
    fs = [frames[0], frames[1], nobody]
    fm = [np.full(frames[0].n, -1, np.int32), np.full(frames[1].n, -1, np.int32), np.zeros(0, np.int32)]
    fm[1][:200] = np.arange(200)
    S = max(fr.n for fr in fs) + 9
    got = launch_local(torch, ctx, fs, small, fm, G, 3.0, S=S)
    refs = [ex.frame(("small", f), fr, small, 0, 200, fm[f], 3.0, True) for f, fr in enumerate(fs)]
    n0 = same_frame(got, 0, fs[0].n, refs[0], "normal frame")
    assert n0 > 20 and refs[0][2] > 50
    assert same_frame(got, 1, fs[1].n, refs[1], "all seen") == 0 and refs[1][2] == 0
    assert same_frame(got, 2, 0, refs[2], "count 0") == 0 and refs[2][2] > 50  # in view, nothing to match them to
    assert launch_local(torch, ctx, [], small, [], G, 3.0)[0].shape[0] == 0
    assert take_error(torch, ctx) == 0


def test_malformed_input_raises_the_flag_and_leaves_the_rest(torch, ctx, scene):
    """run once: a d_frame_mp index >= M (treated as none), a d_range with begin > end and one past M (those frames
    blanked), a count above kp_stride (clamped); the frames beside them equal the oracle"""
    frames, table, frame_mp, G, ex = scene
    M = table.M
    S = max(fr.n for fr in frames)
    big = int(np.argmax([fr.n for fr in frames]))  # fills kp_stride: its count is overstated below
    r1, r2, ix = [f for f in range(4) if f != big]
    fm = [r.copy() for r in frame_mp]
    j = int(np.nonzero(fm[ix] >= 0)[0][0])
    fm[ix][j] = M  # out of range
    ranges = [(0, M)] * 4
    ranges[r1], ranges[r2] = (5, 2), (0, M + 1)
    counts = [fr.n for fr in frames]
    counts[big] = S + 5
    assert take_error(torch, ctx) == 0
    got = launch_local(torch, ctx, frames, table, fm, G, 3.0, ranges=ranges, S=S, counts=counts)
    assert take_error(torch, ctx) == EDEVICE
    assert take_error(torch, ctx) == 0
    out, nm, ntm, inv = got
    for f in (r1, r2):
        assert nm[f] == 0 and ntm[f] == 0 and (out[f] == -1).all() and not inv[f].any(), f
    for f in (ix, big):
        row = np.where(fm[f] >= M, -1, fm[f])
        ref = ex.frame(("mal", f), frames[f], table, 0, M, row, 3.0, True)
        n = frames[f].n
        assert np.array_equal(out[f, :n], ref[1]) and nm[f] == ref[0] > 50 and ntm[f] == ref[2], f
        assert np.array_equal(inv[f], ref[3])
    # a bad index alone raises the flag too
    launch_local(torch, ctx, [frames[ix]], table, [fm[ix]], G, 3.0)
    assert take_error(torch, ctx) == EDEVICE


def test_contract_excluded_points_raise_the_flag(torch, ctx, scene):
    """a NaN position and an infinite max_dist in the table: those points are rejected, the flag is raised, and the
    frame's result is the oracle's with those points out of view"""
    frames, table, frame_mp, G, ex = scene
    t = Table(table.pos.copy(), table.normal, table.mind, table.maxd.copy(), table.desc, table.flags & ~np.uint8(2))
    fm = [np.full(frames[0].n, -1, np.int32)]
    ok = ex.frame(("nan0",), frames[0], t, 0, t.M, fm[0], 3.0, True)
    a, b = np.nonzero(ok[3])[0][[3, 40]]
    t.pos[a, 1] = np.nan
    t.maxd[b] = np.inf
    ref = ex.frame(("nan1",), frames[0], t, 0, t.M, fm[0], 3.0, True)
    assert ref[2] == ok[2] - 2 and ref[4][a] == FP.EXCLUDED and ref[4][b] == FP.EXCLUDED
    got = launch_local(torch, ctx, frames[:1], t, fm, G, 3.0)
    same_frame(got, 0, frames[0].n, ref, "excluded points")
    assert take_error(torch, ctx) == EDEVICE


# ------------------------------------------------------------------------------------------------ the chain
def test_extract_to_track_local_chain(torch):
    """a 3-frame stereo batch at 640x480: extraction, UndistortKeyPoints, ComputeStereoMatches, UnprojectStereo,
    SearchByProjection(frame f + 1, frame f) and SearchLocalPoints on one stream with no host step between them. The
    local map is the table of every frame's unprojected keypoints (index f * stride + i; normals, distance bounds and
    the features' MapPoints derived from the device arrays by elementwise torch glue); frame f's slice is the points of
    frames f - 1 and f. Read back afterwards, the result equals the oracle fed the same intermediate arrays."""
    from orbamd.device import STEREO_RIGS, BatchPipeline
    from orbamd.frame import image_bounds
    W, H, B = 640, 480, 3
    cam = U.MY_YAML[0]
    rig = STEREO_RIGS["euroc"]
    pp = BatchPipeline(torch, W, H, B, nfeatures=500, stereo=rig, camera=cam.astuple())
    S = pp.stride
    left = orbamd.synth_frames(1, 5, B, W, H)
    right = orbamd.synth_frames(1, 5, B, W, H, dx=8)
    imgs = torch.from_numpy(np.concatenate([left, right])).to(pp.dev)
    rng = np.random.default_rng(3)
    poses = np.stack([ps.pose(ps.rot(rng, 0.2), rng.normal(0, 0.01, 3)) for _ in range(B)]).astype(f32)
    tposes = torch.from_numpy(poses).to(pp.dev)
    R = tposes[:, :3, :3].double()
    Ow = (-(R.transpose(1, 2) @ tposes[:, :3, 3:].double())).float().reshape(B, 1, 3)  # glue: only the normals use it
    flags = torch.zeros((B, S), dtype=torch.uint8, device=pp.dev)
    cur = torch.arange(1, B, dtype=torch.int32, device=pp.dev)
    last = torch.arange(0, B - 1, dtype=torch.int32, device=pp.dev)
    pairs = torch.full((B - 1, S), -7, dtype=torch.int32, device=pp.dev)
    npairs = torch.zeros(B - 1, dtype=torch.int32, device=pp.dev)
    out = torch.full((B, S), -7, dtype=torch.int32, device=pp.dev)
    nm = torch.zeros(B, dtype=torch.int32, device=pp.dev)
    ntm = torch.zeros(B, dtype=torch.int32, device=pp.dev)
    inv = torch.zeros((B, B * S), dtype=torch.uint8, device=pp.dev)
    ranges = torch.tensor([[max(f - 1, 0) * S, (f + 1) * S] for f in range(B)], dtype=torch.int32, device=pp.dev)
    scale = torch.from_numpy(np.asarray(pp.scale, f32)).to(pp.dev)
    pp.extract(imgs)  # extraction, undistortion and stereo matching
    pos = pp.unproject(tposes, mp_flags=flags)
    pp.track_pairs(cur, last, pos, flags, tposes, 15.0, False, True, pairs, npairs)
    # the table, all on the device: a keypoint without depth is a bad entry
    po = pos - Ow
    dist = po.norm(dim=2)
    normal = (po / dist.clamp_min(1e-12).unsqueeze(2)).contiguous()
    octave = pp.kps_un[:B, :, 5].contiguous().view(torch.int32).clamp(0, 7).long()
    maxd = (dist * scale[octave]).contiguous()
    mind = (maxd / scale[7]).contiguous()
    tflags = torch.where(flags == 0, torch.full_like(flags, 2), flags).contiguous()
    frame_mp = torch.full((B, S), -1, dtype=torch.int32, device=pp.dev)
    base = (torch.arange(0, B - 1, dtype=torch.int32, device=pp.dev) * S).unsqueeze(1)
    frame_mp[1:] = torch.where(pairs >= 0, pairs + base, torch.full_like(pairs, -1))
    pp.track_local(tposes, pos.view(-1, 3), normal.view(-1, 3), mind.view(-1), maxd.view(-1),
                   pp.desc[:B].reshape(-1, 32), tflags.view(-1), frame_mp, 3.0, out, nm, ntm, ranges=ranges,
                   in_view=inv)
    torch.cuda.synchronize()
    pp.check_error()
    pp.check_match_error()
    b, gw, gh = image_bounds(cam.astuple(), W, H)
    G = FP.Geom(cam.fx, cam.fy, cam.cx, cam.cy, rig[0], b, b=rig[1])
    G.scale_factors = np.asarray(pp.scale, f32)
    G.grid_w_inv, G.grid_h_inv = gw, gh
    assert G.log_scale_factor == f32(pp.log_scale_factor())
    table = Table(pos.cpu().numpy().reshape(-1, 3), normal.cpu().numpy().reshape(-1, 3), mind.cpu().numpy().reshape(-1),
                  maxd.cpu().numpy().reshape(-1), pp.desc[:B].cpu().numpy().reshape(-1, 32),
                  tflags.cpu().numpy().reshape(-1))
    fmp = frame_mp.cpu().numpy()
    got = (out.cpu().numpy(), nm.cpu().numpy(), ntm.cpu().numpy(), inv.cpu().numpy())
    rg = ranges.cpu().numpy()
    ex = Expect(G)
    total = []
    for f in range(B):
        k = pp.host_keypoints_un(f)
        _, d = pp.host_keypoints(f)
        ur, _, ns = pp.host_stereo(f)
        fr = Frame(k, d, poses[f], ur)
        ref = ex.frame(f, fr, table, int(rg[f, 0]), int(rg[f, 1]), fmp[f], 3.0, True)
        total.append(same_frame(got, f, fr.n, ref, "chain frame %d" % f))
        assert ns > 30 and ref[2] > 30
    assert (fmp[1:] >= 0).sum() > 50 and max(total) > 0
    pp.close()

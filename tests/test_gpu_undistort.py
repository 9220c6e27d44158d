"""GPU: Frame::UndistortKeyPoints on the device (orbx_undistort_batch_device, csrc/undistort_kernels.hip) against the
pure-Python restatement tests/undistort_py.py as raw bits, its composition with the batch extractor, the batch
matcher and the keyframe slot, and the schedule with a distorted camera (BatchPipeline / AgentSchedule camera=...)
against the oracle fed the restated mvKeysUn."""
import ctypes as C

import numpy as np
import pytest

import oracle_py
import orbamd
import undistort_py as U
from orbamd._lib import SLOT_F_KUN
from orbamd.frame import make_camera

pytestmark = pytest.mark.gpu

STRIDE, NFRAMES = 130, 3
CAMS = dict(U.CAMERAS, k1zero=U.K1_ZERO)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ext():
    e = orbamd.ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def handmade():
    """per camera: NFRAMES x STRIDE keypoints from the test point set (corners, principal point, outside points first)
    and their restated mvKeysUn, computed once"""
    out = {}
    for name, (cam, cols, rows) in CAMS.items():
        kps = U.test_keypoints(cols, rows, cam)[:NFRAMES * STRIDE]
        assert len(kps) == NFRAMES * STRIDE
        out[name] = (cam, kps.reshape(NFRAMES, STRIDE), U.undistort_keypoints(cam, kps).reshape(NFRAMES, STRIDE))
    return out


def to_host(t):
    return t.cpu().numpy().view(np.uint8).reshape(t.shape[0], t.shape[1], 24)


@pytest.mark.parametrize("counts", [[0, 1, 130], [63, 64, 65]])
@pytest.mark.parametrize("name", sorted(CAMS))
def test_kernel_on_handmade_arrays(torch, ext, handmade, name, counts):
    cam, kps, want = handmade[name]
    sentinel = np.frombuffer(bytes([0xA5, 0x5A, 0xC3, 0x3C] * 6), np.uint8)
    src = kps.copy().view(np.uint8).reshape(NFRAMES, STRIDE, 24)
    for f, n in enumerate(counts):
        src[f, n:] = sentinel  # rows past the count are never read as keypoints
    expect = src.copy()
    wb = want.view(np.uint8).reshape(NFRAMES, STRIDE, 24)
    for f, n in enumerate(counts):
        expect[f, :n] = wb[f, :n]
    d_in = torch.from_numpy(src.copy()).cuda().view(torch.float32)
    d_cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    d_out = torch.from_numpy(np.broadcast_to(sentinel, src.shape).copy()).cuda().view(torch.float32)
    KUN_FILL = -12345.0
    d_kun = torch.full((NFRAMES, STRIDE, 2), KUN_FILL, dtype=torch.float32, device="cuda")
    ext.undistort_batch_device(cam.astuple(), d_in, d_cnt, d_out, d_kun)
    torch.cuda.synchronize()
    got = to_host(d_out)
    assert np.array_equal(to_host(d_in), src)  # the input is only read
    kun = d_kun.cpu().numpy()
    for f, n in enumerate(counts):
        assert np.array_equal(got[f, :n], expect[f, :n]), (name, f)          # xy and carried fields, raw bits
        assert np.array_equal(got[f, n:], np.broadcast_to(sentinel, got[f, n:].shape)), (name, f)  # untouched
        assert np.array_equal(kun[f, :n].view(np.uint32), got[f, :n, :8].copy().view(np.uint32).reshape(n, 2))
        assert np.all(kun[f, n:] == KUN_FILL)
    # in place, without kun
    d_io = torch.from_numpy(src.copy()).cuda().view(torch.float32)
    ext.undistort_batch_device(cam.astuple(), d_io, d_cnt, d_io)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(d_io), expect)
    assert np.array_equal(expect, src) == (name == "k1zero")  # k1 == 0: the uniform copy branch


def test_batch_entry_bad_arguments(torch, ext):
    lib = orbamd.load()
    cam = make_camera(U.MY_YAML[0].astuple())
    k = torch.zeros((1, 8, 6), dtype=torch.float32, device="cuda")
    c = torch.zeros(1, dtype=torch.int32, device="cuda")
    E = -1
    kp, cp, cm = k.data_ptr(), c.data_ptr(), C.byref(cam)

    def call(h=ext._h, cam_=cm, nf=1, kps=kp, cnt=cp, stride=8, out=kp):
        return lib.orbx_undistort_batch_device(h, cam_, nf, kps, cnt, stride, out, None, None)
    assert call(h=None) == E and call(cam_=None) == E and call(nf=-1) == E and call(kps=None) == E
    assert call(cnt=None) == E and call(stride=0) == E and call(out=None) == E
    assert call(kps=kp + 4) == E  # records are moved as 8-byte words
    assert call(nf=0) == 0 and call() == 0


W, H = 640, 480


@pytest.fixture(scope="module")
def two_frames():
    """two synthetic frames, the oracle's extraction, the restated mvKeysUn (my.yaml camera) and the oracle's
    SearchForTriangulation rows of (frame 0, frame 1) and (frame 1, frame 0) on raw and on undistorted keypoints"""
    frames = orbamd.synth_frames(0, 0, 2, W, H)
    orc = oracle_py.OracleExtractor(1000, 1.2, 8, 20, 7)
    res = [orc(f) for f in frames]
    tabs = orc.tables()
    cam = U.MY_YAML[0]
    un = [U.undistort_keypoints(cam, k) for k, _ in res]
    F12, ex, ey = orbamd.device.default_geometry()

    def rows(ks):
        v = [orbamd.KeyFrameView(k, d, tabs["scale"], tabs["sigma2"]) for k, (_, d) in zip(ks, res)]
        return [oracle_py.search_for_triangulation(v[a], v[b], F12, ex, ey, False, False)[1]
                for a, b in ((0, 1), (1, 0))]
    rows_raw, rows_un = rows([k for k, _ in res]), rows(un)
    # the camera matters to the epipolar test (ORBmatcher.cc:743-760): checked on oracle outputs alone
    assert any(not np.array_equal(a, b) for a, b in zip(rows_raw, rows_un))
    return dict(frames=frames, res=res, un=un, rows_raw=rows_raw, rows_un=rows_un, cam=cam, tabs=tabs)


def test_extract_undistort_match_pack(torch, two_frames):
    """orbx_extract_batch_device -> orbx_undistort_batch_device -> orbm_triangulation_bf_batch_device on d_kps_un,
    then orbx_pack_keyframe_device with the kernel's kun"""
    from orbamd.device import BatchPipeline
    from orbamd.exchange import kf_source, parse
    t = two_frames
    pp = BatchPipeline(torch, W, H, 2)  # buffers and the matcher ctx only: no camera, so nothing undistorts for us
    lib = orbamd.load()
    st = pp.stream_ptr()
    pp.extract(torch.from_numpy(t["frames"]).cuda())
    kps_un = torch.zeros_like(pp.kps)
    kun = torch.zeros((2, pp.stride, 2), dtype=torch.float32, device=pp.dev)
    pp.ext.undistort_batch_device(t["cam"].astuple(), pp.kps, pp.counts, kps_un, kun, st)
    F = np.ascontiguousarray(pp.F12.reshape(9))
    assert lib.orbm_triangulation_bf_batch_device(
        pp.mh, 2, pp.q1.data_ptr(), pp.q2.data_ptr(), kps_un.data_ptr(), pp.desc.data_ptr(), pp.counts.data_ptr(),
        pp.stride, F.ctypes.data, pp.ex, pp.ey, len(pp.scale), pp.scale.ctypes.data, pp.sigma2.ctypes.data, 0,
        pp.match.data_ptr(), pp.nmatch.data_ptr(), st) == 0
    slot = torch.zeros(pp.slot_bytes(), dtype=torch.uint8, device=pp.dev)
    pp.pack(0, slot, pp.meta(0), src=kf_source(pp.kps[0], pp.desc[0], pp.counts[0:1], kun=kun[0]))
    torch.cuda.synchronize()
    pp.check_error()
    for b in range(2):
        kg, dg = pp.host_keypoints(b)
        ko, do = t["res"][b]
        assert kg.tobytes() == ko.tobytes() and np.array_equal(dg, do)
        n = len(ko)
        ku = kps_un[b, :n].cpu().numpy().copy().view(np.uint8).view(orbamd.kp_dtype).reshape(n)
        assert ku.tobytes() == t["un"][b].tobytes()
        assert np.array_equal(pp.match[b, :n].cpu().numpy(), t["rows_un"][b]), b
    s = parse(slot.cpu().numpy())
    assert s["flags"] & SLOT_F_KUN
    assert s["kps"].tobytes() == t["res"][0][0].tobytes()  # mvKeys stay raw
    want = np.stack([t["un"][0]["x"], t["un"][0]["y"]], 1)
    assert np.array_equal(s["kun"].view(np.uint32), want.view(np.uint32))
    pp.close()


def test_one_frame_path(two_frames):
    """orbx_set_camera: three orbx_extract calls (eager, capturing, replayed) over two distinct frames deliver the
    camera-less handle's keypoints and descriptors and the restated mvKeysUn; camera off again: no mvKeysUn"""
    t = two_frames
    lib = orbamd.load()
    plain = orbamd.ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    camx = orbamd.ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    camx.set_camera(t["cam"].astuple())
    cap = camx.max_keypoints(W, H)
    buf = np.empty(cap, orbamd.kp_dtype)
    n = C.c_int(-7)
    for idx in (0, 1, 0):
        kp, dp = plain(t["frames"][idx])
        kc, dc = camx(t["frames"][idx])
        ko, do = t["res"][idx]
        assert kp.tobytes() == ko.tobytes() and np.array_equal(dp, do)
        assert kc.tobytes() == ko.tobytes() and np.array_equal(dc, do)
        assert camx.last_keypoints_un().tobytes() == t["un"][idx].tobytes()
        assert lib.orbx_last_keypoints_un(camx._h, buf.ctypes.data, len(ko) - 1, C.byref(n)) == -3  # ORBX_ECAPACITY
        assert lib.orbx_last_keypoints_un(plain._h, buf.ctypes.data, cap, C.byref(n)) == -1  # no camera: ORBX_EARG
    camx.set_camera(None)
    assert lib.orbx_last_keypoints_un(camx._h, buf.ctypes.data, cap, C.byref(n)) == -1
    for idx in (1, 0, 1):
        kc, dc = camx(t["frames"][idx])
        assert kc.tobytes() == t["res"][idx][0].tobytes() and np.array_equal(dc, t["res"][idx][1])
        assert lib.orbx_last_keypoints_un(camx._h, buf.ctypes.data, cap, C.byref(n)) == -1
    bad = make_camera(t["cam"].astuple())
    bad.fx = 0.0
    assert lib.orbx_set_camera(camx._h, C.byref(bad)) == -1 and lib.orbx_set_camera(None, None) == -1
    plain.close()
    camx.close()


@pytest.mark.parametrize("camera,async_x", [(True, False), (False, False), (True, True)])
def test_schedule_with_camera(torch, two_frames, camera, async_x):
    """AgentSchedule(camera=...): one graph, two frames, world 1, exchange on, one step. With the camera the match
    rows, the exchange rows, host_keypoints_un and the slot follow mvKeysUn; with camera=None they are the raw ones.
    async_x: the exchange on its own stream, from its copy of the keyframe (kun included)"""
    from orbamd.agent import KF_LEVELSUP, LOOP_NNRATIO, AgentSchedule, kf_mp_flags
    from orbamd.exchange import parse
    from check_schedule import _oracle_vocabulary
    t = two_frames
    sched = AgentSchedule(torch, t["frames"], W, H, 1, device=0, camera=t["cam"].astuple() if camera else None,
                          async_exchange=async_x)
    sched.step()
    torch.cuda.synchronize()
    sched.check_errors()
    keys = t["un"] if camera else [k for k, _ in t["res"]]
    rows = t["rows_un"] if camera else t["rows_raw"]
    for b in range(2):
        kg, dg, mg = sched.frame_results(0, b)
        ko, do = t["res"][b]
        assert kg.tobytes() == ko.tobytes() and np.array_equal(dg, do)  # mvKeys: raw either way
        assert sched.host_keypoints_un(0, b).tobytes() == keys[b].tobytes()
        assert np.array_equal(mg, rows[b]), b
    # the exchange: this agent's keyframe (frame 0) against its own slot
    tabs, voc = t["tabs"], _oracle_vocabulary(sched)
    d0 = t["res"][0][1]
    f = kf_mp_flags(len(d0))

    def view(with_fv):
        fv = voc.transform(d0, KF_LEVELSUP)[1] if with_fv else None
        return orbamd.KeyFrameView(keys[0], d0, tabs["scale"], tabs["sigma2"], feat_vec=fv,
                                   has_mp=(f & 1).astype(bool), mp_bad=((f >> 1) & 1).astype(bool))
    F12, ex, ey = orbamd.device.default_geometry()
    xm, xn, xb, xbn = sched.exchange_results()
    n_o, mo = oracle_py.search_for_triangulation(view(False), view(False), F12, ex, ey, False, False)
    assert np.array_equal(xm[0], mo) and int(xn[0]) == n_o
    nb_o, mb = oracle_py.search_by_bow(view(True), view(True), LOOP_NNRATIO, True, other_is_keyframe=True)
    assert np.array_equal(xb[0], mb) and int(xbn[0]) == nb_o and nb_o > 100
    s = parse(sched.all_slots[:sched.slot_bytes].cpu().numpy())
    assert bool(s["flags"] & SLOT_F_KUN) == camera
    assert s["kps"].tobytes() == t["res"][0][0].tobytes()
    assert np.array_equal(s["kun"].view(np.uint32), np.stack([keys[0]["x"], keys[0]["y"]], 1).view(np.uint32))
    sched.close()

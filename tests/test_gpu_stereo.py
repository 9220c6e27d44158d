"""GPU parity: Frame::ComputeStereoMatches (ORB_SLAM2.1/src/Frame.cc:470-641) on the HIP path
(k_stereo over the device-resident pyramids) vs the CPU oracle, bit-exact on mvuRight and
mvDepth (raw float bits) and the kept count.

The synthetic pairs (orbamd.synth_frames with dx) are one crop shifted by a whole number of pixels: every
level-0 SAD is 0 and the median tiny. The scenes of stereo_scenes.py add disparities that vary per row band
(fractional ones, noise, occlusions) and hand-made keypoints on hand-made images, one per edge of the algorithm:
the largest SAD (61 200, past SHRT_MAX in one 16-bit half sum), windows on the last columns of levels whose
width is no multiple of 4, every (c0l & 3, c0r & 3) pair, Hamming and SAD ties, more than 64 candidates in a
band, the median's bin boundaries and its float-rounding edge, the 0.01 branch, both ends of the disparity
range and of the row band. What each scene exercises is asserted on the CPU restatement in
test_oracle_frame.py; here the same inputs go through the HIP path. 320x240 (and 323, 375, 376 wide) are
accepted by both extractors with 8 levels (level 7 is 89x67).

No test asserts a rejection by `deltaR < -1 || deltaR > 1` (Frame.cc:616): there is none to find. The centre of
the fit is the strict first minimum d2 of the 11 distances, so with a = d1 - d2 >= 0 and b = d3 - d2 >= 0 (not
both 0 unless d1 = d2, which the first-minimum rule excludes for the left neighbour) |d1 - d3| = |a - b| <=
a + b = d1 + d3 - 2 d2, hence |deltaR| <= 0.5, and the denominator is 0 only for d1 = d2. The CPU tests assert
instead that no case ever lands there.
"""
import numpy as np
import pytest

import oracle_py
import orbamd
import stereo_scenes as ss

pytestmark = pytest.mark.gpu

MBF, MB = 47.90639384423901, 0.11  # EuRoC-like rig: fx 435.2, baseline 0.11 m


def _pair(agent, t, W, H, dx):
    return orbamd.synth_frames(agent, t, 1, W, H)[0], orbamd.synth_frames(agent, t, 1, W, H, dx=dx)[0]


def _check(ur, dp, n, uo, do, no):
    assert n == no, "kept %d vs oracle %d" % (n, no)
    bad = np.nonzero(ur.view(np.uint32) != uo.view(np.uint32))[0]
    assert bad.size == 0, "mvuRight differs at %s: %s vs %s" % (bad[:5], ur[bad[:5]], uo[bad[:5]])
    bad = np.nonzero(dp.view(np.uint32) != do.view(np.uint32))[0]
    assert bad.size == 0, "mvDepth differs at %s: %s vs %s" % (bad[:5], dp[bad[:5]], do[bad[:5]])


@pytest.mark.parametrize("W,H,nf,dx,agent,t", [(752, 480, 1200, 8, 0, 0), (752, 480, 1200, 17, 3, 9),
                                               (1241, 376, 2000, 12, 1, 2), (640, 480, 1000, 1, 2, 33),
                                               (640, 480, 1000, 26, 5, 7)])
def test_stereo_host_path_bit_exact(W, H, nf, dx, agent, t):
    L, R = _pair(agent, t, W, H, dx)
    el = orbamd.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H)
    er = orbamd.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H)
    ol = oracle_py.OracleExtractor(nf, 1.2, 8, 20, 7)
    orr = oracle_py.OracleExtractor(nf, 1.2, 8, 20, 7)
    kl, dl = el(L)
    kr, dr = er(R)
    ko, do_ = ol(L)
    kro, dro = orr(R)
    assert kl.tobytes() == ko.tobytes() and kr.tobytes() == kro.tobytes()
    ur, dp, n = orbamd.compute_stereo_matches(el, er, kl, dl, kr, dr, MBF, MB)
    uo, dpo, no = oracle_py.compute_stereo_matches(ol, orr, ko, do_, kro, dro, MBF, MB)
    assert n > 0
    _check(ur, dp, n, uo, dpo, no)


def test_stereo_empty_and_mismatched():
    W, H = 640, 480
    L, R = _pair(0, 0, W, H, 8)
    el = orbamd.ORBextractor(1000, 1.2, 8, 20, 7)
    er = orbamd.ORBextractor(1000, 1.2, 8, 20, 7)
    kl, dl = el(L)
    kr, dr = er(np.full((H, W), 77, np.uint8))
    assert len(kr) == 0
    ur, dp, n = orbamd.compute_stereo_matches(el, er, kl, dl, kr, dr, MBF, MB)
    assert n == 0 and (ur == -1).all() and (dp == -1).all()
    # same handle on both sides is rejected (its single-frame pyramid holds one image)
    with pytest.raises(RuntimeError):
        orbamd.compute_stereo_matches(el, el, kl, dl, kl, dl, MBF, MB)


def test_stereo_batch_device_matches_oracle():
    torch = pytest.importorskip("torch")
    W, H, nf, B = 752, 480, 1200, 6
    dev = torch.device("cuda", 0)
    left = orbamd.synth_frames(4, 10, B, W, H)
    right = orbamd.synth_frames(4, 10, B, W, H, dx=9)
    # one handle holding left and right images in one batch (frames 0..B-1 left, B..2B-1 right)
    ext = orbamd.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=2 * B)
    stride = ext.max_keypoints(W, H)
    frames = torch.from_numpy(np.concatenate([left, right])).to(dev)
    kps = torch.empty((2 * B, stride, 6), dtype=torch.float32, device=dev)
    desc = torch.empty((2 * B, stride, 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(2 * B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ext.extract_batch_device(frames, kps, desc, cnt, st)
    fl = torch.arange(B, dtype=torch.int32, device=dev)
    fr = fl + B
    ur = torch.empty((B, stride), dtype=torch.float32, device=dev)
    dp = torch.empty((B, stride), dtype=torch.float32, device=dev)
    ns = torch.zeros(B, dtype=torch.int32, device=dev)
    orbamd.frame.stereo_matches_batch_device(ext, ext, fl, fr, kps, desc, cnt, kps, desc, cnt, MBF, MB, ur, dp, ns,
                                             st)
    torch.cuda.synchronize()
    assert orbamd.load().orbx_check_error(ext._h, st) == 0
    ol = oracle_py.OracleExtractor(nf, 1.2, 8, 20, 7)
    orr = oracle_py.OracleExtractor(nf, 1.2, 8, 20, 7)
    for p in range(B):
        ko, do_ = ol(left[p])
        kro, dro = orr(right[p])
        n = int(cnt[p].item())
        assert n == len(ko)
        uo, dpo, no = oracle_py.compute_stereo_matches(ol, orr, ko, do_, kro, dro, MBF, MB)
        _check(ur[p, :n].cpu().numpy(), dp[p, :n].cpu().numpy(), int(ns[p].item()), uo, dpo, no)


# ------------------------------------------------------------------ varied disparities, hand-made edge cases
H = 240
NF = 500
_ref = {}


def _oracle_band(W, seed, bands, rig=(MBF, MB)):
    """(L, R, kl, dl, kr, dr, oracle result) of a band scene, computed once"""
    key = ("band", W, seed, bands, rig)
    if key not in _ref:
        L, R = ss.band_scene(seed, W, H, bands)
        ol = oracle_py.OracleExtractor(NF, 1.2, 8, 20, 7)
        orr = oracle_py.OracleExtractor(NF, 1.2, 8, 20, 7)
        kl, dl = ol(L)
        kr, dr = orr(R)
        _ref[key] = (L, R, kl, dl, kr, dr, oracle_py.compute_stereo_matches(ol, orr, kl, dl, kr, dr, *rig))
    return _ref[key]


def _oracle_directed(W, subset=None, flat_right=False):
    """(kl, dl, kr, dr, oracle result) of the directed cases, of a subset of their left keypoints, or of all
    of them against a flat right image without keypoints; computed once"""
    c = ss.directed_cases(W, H)
    if ("ext", W) not in _ref:
        ol = oracle_py.OracleExtractor(NF, 1.2, 8, 20, 7)
        orr = oracle_py.OracleExtractor(NF, 1.2, 8, 20, 7)
        ofl = oracle_py.OracleExtractor(NF, 1.2, 8, 20, 7)
        ol(c["left"])
        orr(c["right"])
        assert len(ofl(np.full((H, W), 128, np.uint8))[0]) == 0
        _ref[("ext", W)] = (ol, orr, ofl)
    ol, orr, ofl = _ref[("ext", W)]
    key = ("directed", W, subset, flat_right)
    if key not in _ref:
        kl, dl = (c["kl"], c["dl"]) if subset is None else ss.subset(c, ss.MEDIAN_SUBSETS[subset][0])
        kr, dr = (c["kr"][:0], c["dr"][:0]) if flat_right else (c["kr"], c["dr"])
        _ref[key] = (kl, dl, kr, dr, oracle_py.compute_stereo_matches(ol, ofl if flat_right else orr, kl, dl, kr, dr,
                                                                       c["mbf"], c["mb"]))
    return _ref[key]


def _extractors(W):
    return (orbamd.ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H),
            orbamd.ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H))


@pytest.mark.parametrize("W,seed,bands", ss.BAND_CASES)
def test_stereo_band_scene_host_path(W, seed, bands):
    L, R, ko, do_, kro, dro, ref = _oracle_band(W, seed, bands)
    el, er = _extractors(W)
    kl, dl = el(L)
    kr, dr = er(R)
    assert kl.tobytes() == ko.tobytes() and kr.tobytes() == kro.tobytes()
    ur, dp, n = orbamd.compute_stereo_matches(el, er, kl, dl, kr, dr, MBF, MB)
    assert n > 0
    _check(ur, dp, n, *ref)


@pytest.mark.parametrize("W", [320, 323])
def test_stereo_directed_host_path(W):
    """every directed case at once, then subsets of the left keypoints (other populations for the median pass,
    nL < 16, nR > nL); 323 wide is the byte-wise kernel"""
    c = ss.directed_cases(W, H)
    el, er = _extractors(W)
    el(c["left"])  # the pyramids become resident; the keypoints are the hand-made ones
    er(c["right"])
    for subset in [None] + sorted(ss.MEDIAN_SUBSETS):
        kl, dl, kr, dr, ref = _oracle_directed(W, subset)
        ur, dp, n = orbamd.compute_stereo_matches(el, er, kl, dl, kr, dr, c["mbf"], c["mb"])
        try:
            _check(ur, dp, n, *ref)
        except AssertionError as e:
            names = c["names"] if subset is None else ss.MEDIAN_SUBSETS[subset][0]
            bad = np.nonzero((ur.view(np.uint32) != ref[0].view(np.uint32)) |
                             (dp.view(np.uint32) != ref[1].view(np.uint32)))[0]
            raise AssertionError("subset %s, cases %s: %s" % (subset, [names[i] for i in bad], e))
        if subset is not None:
            assert n == ss.MEDIAN_SUBSETS[subset][2]


@pytest.mark.parametrize("W", [320, 323])
def test_stereo_throw_cases_host_path(W):
    """a left window outside its level raises as the oracle does (Frame.cc:574 asserts before the iniu / endu test
    of :586 is reached), and the per-call error word is cleared: a valid call afterwards is bit-exact"""
    c = ss.directed_cases(W, H)
    el, er = _extractors(W)
    el(c["left"])
    er(c["right"])
    kl, dl, kr, dr, ref = _oracle_directed(W)
    for name, tkl, tdl, tkr, tdr in ss.throw_cases(W, H):
        with pytest.raises(RuntimeError):
            orbamd.compute_stereo_matches(el, er, tkl, tdl, tkr, tdr, c["mbf"], c["mb"])
        ur, dp, n = orbamd.compute_stereo_matches(el, er, kl, dl, kr, dr, c["mbf"], c["mb"])
        _check(ur, dp, n, *ref)


SENTINEL = 7777.0


@pytest.mark.parametrize("W,separate", [(376, False), (376, True), (375, False)])
def test_stereo_batch_indexing_and_edges(W, separate):
    """5 pairs in one launch: fl / fr are no identity and no arange + B, one left frame is paired with two right
    frames and one right frame with two left ones, one right frame is flat (nR == 0), one left frame has 7
    keypoints; the directed keypoints are written into the device arrays after extraction. With one handle for
    all frames, and with a left and a right handle that hold different numbers of frames."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    c = ss.directed_cases(W, H)
    rig, seed = (c["mbf"], c["mb"]), ss.BAND_SHARED_SEED[W]  # one rig per launch: the directed cases' (maxD = 40 px)
    bL, bR, bko, _, bkro, _, ref_b = _oracle_band(W, seed, ss.BANDS, rig)
    bL2, bR2, _, _, bkro2, _, ref_b2 = _oracle_band(W, seed, ss.BANDS_ALT, rig)
    assert (bL == bL2).all()
    flat = np.full((H, W), 128, np.uint8)
    few = "edge_21"
    # (image, hand-made keypoints or None = the extractor's)
    dirL = (c["left"], _oracle_directed(W)[:2])
    dirLfew = (c["left"], _oracle_directed(W, few)[:2])
    dirR = (c["right"], _oracle_directed(W)[2:4])
    if separate:
        lefts, rights = [(bL, None), dirL, dirLfew], [(flat, None), dirR, (bR2, None), (bR, None)]
        fl, fr = [1, 0, 0, 2, 1], [1, 3, 2, 1, 0]
    else:
        lefts = rights = [dirR, (bL, None), (flat, None), (bR, None), dirL, (bR2, None), dirLfew]
        fl, fr = [4, 1, 1, 6, 4], [0, 3, 5, 0, 2]
    refs = [_oracle_directed(W)[4], ref_b, ref_b2, _oracle_directed(W, few)[4], _oracle_directed(W, flat_right=True)[4]]
    nLs = [len(c["kl"]), len(bko), len(bko), len(ss.MEDIAN_SUBSETS[few][0]), len(c["kl"])]
    st = torch.cuda.current_stream(dev).cuda_stream

    def side(frames):
        ext = orbamd.ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=len(frames))
        stride = ext.max_keypoints(W, H)
        assert stride >= len(c["kr"])
        imgs = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
        kps = torch.zeros((len(frames), stride, 6), dtype=torch.float32, device=dev)
        desc = torch.zeros((len(frames), stride, 32), dtype=torch.uint8, device=dev)
        cnt = torch.zeros(len(frames), dtype=torch.int32, device=dev)
        ext.extract_batch_device(imgs, kps, desc, cnt, st)
        torch.cuda.synchronize()
        for f, (_, hand) in enumerate(frames):
            if hand is not None:  # the pyramid of the frame stays, its keypoints become the hand-made ones
                k, d = hand
                raw = np.frombuffer(np.ascontiguousarray(k).tobytes(), np.int32).reshape(len(k), 6)
                kps.view(torch.int32)[f, :len(k)] = torch.from_numpy(raw.copy()).to(dev)
                desc[f, :len(k)] = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
                cnt[f] = len(k)
        return ext, stride, imgs, kps, desc, cnt

    L = side(lefts)
    R = side(rights) if separate else L
    assert L[1] == R[1]
    stride = L[1]
    cl, cr = L[5].cpu().numpy(), R[5].cpu().numpy()
    assert [int(cl[f]) for f in fl] == nLs and int(cr[fr[4]]) == 0
    assert int(cr[fr[1]]) == len(bkro) and int(cr[fr[2]]) == len(bkro2)
    P = len(fl)
    ur = torch.full((P, stride), SENTINEL, dtype=torch.float32, device=dev)
    dp = torch.full((P, stride), SENTINEL, dtype=torch.float32, device=dev)
    ns = torch.full((P,), -5, dtype=torch.int32, device=dev)
    tfl = torch.tensor(fl, dtype=torch.int32, device=dev)
    tfr = torch.tensor(fr, dtype=torch.int32, device=dev)
    orbamd.frame.stereo_matches_batch_device(L[0], R[0], tfl, tfr, L[3], L[4], L[5], R[3], R[4], R[5], c["mbf"], c["mb"],
                                             ur, dp, ns, st)
    torch.cuda.synchronize()
    assert orbamd.load().orbx_check_error(L[0]._h, st) == 0 and orbamd.load().orbx_check_error(R[0]._h, st) == 0
    ur, dp, ns = ur.cpu().numpy(), dp.cpu().numpy(), ns.cpu().numpy()
    for p in range(P):
        _check(ur[p, :nLs[p]], dp[p, :nLs[p]], int(ns[p]), *refs[p])
        # rows at and beyond cnt are untouched
        assert (ur[p, nLs[p]:] == SENTINEL).all() and (dp[p, nLs[p]:] == SENTINEL).all()
    assert (ur[4, :nLs[4]] == -1).all() and ns[4] == 0
    assert ns[1] > 0 and ns[2] > 0 and (ur[1] != ur[2]).any()  # one left frame, two right frames, two results

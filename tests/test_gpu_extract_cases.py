"""GPU parity on the directed extractor cases (tests/extract_cases.py) through every launch schedule, bit-exact.

The images are the ones tests/test_oracle_extract.py proves to reach their branches. Each group (one size and parameter
set) runs through: the host path (ORBextractor.__call__: eager, captured, replayed), a small batch (< 64 frames:
run_extract_levels), a large batch (>= 64: whole-frame pyramid, split octree launches, fork / join), and both batch
sizes again with the frames one byte into their buffer (no fused describe, byte-wise FAST staging, k_blur_strips).
Compared: raw bits of all six keypoint fields, every descriptor byte, every count and every pyramid level."""
import numpy as np
import pytest

import extract_cases as X
import oracle_py
import orbamd
from test_gpu_extract import _compare

pytestmark = pytest.mark.gpu

CASES = X.all_cases()
GROUPS = X.groups(CASES)
GROUP_IDS = ["%dx%d-%s" % (k[0], k[1], "-".join(str(v) for v in k[2:])) for k in GROUPS]
_oracle = {}


def expected(key, image, params):
    """(keypoints, descriptors, pyramid levels) of the oracle, computed once per image"""
    if key not in _oracle:
        orc = oracle_py.OracleExtractor(*params)
        ko, do = orc(image)
        _oracle[key] = (ko, do, [orc.pyramid(l) for l in range(params[2])])
    return _oracle[key]


def group_frames(key):
    """[(name, image)] of a group in mixed order with flat frames (no keypoints) in between"""
    W, H = key[:2]
    cases = GROUPS[key]
    n = len(cases)
    step = next(s for s in (7, 5, 3, 2, 1) if n % s or n == 1)
    order = [cases[(i * step) % n] for i in range(n)]
    assert len({c.name for c in order}) == n
    out = [("flat", X.flat(100, W, H))]
    for i, c in enumerate(order):
        out.append((c.name, c.image))
        if i % 5 == 1:
            out.append(("flat", X.flat(100, W, H)))
    if out[-1][0] != "flat":  # the last case, too, sits between two other frames
        out.append(("flat", X.flat(100, W, H)))
    return out


def device_frames(torch, imgs, offset):
    """[B, H, W] device view with a 4-byte-aligned row pitch, `offset` bytes into its buffer"""
    B, H, W = imgs.shape
    P = (W + 3) // 4 * 4
    buf = torch.zeros(B * H * P + 4, dtype=torch.uint8, device="cuda")
    fr = buf[offset:offset + B * H * P].view(B, H, P)[:, :, :W]
    fr.copy_(torch.from_numpy(imgs).cuda())
    fused = orbamd.load().orbx_describe_blur_fused(fr.data_ptr(), fr.stride(0), fr.stride(1))
    assert fused == (1 if offset == 0 else 0)
    return fr


def run_batch(torch, pipe, key, named, offset, steps=1, pyramid_of=None):
    params = key[2:]
    imgs = np.stack([img for _, img in named])
    fr = device_frames(torch, imgs, offset)
    for _ in range(steps):
        pipe.extract(fr)
        pipe.check_error()
    torch.cuda.synchronize()
    counts = pipe.counts[:len(named)].cpu().numpy()
    for b, (name, img) in enumerate(named):
        ko, do, pyr = expected((key, name), img, params)
        assert counts[b] == len(ko), "frame %d (%s): count %d vs oracle %d" % (b, name, counts[b], len(ko))
        kg, dg = pipe.host_keypoints(b)
        try:
            _compare(kg, dg if len(kg) else do, ko, do)
        except AssertionError as e:
            raise AssertionError("frame %d (%s): %s" % (b, name, e))
        if pyramid_of is None or b in pyramid_of:
            for l in range(params[2]):
                np.testing.assert_array_equal(pipe.ext.pyramid_level(l, frame=b), pyr[l],
                                              err_msg="frame %d (%s) pyramid level %d" % (b, name, l))


def make_pipe(torch, key, B):
    W, H, nf, sf, nl, ini, mn = key
    return orbamd.device.BatchPipeline(torch, W, H, B, nfeatures=nf, scale=sf, nlevels=nl, ini=ini, mini=mn)


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_cases_host_path(key):
    """eager first call, captured second, replays after: at least three calls per geometry, every call compared"""
    W, H = key[:2]
    params = key[2:]
    ext = orbamd.ORBextractor(*params, max_width=W, max_height=H)
    named = group_frames(key)
    while len(named) < 4:
        named = named + named
    for name, img in named:
        kg, dg = ext(img)
        ko, do, pyr = expected((key, name), img, params)
        try:
            _compare(kg, dg if dg is not None else do, ko, do)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        assert (dg is None) == (len(ko) == 0)
        for l in range(params[2]):
            np.testing.assert_array_equal(ext.pyramid_level(l), pyr[l], err_msg="%s pyramid level %d" % (name, l))
    ext.close()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_cases_small_batch(key, offset):
    """all cases of a group in one tensor of fewer than 64 frames (more cases: several tensors), three steps each"""
    torch = pytest.importorskip("torch")
    named = group_frames(key)
    pipe = make_pipe(torch, key, min(len(named), 48))
    for i in range(0, len(named), 48):
        chunk = named[i:i + 48]
        if len(chunk) < 3:
            chunk = named[-3:]
        run_batch(torch, pipe, key, chunk, offset, steps=3)
    pipe.close()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_cases_large_batch(key, offset):
    """the group's cases repeated to fill 64 frames (more cases: 64 per tensor), two steps on one pipeline; every
    frame's keypoints, count and pyramid levels compared"""
    torch = pytest.importorskip("torch")
    named = group_frames(key)
    B = 64
    pipe = make_pipe(torch, key, B)
    for i in range(0, len(named), B):
        chunk = [named[(i + j) % len(named)] for j in range(B)]
        run_batch(torch, pipe, key, chunk, offset, steps=2)
    pipe.close()


@pytest.mark.parametrize("hclass", [0, 1, 2], ids=["h62", "square", "portrait"])
def test_sweep(hclass):
    """the cell-geometry sweep (one level, W = 62..140): one handle per size, created and destroyed in turn; the host
    path three times, then a small and a large batch, each aligned and one byte off"""
    torch = pytest.importorskip("torch")
    sizes = [(w, h) for w, h in X.sweep_sizes() if h == (62, w, w + 17)[hclass]]
    assert len(sizes) == 79
    for w, h in sizes:
        key = (w, h) + X.SWEEP_PARAMS
        img = X.sweep_image(w, h)
        named = [("flat", X.flat(100, w, h)), ("sweep", img), ("flipped", np.ascontiguousarray(img[::-1, ::-1])),
                 ("flat", X.flat(100, w, h))]
        pipe = make_pipe(torch, key, 64)
        ko, do, _ = expected((key, "sweep"), img, X.SWEEP_PARAMS)
        for _ in range(3):
            kg, dg = pipe.ext(img)
            _compare(kg, dg, ko, do)
        large = [named[j % 3] for j in range(64)]
        for offset in (0, 1):
            run_batch(torch, pipe, key, named, offset, pyramid_of=())
            run_batch(torch, pipe, key, large, offset, pyramid_of=())
        pipe.close()


def test_rejected_inputs_leave_the_handle_usable():
    """ORBX_EARG for a level under 62 px, for a level whose borderless aspect ratio rounds to 0 octree roots, and for an
    exact 2x downscale; the next valid call on the same handle is bit-exact (the oracle is not called on the
    rejected inputs: it aborts on the portrait shape and extracts the other two)"""
    for name, bw, bh, params, (gw, gh) in [(n, w, h, p, (161, 161) if p[1] == 2.0 else (120, 100))
                                           for n, w, h, p in X.REJECTED]:
        ext = orbamd.ORBextractor(*params, max_width=max(gw, bw), max_height=max(gh, bh))
        good = X.dots(X.noise(gw, gh, 31, 60, 140), [(40, 40, 250), (70, 60, 5)])
        ko, do, _ = expected(("rejected", name), good, params)
        assert len(ko) > 10
        for _ in range(2):
            kg, dg = ext(good)
            _compare(kg, dg, ko, do)
            with pytest.raises(RuntimeError, match="ORBX_EARG"):
                ext(X.noise(bw, bh, 32))
        kg, dg = ext(good)
        _compare(kg, dg, ko, do)
        ext.close()

"""GPU: the hand-made matcher cases of match_cases.py through every entry point that can express them, exact
equality with the oracle for the match row, the count and the rows the call must not touch. That the oracle is
right, and that each case sits on the edge it is named for, is shown on the CPU (test_oracle_match.py).

  host API       ORBmatcher.SearchForTriangulation / SearchByBoW x2 and their *Cached forms (any case)
  batch          orbm_triangulation_bf_batch_device            one node, no MapPoints, monocular
                 orbm_triangulation_bf_stereo_batch_device     one node, no MapPoints
                 orbm_triangulation_nodes_batch_device         no MapPoints, monocular, bOnlyStereo = false
                 orbm_search_by_bow_batch_device               every SearchByBoW case
  slot kernels   match_slots_device (brute force and over common nodes), bow_slots_device (KF,KF)
"""
import ctypes as C

import numpy as np
import pytest

import match_cases as mc
import orbamd
from orbamd import exchange
from orbamd._lib import ORBX_EARG

pytestmark = pytest.mark.gpu
SENTINEL = -7


# ------------------------------------------------------------------ host API
@pytest.fixture(scope="module")
def host():
    """one matcher and one cache for every case of the module: the per-call state words and sequence numbers
    carry from call to call and from kernel to kernel"""
    m, cache = orbamd.ORBmatcher(0.6, False), orbamd.matcher.KeyFrameCache()
    yield m, cache, iter(range(1, 1 << 30))
    m.close()
    cache.close()


def _tri_kernel(c):
    """matcher.cpp tri_common: `max_nc <= 256 && tasks.size() <= (size_t)kSmallTasks && kf1->n <= 65535 && kf2->n <=
    65535 && node_feats(kf1) <= 32 * kSmallBitWords && node_feats(kf2) <= 32 * kSmallBitWords` -> k_tri_small,
    else k_tri_nodes (kSmallTasks = 160, 32 * kSmallBitWords = 2048; a task = 64 queries of a common node)"""
    v1, v2 = c.views()
    ids2 = {int(n): k for k, n in enumerate(v2.node_id)}
    max_nc = tasks = 0
    for k1, n in enumerate(v1.node_id):
        if int(n) in ids2:
            k2 = ids2[int(n)]
            max_nc = max(max_nc, int(v2.node_off[k2 + 1] - v2.node_off[k2]))
            tasks += -(-int(v1.node_off[k1 + 1] - v1.node_off[k1]) // 64)
    if tasks == 0:
        return "none"
    small = max_nc <= 256 and tasks <= 160 and v1.node_off[-1] <= 2048 and v2.node_off[-1] <= 2048
    return "k_tri_small" if small else "k_tri_nodes"


def _bow_kernel(c):
    """matcher.cpp bow_common: `max_nc <= 64 && ... tasks.size() <= (size_t)kSmallTasks && node_feats(vq) <= 32 *
    kSmallBitWords && node_feats(vc) <= 32 * kSmallBitWords` -> k_bow_small; else launch_bow: `max_nc <= kBowStage`
    (512) -> k_bow<true>, whose nodes of `nc <= 64` take the lane-per-candidate branch and the others the staged
    one; else k_bow<false>"""
    v1, v2 = c.views()
    ids2 = {int(n): k for k, n in enumerate(v2.node_id)}
    ncs = [int(v2.node_off[ids2[int(n)] + 1] - v2.node_off[ids2[int(n)]]) for n in v1.node_id if int(n) in ids2]
    if not ncs:
        return "none"
    if max(ncs) <= 64 and len(ncs) <= 160 and v1.node_off[-1] <= 2048 and v2.node_off[-1] <= 2048:
        return "k_bow_small"
    if max(ncs) <= 512:
        return "k_bow<true> staged+lanes" if min(ncs) <= 64 else "k_bow<true> staged"
    return "k_bow<false>"


# which kernel the sizes of each dispatch case select (the conditions quoted above)
TRI_KERNEL = {
    "f_nc1": "k_tri_small", "f_nc63": "k_tri_small", "f_nc64": "k_tri_small",   # one 64-candidate load per node
    "f_nc65": "k_tri_small", "f_nc255": "k_tri_small",                          # two and four loads
    "f_nc256": "k_tri_small",                                                   # max_nc <= 256 still holds
    "f_nc257": "k_tri_nodes", "f_nc513": "k_tri_nodes",                         # max_nc > 256: two and three rounds
    "f_161_nodes": "k_tri_nodes",                                               # 161 tasks > kSmallTasks
    "f_2049_entries": "k_tri_nodes",                                            # node_feats(kf2) = 2049 > 2048
}
BOW_KERNEL = {
    "g_greedy_nc8_nq3": "k_bow_small", "g_greedy_nc8_nq66": "k_bow_small",      # max_nc = 8 <= 64
    "g_greedy_nc65_nq3": "k_bow<true> staged+lanes",                            # 64 < max_nc = 65 <= 512, and a node of 8
    "g_greedy_nc65_nq66": "k_bow<true> staged+lanes",
    "g_greedy_nc513_nq3": "k_bow<false>", "g_greedy_nc513_nq66": "k_bow<false>",  # max_nc = 513 > kBowStage
}


def test_dispatch_cases_select_their_kernels():
    """launches nothing: the sizes of the dispatch cases against the host API's conditions"""
    assert {c.name: _tri_kernel(c) for c in mc.group("f")} == TRI_KERNEL
    got = {c.name: _bow_kernel(c) for c in mc.group("g") if c.name.startswith("g_greedy")}
    assert got == BOW_KERNEL


def _host_call(m, cache, keys, c, call, cached):
    v1, v2 = c.views()
    m.mfNNratio, m.mbCheckOrientation = float(call["nnratio"]), bool(call["check_ori"])
    if call["kind"] == "tri":
        if cached:
            return m.SearchForTriangulationCached(cache, keys[0], v1, keys[1], v2, c.F12, c.ex, c.ey, call["only_stereo"])
        return m.SearchForTriangulation(v1, v2, c.F12, c.ex, c.ey, call["only_stereo"])
    kfkf = call["kind"] == "bow1"
    if cached:
        return m.SearchByBoWCached(cache, keys[0], v1, v2, other_is_keyframe=kfkf, key2=keys[1])
    return m.SearchByBoW(v1, v2, other_is_keyframe=kfkf)


@pytest.mark.parametrize("g", list(mc.GROUPS))
def test_host_api_cases(host, g):
    m, cache, seq = host
    cases = sorted(mc.group(g), key=lambda c: -(c.k1.n + c.k2.n))   # largest frame first
    total = 0
    for c in cases:
        keys = (next(seq), next(seq))
        for call in c.calls:
            no, mo = mc.oracle_result(c, call)
            for cached in (False, True, True):   # the second cached call finds both keyframes in the cache
                ng, mg = _host_call(m, cache, keys, c, call, cached)
                np.testing.assert_array_equal(mg, mo, err_msg="%s %s cached=%s" % (c.name, call["key"], cached))
                assert ng == no, (c.name, call["key"], cached)
            total += no
    print("host API group %s: %d cases, %d calls x 3, %d matches" % (g, len(cases), sum(len(c.calls) for c in cases), total))
    assert total > 0


# ------------------------------------------------------------------ batch entry points
def _geom_key(c, call):
    return (c.F12.tobytes(), c.ex, c.ey, c.scale.tobytes(), c.sigma2.tobytes(), call["only_stereo"],
            call["check_ori"], call["nnratio"], call["kind"])


def _launches(items):
    """(case, call) pairs grouped by what a batch launch takes once for all its pairs"""
    out = {}
    for c, call in items:
        out.setdefault(_geom_key(c, call), []).append((c, call))
    return list(out.values())


class _Batch:
    """the frames of some cases as one device batch: frame 2 i = case i's candidate side, 2 i + 1 its query side,
    so frame 0 is a candidate frame and the pair lists (q1 = 1, 3, ..; q2 = 0, 2, ..) are no identity"""

    def __init__(self, torch, cases):
        self.torch, self.cases = torch, cases
        kfs = [k for c in cases for k in (c.k2, c.k1)]
        self.B = len(kfs)
        self.S = S = max(k.n for k in kfs) + 3
        kps = np.zeros((self.B, S), mc.KP)
        desc = np.zeros((self.B, S, 32), np.uint8)
        ur = np.full((self.B, S), -1.0, np.float32)
        flags = np.zeros((self.B, S), np.uint8)
        fv_node, fv_off = np.zeros((self.B, S), np.uint32), np.zeros((self.B, S + 1), np.int32)
        fv_feat, nfv = np.zeros((self.B, S), np.int32), np.zeros(self.B, np.int32)
        for b, k in enumerate(kfs):
            if not k.n:
                continue
            kps[b, :k.n], desc[b, :k.n], ur[b, :k.n] = k.keypoints(), k.descriptors(), k.ur
            flags[b, :k.n] = np.array(k.mp, np.uint8) | (np.array(k.bad, np.uint8) << 1)
            fv = k.feat_vec()
            ids = sorted(fv)
            feats = [f for i in ids for f in sorted(fv[i])]
            nfv[b] = len(ids)
            fv_node[b, :len(ids)] = ids
            fv_off[b, 1:len(ids) + 1] = np.cumsum([len(fv[i]) for i in ids])
            fv_feat[b, :len(feats)] = feats
        self.max_nodes = int(nfv.max())
        assert self.max_nodes <= S and all(k.n <= S for k in kfs)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.kps, self.desc, self.ur, self.flags = dev(kps.view(np.uint8)), dev(desc), dev(ur), dev(flags)
        self.counts = dev(np.array([k.n for k in kfs], np.int32))
        self.fv_node, self.fv_off = dev(fv_node.view(np.int32)), dev(fv_off)
        self.fv_feat, self.nfv = dev(fv_feat), dev(nfv)
        P = len(cases)
        self.q1 = dev(np.arange(P, dtype=np.int32) * 2 + 1)
        self.q2 = dev(np.arange(P, dtype=np.int32) * 2)
        self.out = torch.full((P, S), SENTINEL, dtype=torch.int32, device="cuda")
        self.nm = torch.full((P,), SENTINEL, dtype=torch.int32, device="cuda")

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def check(self, calls, untouched):
        """every pair's rows against the oracle; rows past the query frame's count: the sentinel where the entry
        point writes only its queries' rows (untouched), else -1"""
        self.torch.cuda.synchronize()
        out, nm = self.out.cpu().numpy(), self.nm.cpu().numpy()
        total = 0
        for p, (c, call) in enumerate(zip(self.cases, calls)):
            no, mo = mc.oracle_result(c, call)
            rows = len(mo)
            np.testing.assert_array_equal(out[p, :rows], mo, err_msg="%s %s" % (c.name, call["key"]))
            assert (out[p, rows:] == (SENTINEL if untouched else -1)).all(), c.name
            assert nm[p] == no, (c.name, call["key"])
            total += no
        self.out.fill_(SENTINEL)
        self.nm.fill_(SENTINEL)
        return total


def _tri_items(groups, pred):
    return [(c, call) for g in groups for c in mc.group(g) for call in c.calls if call["kind"] == "tri" and pred(c, call)]


def _run_bf(torch, mh, items, stereo):
    lib = orbamd.load()
    total = 0
    for launch in _launches(items):
        cases, calls = [c for c, _ in launch], [k for _, k in launch]
        b, c0, k0 = _Batch(torch, cases), cases[0], calls[0]
        F = np.ascontiguousarray(c0.F12.reshape(9))
        head = (mh, len(cases), b.q1.data_ptr(), b.q2.data_ptr(), b.kps.data_ptr(), b.desc.data_ptr(), b.counts.data_ptr())
        geom = (b.S, F.ctypes.data, c0.ex, c0.ey, len(c0.scale), c0.scale.ctypes.data, c0.sigma2.ctypes.data)
        tail = (int(k0["check_ori"]), b.out.data_ptr(), b.nm.data_ptr(), b.stream())
        if stereo:
            rc = lib.orbm_triangulation_bf_stereo_batch_device(*head, b.ur.data_ptr(), *geom, int(k0["only_stereo"]), *tail)
        else:
            rc = lib.orbm_triangulation_bf_batch_device(*head, *geom, *tail)
        assert rc == 0
        total += b.check(calls, untouched=True)
    print("k_tri_mfma<%s>: %d launches, %d pairs, %d matches" % (str(stereo).lower(), len(_launches(items)), len(items), total))
    return total


@pytest.fixture(scope="module")
def mh():
    h = C.c_void_p()
    orbamd._lib.check(orbamd.load().orbm_create(0, C.byref(h)), "orbm_create")
    yield h
    orbamd.load().orbm_destroy(h)


def test_bf_batch_rejects_a_stride_over_the_key_range(mh):
    """k_tri_mfma's selection key holds 65535 - idx2 in 16 bits: kp_stride > 65536 is ORBX_EARG in both forms
    (before anything is launched or read: every pointer here is null)"""
    lib = orbamd.load()
    F = np.zeros(9, np.float32)
    tab = np.ones(8, np.float32)
    for stride, want in ((65537, ORBX_EARG), (1 << 20, ORBX_EARG), (0, ORBX_EARG), (65536, 0)):
        geom = (stride, F.ctypes.data, 0.0, 0.0, 8, tab.ctypes.data, tab.ctypes.data)
        npairs = 0 if want == 0 else 1   # an accepted stride with no pair returns before any launch
        assert lib.orbm_triangulation_bf_batch_device(mh, npairs, None, None, None, None, None, *geom, 0, None, None,
                                                      None) == want
        assert lib.orbm_triangulation_bf_stereo_batch_device(mh, npairs, None, None, None, None, None, None, *geom, 0,
                                                             0, None, None, None) == want


@pytest.mark.parametrize("stereo", [False, True])
def test_bf_batch_mfma_structure(mh, stereo):
    """group e through k_tri_mfma<false|true>: frame sizes at the tile, chunk and workgroup edges, ties across
    them, the key walk, the padding rows; the empty candidate frame is frame 0 of its batch"""
    torch = pytest.importorskip("torch")
    items = _tri_items("e", lambda c, call: c.stereo_form == stereo)
    assert items[0][0].k2.n == 0 and items[0][0].k1.n > 0
    assert _run_bf(torch, mh, items, stereo) > 0


@pytest.mark.parametrize("stereo", [False, True])
def test_bf_batch_rule_cases(mh, stereo):
    """groups a, b, c, d and h (rotation filter on) through k_tri_mfma: the mono form takes the monocular
    cases, the stereo form every case of one node without MapPoints"""
    torch = pytest.importorskip("torch")
    items = _tri_items("abcdh", lambda c, call: c.one_node and c.no_mp and (stereo or (c.mono and not call["only_stereo"])))
    assert {c.name[0] for c, _ in items} == set("abcdh")
    assert _run_bf(torch, mh, items, stereo) > 0


def test_nodes_batch_cases(mh):
    """k_tri_nodes_pairs over the device FeatureVectors: every monocular case without MapPoints, the 161-node
    and the 2049-entry case among them"""
    torch = pytest.importorskip("torch")
    lib = orbamd.load()
    items = _tri_items("abcdefh", lambda c, call: c.no_mp and c.mono and not call["only_stereo"])
    assert {"f_161_nodes", "f_2049_entries"} <= {c.name for c, _ in items}
    total = 0
    for launch in _launches(items):
        cases, calls = [c for c, _ in launch], [k for _, k in launch]
        b, c0, k0 = _Batch(torch, cases), cases[0], calls[0]
        F = np.ascontiguousarray(c0.F12.reshape(9))
        rc = lib.orbm_triangulation_nodes_batch_device(
            mh, len(cases), b.q1.data_ptr(), b.q2.data_ptr(), b.kps.data_ptr(), b.desc.data_ptr(), b.counts.data_ptr(),
            b.S, b.fv_node.data_ptr(), b.fv_off.data_ptr(), b.fv_feat.data_ptr(), b.nfv.data_ptr(), b.max_nodes,
            F.ctypes.data, c0.ex, c0.ey, len(c0.scale), c0.scale.ctypes.data, c0.sigma2.ctypes.data,
            int(k0["check_ori"]), b.out.data_ptr(), b.nm.data_ptr(), b.stream())
        assert rc == 0
        total += b.check(calls, untouched=False)
    print("k_tri_nodes_pairs: %d launches, %d pairs, %d matches" % (len(_launches(items)), len(items), total))
    assert total > 0


def test_bow_batch_cases(mh):
    """k_bow_pairs: groups g and h, both modes"""
    torch = pytest.importorskip("torch")
    lib = orbamd.load()
    items = [(c, call) for g in "gh" for c in mc.group(g) for call in c.calls if call["kind"] != "tri"]
    total = 0
    for launch in _launches(items):
        cases, calls = [c for c, _ in launch], [k for _, k in launch]
        b, k0 = _Batch(torch, cases), calls[0]
        rc = lib.orbm_search_by_bow_batch_device(
            mh, len(cases), int(k0["kind"][-1]), b.q1.data_ptr(), b.q2.data_ptr(), b.kps.data_ptr(), b.desc.data_ptr(),
            b.counts.data_ptr(), b.S, b.flags.data_ptr(), b.fv_node.data_ptr(), b.fv_off.data_ptr(),
            b.fv_feat.data_ptr(), b.nfv.data_ptr(), b.max_nodes, float(k0["nnratio"]), int(k0["check_ori"]),
            b.out.data_ptr(), b.nm.data_ptr(), b.stream())
        assert rc == 0
        total += b.check(calls, untouched=False)
    print("k_bow_pairs: %d launches, %d pairs, %d matches" % (len(_launches(items)), len(items), total))
    assert total > 0


# ------------------------------------------------------------------ slot kernels
def _slot_inputs(torch, c, cap):
    """KF1 as the device query source, KF2 packed into a slot by the host packer (its scale tables travel in
    the slot's meta)"""
    from test_gpu_exchange import _device_source

    def extras(k):
        ur = np.array(k.ur, np.float32)
        fv = k.feat_vec()
        ids = sorted(fv)
        off = np.concatenate([[0], np.cumsum([len(fv[i]) for i in ids])]).astype(np.int32)
        feat = np.array([f for i in ids for f in sorted(fv[i])], np.int32)
        return dict(uright=ur, depth=np.where(ur >= 0, np.float32(3.5), np.float32(-1)).astype(np.float32),
                    mp_flags=np.array(k.mp, np.uint8) | (np.array(k.bad, np.uint8) << 1),
                    fv=(np.array(ids, np.uint32), off, feat))
    src, keep = _device_source(torch, c.k1.keypoints(), c.k1.descriptors(), extras(c.k1))
    inv = (np.float32(1) / c.sigma2).astype(np.float32)
    meta = exchange.make_meta(agent=1, mnId=3, nlevels=len(c.scale), scale=c.scale, sigma2=c.sigma2, inv_sigma2=inv)
    slot = exchange.pack_host(meta, c.k2.keypoints(), c.k2.descriptors(), cap, **extras(c.k2))
    return src, keep, torch.from_numpy(slot).cuda()


def _slot_cases(groups, kind):
    out = []
    for g in groups:
        for c in mc.group(g):
            for call in c.calls:
                # the slot entry points take no bOnlyStereo and no rotation setting for SearchForTriangulation,
                # and SearchByBoW in its (KF,KF) form only
                if call["kind"] == kind and not call["only_stereo"] and (kind != "tri" or not call["check_ori"]):
                    if c.k1.n and c.k2.n:
                        out.append((c, call))
    return out


def test_slot_triangulation_cases():
    """k_tri_slots (brute force: the one-node cases) and k_tri_slots_bow (common nodes: every case) on groups
    a, c and d, with a small cap"""
    torch = pytest.importorskip("torch")
    m = orbamd.ORBmatcher(0.6, False)
    total = 0
    for c, call in _slot_cases("acd", "tri"):
        cap = max(c.k1.n, c.k2.n) + 5
        src, keep, slot = _slot_inputs(torch, c, cap)
        no, mo = mc.oracle_result(c, call)
        for use_bow in ([False, True] if c.one_node else [True]):
            out = torch.full((1, cap), SENTINEL, dtype=torch.int32, device="cuda")
            nm = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
            exchange.match_slots_device(m._h, src, cap, 1, slot, exchange.slot_bytes(cap), [(c.F12, c.ex, c.ey)], out,
                                        nm, use_bow=use_bow, max_nodes=len(set(c.k1.node)))
            torch.cuda.synchronize()
            assert orbamd.load().orbm_check_error(m._h, None) == 0
            got = out[0].cpu().numpy()
            np.testing.assert_array_equal(got[:c.k1.n], mo, err_msg="%s use_bow=%s" % (c.name, use_bow))
            assert (got[c.k1.n:] == -1).all() and int(nm[0].item()) == no
        total += no
    m.close()
    assert total > 0


def test_slot_search_by_bow_cases():
    """k_bow_slots (its own two-minima merge and accept line) on groups g and h, (KF,KF)"""
    torch = pytest.importorskip("torch")
    m = orbamd.ORBmatcher(0.6, False)
    total = 0
    for c, call in _slot_cases("gh", "bow1"):
        cap = max(c.k1.n, c.k2.n) + 5
        src, keep, slot = _slot_inputs(torch, c, cap)
        no, mo = mc.oracle_result(c, call)
        out = torch.full((1, cap), SENTINEL, dtype=torch.int32, device="cuda")
        nm = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
        exchange.bow_slots_device(m._h, src, cap, 1, slot, exchange.slot_bytes(cap), out, nm, call["nnratio"],
                                  call["check_ori"], max_nodes=len(set(c.k1.node)))
        torch.cuda.synchronize()
        assert orbamd.load().orbm_check_error(m._h, None) == 0
        got = out[0].cpu().numpy()
        np.testing.assert_array_equal(got[:c.k1.n], mo, err_msg=c.name)
        assert (got[c.k1.n:] == -1).all() and int(nm[0].item()) == no
        total += no
    m.close()
    assert total > 0

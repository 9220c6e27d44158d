#!/usr/bin/env python3
"""Measurements of the SURVEY.md 8(f) rows built beside the headline path (one JSON line each).

  stereo       Frame::ComputeStereoMatches on C3 (752x480 stereo, 1200 features): B pairs resident in
               HBM, one step = extract 2B frames + k_stereo over the B pairs (device batch API);
               reported as stereo pairs/s, k_stereo's share from HIP events, and the CPU oracle's
               ComputeStereoMatches alone on the same pairs.
  projection   SearchByProjection(Frame&, vector<MapPoint*>, th) host API (H2D + grid + scan + resolve
               + D2H) per call on a 640x480 frame with ~900 candidate MapPoints vs the CPU oracle.
  distinctive  MapPoint::ComputeDistinctiveDescriptors for 20k MapPoints x ~25 observations (device
               batch) vs the CPU oracle.
  bow          Frame::ComputeBoW (DBoW2 transform, levelsup 4) of 256 extracted 640x480 frames with a synthetic
               vocabulary of ORBvoc.txt's shape (k=10, L=6, 1.1M nodes) resident in HBM, vs the CPU oracle.
  tri_nodes    SearchForTriangulation over common BoW nodes (levelsup 4, ORBvoc.txt-shaped synthetic
               vocabulary) for 256 frame pairs, FeatureVectors from the device BoW transform, vs the
               BF batch (one node) on the same pairs and vs the oracle per pair.
  extract_host ORBextractor::operator() through the host-buffer C ABI on one 640x480 frame per call
               (H2D + whole pipeline + D2H): the Tracking thread's per-frame latency, vs the oracle.
  matcher_host SearchForTriangulation (BF and over BoW nodes), SearchByBoW(KF,F), SearchByBoW(KF,KF)
               through the host C ABI, one keyframe pair per call (how the C++ drop-ins call them).
  kfdb         KeyFrameDatabase query (orbdb_query_device): 4096 keyframes' BowVectors from the device BoW
               transform of synthetic 640x480 frames (ORBvoc.txt-shaped synthetic vocabulary) resident in HBM,
               Q = 1 and Q = 8 queries taken in place from a transform batch; kernel time from HIP events and
               the entry bytes read (sum of counts x 12 B per query) over it as a share of the HBM peak.
  undistort    Frame::UndistortKeyPoints on the device (orbx_undistort_batch_device) over the keypoints of a
               1024-frame C2 extraction (640x480, 1000 features, my.yaml's distorted camera), with and without the
               `kun` output: kernel time from HIP events around 200 launches (median of five windows, min-max), and the
               bytes moved (sum of counts x 48 B, + 8 B with kun) over it as a share of the HBM peak.
  track        Frame-to-frame tracking on C2's shape (640x480 stereo, 1000 features): one 1280-frame stereo batch
               resident in HBM, Frame::UnprojectStereo of every keypoint (orbx_unproject_stereo_batch_device, depths
               and flags from the stereo batch) and SearchByProjection(frame f + 1, frame f) for the 1279 consecutive
               pairs in one launch (orbm_search_by_projection_last_frame_batch_device), each alone from HIP events
               (median of five windows, min-max), vs the per-call orbm_search_by_projection_last_frame over the same
               pairs from host arrays (wall clock around the calls); the two must agree on every pair.
  local        Local-map tracking on C2's shape: a 256-frame stereo batch resident in HBM and a local map of M = 4096
               MapPoints (the unprojected stereo keypoints of frames spread over the batch), Tracking::SearchLocalPoints
               of every frame in one launch (orbm_search_local_points_batch_device: marks, isInFrustum, search) and
               Frame::isInFrustum of the table under every pose alone (orbx_is_in_frustum_batch_device), from HIP events
               (median of five windows, min-max), vs the only route without them: the host unit orbx_is_in_frustum per
               frame, then the per-call orbm_search_by_projection_local from host arrays (wall clock around each); the
               two routes must agree on every frame.
  newpoints    New MapPoints on C2's shape: a 256-frame stereo batch 14 pan steps apart, the stereo BF triangulation
               matcher's rows for the 256 pairs, LocalMapping::CreateNewMapPoints' per-match loop for all pairs in one
               launch (orbm_create_new_map_points_batch_device) from HIP events (median of five windows, min-max), vs
               the only route without it: the match rows copied back and the host unit orbx_triangulate_matches per
               pair (wall clock, median of five); the two must agree on every pair.
  pose         Pose optimisation on C2's shape: a 256-frame stereo batch resident in HBM, about 300 matched MapPoints
               per frame (the frame's own stereo keypoints unprojected under its true pose, 5 mm of noise on each
               position, 5% of them displaced by 0.5 m), a start pose 3 cm and 1 degree off, Optimizer::PoseOptimization
               of every frame in one launch (orbm_pose_optimization_batch_device) from HIP events (median of five
               windows, min-max), vs the only route without it: the host unit orbx_pose_optimization per frame from
               host arrays (wall clock, median of five); the two must agree on every frame, bit for bit.
The CPU figures are the oracle (a plain-C restatement, 1 thread), not the reference build.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cooperative-orb-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


def bench_stereo(torch, steps, B=128):
    import orbamd
    import oracle_py
    W, H, nf = 752, 480, 1200
    MBF, MB = 47.90639384423901, 0.11
    dev = torch.device("cuda", 0)
    left = orbamd.synth_frames(0, 0, B, W, H)
    right = orbamd.synth_frames(0, 0, B, W, H, dx=9)
    ext = orbamd.ORBextractor(nf, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=2 * B)
    stride = ext.max_keypoints(W, H)
    frames = torch.from_numpy(np.concatenate([left, right])).to(dev)
    kps = torch.empty((2 * B, stride, 6), dtype=torch.float32, device=dev)
    desc = torch.empty((2 * B, stride, 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(2 * B, dtype=torch.int32, device=dev)
    fl = torch.arange(B, dtype=torch.int32, device=dev)
    fr = fl + B
    ur = torch.empty((B, stride), dtype=torch.float32, device=dev)
    dp = torch.empty((B, stride), dtype=torch.float32, device=dev)
    ns = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def step(ev=None):
        ext.extract_batch_device(frames, kps, desc, cnt, st)
        if ev:
            ev[0].record()
        orbamd.frame.stereo_matches_batch_device(ext, ext, fl, fr, kps, desc, cnt, kps, desc, cnt, MBF, MB, ur, dp,
                                                 ns, st)
        if ev:
            ev[1].record()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    t0 = time.perf_counter()
    for i in range(steps):
        step(evs[i])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    k_ms = sum(a.elapsed_time(b) for a, b in evs) / steps
    # CPU oracle: ComputeStereoMatches alone (extraction excluded) on a sample of the pairs
    ol = oracle_py.OracleExtractor(nf, 1.2, 8, 20, 7)
    orr = oracle_py.OracleExtractor(nf, 1.2, 8, 20, 7)
    tc, nc = 0.0, 0
    for p in range(8):
        ko, do_ = ol(left[p])
        kro, dro = orr(right[p])
        t = time.perf_counter()
        oracle_py.compute_stereo_matches(ol, orr, ko, do_, kro, dro, MBF, MB)
        tc += time.perf_counter() - t
        nc += 1
    return {"row": "stereo", "workload": "C3 752x480 stereo, 1200 feat, B=%d pairs/step" % B,
            "pairs_per_s_extract_plus_stereo": round(B * steps / el, 1),
            "k_stereo_ms_per_step": round(k_ms, 4), "k_stereo_us_per_pair": round(k_ms * 1e3 / B, 3),
            "stereo_kept_per_pair": round(float(ns.float().mean().item()), 1),
            "cpu_oracle_ms_per_pair": round(tc / nc * 1e3, 3), "cpu_threads": 1}


def bench_tri_nodes(torch, reps):
    import orbamd
    import oracle_py
    from orbamd.matcher import KeyFrameView
    from orbamd.vocabulary import synth_vocabulary_full, L1_NORM, TF_IDF
    k, L, parent, leaf, desc, weight = synth_vocabulary_full(10, 6, 7)
    gv = orbamd.ORBVocabulary.from_arrays(k, L, L1_NORM, TF_IDF, parent, leaf, desc, weight)
    B = 256
    pipe = orbamd.device.BatchPipeline(torch, 640, 480, B)
    frames = orbamd.synth_frames(0, 0, B, 640, 480)
    pipe.extract(torch.from_numpy(frames).cuda())
    pipe.bow(gv, 4)
    torch.cuda.synchronize()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    t_nodes = timed(pipe.match_pairs_nodes)
    n_nodes = float(pipe.nmatch.float().mean().item())
    t_bow = timed(lambda: pipe.bow(gv, 4))
    t_bf = timed(pipe.match_pairs)
    n_bf = float(pipe.nmatch.float().mean().item())
    ov = oracle_py.OracleVocabulary(k, L, L1_NORM, TF_IDF, parent, leaf, desc, weight)
    orc = oracle_py.OracleExtractor(1000, 1.2, 8, 20, 7)
    tabs = orc.tables()
    r0, r1 = orc(frames[1]), orc(frames[0])
    v1 = KeyFrameView(r0[0], r0[1], tabs["scale"], tabs["sigma2"], feat_vec=ov.transform(r0[1], 4)[1])
    v2 = KeyFrameView(r1[0], r1[1], tabs["scale"], tabs["sigma2"], feat_vec=ov.transform(r1[1], 4)[1])
    t = time.perf_counter()
    for _ in range(5):
        oracle_py.search_for_triangulation(v1, v2, pipe.F12, pipe.ex, pipe.ey, False, False)
    c = (time.perf_counter() - t) / 5
    pipe.close()
    return {"row": "search_for_triangulation_bow_nodes", "workload": "256 pairs of 640x480 frames, levelsup 4, "
            "vocabulary k=10 L=6", "gpu_ms_per_256_pairs_nodes": round(t_nodes, 4),
            "gpu_ms_per_256_frames_bow": round(t_bow, 4), "gpu_ms_per_256_pairs_bf": round(t_bf, 4),
            "matches_per_pair_nodes": round(n_nodes, 1), "matches_per_pair_bf": round(n_bf, 1),
            "cpu_oracle_ms_per_pair_nodes": round(c * 1e3, 3), "cpu_threads": 1}


def bench_extract_host(reps):
    import orbamd
    import oracle_py
    img = orbamd.synth_frames(0, 5, 1, 640, 480)[0]
    ext = orbamd.ORBextractor(1000, 1.2, 8, 20, 7)
    for _ in range(5):
        ext(img)
    t = time.perf_counter()
    for _ in range(reps):
        k, d = ext(img)
    g = (time.perf_counter() - t) / reps
    orc = oracle_py.OracleExtractor(1000, 1.2, 8, 20, 7)
    t = time.perf_counter()
    for _ in range(5):
        ko, do = orc(img)
    c = (time.perf_counter() - t) / 5
    assert len(k) == len(ko) and np.array_equal(d, do)
    return {"row": "extract_single_frame_host_api", "workload": "640x480, 1000 features, one frame per call",
            "gpu_ms_per_call": round(g * 1e3, 4), "cpu_oracle_ms_per_call": round(c * 1e3, 3), "cpu_threads": 1}


def bench_matcher_host(reps):
    """per-call latency of the drop-in matcher entry points through the host C ABI (one keyframe pair
    per call, as LocalMapping.cc:268 / Tracking.cc:767 / LoopClosing.cc:267 call them) vs the oracle"""
    import orbamd
    import oracle_py
    from orbamd.matcher import KeyFrameView
    rng = np.random.default_rng(7)
    orc = oracle_py.OracleExtractor(1000, 1.2, 8, 20, 7)
    tabs = orc.tables()
    (k1, d1), (k2, d2) = [orc(img) for img in orbamd.synth_frames(0, 10, 2, 640, 480)]
    F12, ex, ey = orbamd.device.default_geometry()
    ids = np.sort(rng.choice(100000, 90, replace=False))  # ~ the node count at levelsup 4 of ORBvoc.txt

    def fv(n):
        a = rng.integers(0, len(ids), n)
        return {int(ids[i]): list(np.nonzero(a == i)[0]) for i in range(len(ids)) if (a == i).any()}
    fv1, fv2 = fv(len(k1)), fv(len(k2))
    mp1, mp2 = rng.random(len(k1)) < 0.8, rng.random(len(k2)) < 0.8
    rows = []
    cases = [
        ("search_for_triangulation_bf", "SearchForTriangulation, one node (BF), mono, no MapPoints",
         lambda m, a, b: m.SearchForTriangulation(a, b, F12, ex, ey),
         lambda a, b: oracle_py.search_for_triangulation(a, b, F12, ex, ey, False, False),
         KeyFrameView(k1, d1, tabs["scale"], tabs["sigma2"]), KeyFrameView(k2, d2, tabs["scale"], tabs["sigma2"]),
         (0.6, False)),
        ("search_for_triangulation_nodes", "SearchForTriangulation over ~90 common BoW nodes (LocalMapping.cc:268)",
         lambda m, a, b: m.SearchForTriangulation(a, b, F12, ex, ey),
         lambda a, b: oracle_py.search_for_triangulation(a, b, F12, ex, ey, False, False),
         KeyFrameView(k1, d1, tabs["scale"], tabs["sigma2"], feat_vec=fv1),
         KeyFrameView(k2, d2, tabs["scale"], tabs["sigma2"], feat_vec=fv2), (0.6, False)),
        ("search_by_bow_kf_f", "SearchByBoW(KF, F), ~90 nodes, 80% MapPoints, ratio 0.7, rotation check (Tracking.cc:767)",
         lambda m, a, b: m.SearchByBoW(a, b, other_is_keyframe=False),
         lambda a, b: oracle_py.search_by_bow(a, b, 0.7, True, other_is_keyframe=False),
         KeyFrameView(k1, d1, tabs["scale"], tabs["sigma2"], feat_vec=fv1, has_mp=mp1),
         KeyFrameView(k2, d2, tabs["scale"], tabs["sigma2"], feat_vec=fv2), (0.7, True)),
        ("search_by_bow_kf_kf", "SearchByBoW(KF, KF), ~90 nodes, 80% MapPoints, ratio 0.75 (LoopClosing.cc:267)",
         lambda m, a, b: m.SearchByBoW(a, b, other_is_keyframe=True),
         lambda a, b: oracle_py.search_by_bow(a, b, 0.75, True, other_is_keyframe=True),
         KeyFrameView(k1, d1, tabs["scale"], tabs["sigma2"], feat_vec=fv1, has_mp=mp1),
         KeyFrameView(k2, d2, tabs["scale"], tabs["sigma2"], feat_vec=fv2, has_mp=mp2), (0.75, True)),
    ]
    for name, what, g_call, o_call, a, b, (ratio, ori) in cases:
        m = orbamd.ORBmatcher(ratio, ori)
        for _ in range(5):
            ng, mg = g_call(m, a, b)
        t = time.perf_counter()
        for _ in range(reps):
            g_call(m, a, b)
        g = (time.perf_counter() - t) / reps
        t = time.perf_counter()
        for _ in range(max(reps // 5, 3)):
            no, mo = o_call(a, b)
        c = (time.perf_counter() - t) / max(reps // 5, 3)
        assert ng == no and np.array_equal(mg, mo), name
        rows.append({"row": name, "workload": what + "; 640x480 frames, %d / %d features" % (len(k1), len(k2)),
                     "gpu_host_api_ms_per_call": round(g * 1e3, 4), "cpu_oracle_ms_per_call": round(c * 1e3, 4),
                     "nmatches": int(ng), "cpu_threads": 1})
        m.close()
    return rows


def bench_projection(reps):
    import orbamd
    import oracle_py
    import proj_scenes as ps
    F, mps = ps.local_scene(1, True)
    mt = orbamd.ORBmatcher(0.8, False)
    for _ in range(3):
        mt.SearchByProjectionLocal(F, mps, 3.0)
    t = time.perf_counter()
    for _ in range(reps):
        n, _m = mt.SearchByProjectionLocal(F, mps, 3.0)
    g = (time.perf_counter() - t) / reps
    t = time.perf_counter()
    for _ in range(reps):
        oracle_py.search_by_projection_local(F, mps, 3.0, 0.8)
    c = (time.perf_counter() - t) / reps
    return {"row": "search_by_projection_local", "workload": "640x480 frame, %d features, %d MapPoints" % (F.n, mps.n),
            "gpu_host_api_ms_per_call": round(g * 1e3, 4), "cpu_oracle_ms_per_call": round(c * 1e3, 4),
            "nmatches": int(n), "cpu_threads": 1}


def bench_fuse(reps):
    """ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:825-975) per call: the device search
    (host prologue + one H2D, three kernels, one D2H) vs the oracle's search loop (the map updates that
    follow are host bookkeeping in both)."""
    import orbamd
    import oracle_py
    import proj_scenes as ps
    F, Tcw, Ow, mps, inv = ps.fuse_scene(3, True)
    mt = orbamd.ORBmatcher(0.6, True)
    for _ in range(3):
        mt.Fuse(F, Tcw, Ow, mps, 3.0, inv)
    t = time.perf_counter()
    for _ in range(reps):
        n, _b = mt.Fuse(F, Tcw, Ow, mps, 3.0, inv)
    g = (time.perf_counter() - t) / reps
    # the keyframe (arrays + feature grid) held in the keyframe cache: only the MapPoint queries travel
    cache = orbamd.KeyFrameCache()
    for _ in range(3):
        mt.FuseCached(cache, 7, F, Tcw, Ow, mps, 3.0, inv)
    t = time.perf_counter()
    for _ in range(reps):
        n2, b2 = mt.FuseCached(cache, 7, F, Tcw, Ow, mps, 3.0, inv)
    gc = (time.perf_counter() - t) / reps
    t = time.perf_counter()
    for _ in range(reps):
        no, bo = oracle_py.fuse(F, Tcw, Ow, mps, 3.0, inv)
    c = (time.perf_counter() - t) / reps
    same = no == n == n2 and (bo == _b).all() and (bo == b2).all()
    return {"row": "fuse", "workload": "Fuse(pKF, vpMapPoints, 3) (LocalMapping::SearchInNeighbors), 640x480 keyframe, "
            "%d features, %d MapPoints" % (F.n, mps.n),
            "gpu_host_api_ms_per_call": round(g * 1e3, 4), "gpu_cached_kf_ms_per_call": round(gc * 1e3, 4),
            "cpu_oracle_ms_per_call": round(c * 1e3, 4), "identical": bool(same), "nfused": int(n), "cpu_threads": 1}


def bench_distinctive(torch, reps):
    import orbamd
    import oracle_py
    rng = np.random.default_rng(3)
    P = 20000
    sizes = rng.integers(2, 50, P)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    desc = rng.integers(0, 256, (int(off[-1]), 32), dtype=np.uint8)
    dev = torch.device("cuda", 0)
    d_off = torch.from_numpy(off).to(dev)
    d_desc = torch.from_numpy(desc).to(dev)
    d_best = torch.empty(P, dtype=torch.int32, device=dev)
    d_out = torch.empty((P, 32), dtype=torch.uint8, device=dev)
    mt = orbamd.ORBmatcher()
    lib = orbamd.load()
    st = torch.cuda.current_stream(dev).cuda_stream

    def run():
        lib.orbm_compute_distinctive_descriptors_device(mt._h, P, d_off.data_ptr(), d_desc.data_ptr(),
                                                        d_best.data_ptr(), d_out.data_ptr(), st)
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    g = e0.elapsed_time(e1) / reps
    ref = None
    t = time.perf_counter()
    ref = oracle_py.compute_distinctive_descriptors(off[:2001], desc)
    c = (time.perf_counter() - t) / 2000 * P
    assert (d_best[:2000].cpu().numpy() == ref).all()
    return {"row": "compute_distinctive_descriptors", "workload": "%d MapPoints, %d observations" % (P, int(off[-1])),
            "gpu_ms_per_batch": round(g, 4), "cpu_oracle_ms_per_batch": round(c * 1e3, 2), "cpu_threads": 1}


def bench_bow(torch, reps):
    import orbamd
    import oracle_py
    from orbamd.vocabulary import synth_vocabulary_full, L1_NORM, TF_IDF
    k, L, parent, leaf, desc, weight = synth_vocabulary_full(10, 6, 7)
    gv = orbamd.ORBVocabulary.from_arrays(k, L, L1_NORM, TF_IDF, parent, leaf, desc, weight)
    B = 256
    pipe = orbamd.device.BatchPipeline(torch, 640, 480, B)
    dev = torch.device("cuda", 0)
    frames = torch.from_numpy(orbamd.synth_frames(0, 0, B, 640, 480)).to(dev)
    pipe.extract(frames)
    S = pipe.stride
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    word, wt, nid = z(B, S), z(B, S, dt=torch.float64), z(B, S)
    bw, bv, nb = z(B, S), z(B, S, dt=torch.float64), z(B)
    fn, fo, ff, nf = z(B, S), z(B, S + 1), z(B, S), z(B)
    lib = orbamd.load()
    st = torch.cuda.current_stream(dev).cuda_stream

    def run():
        lib.orbv_transform_batch_device(gv._h, B, pipe.desc.data_ptr(), pipe.counts.data_ptr(), S, 4, word.data_ptr(),
                                        wt.data_ptr(), nid.data_ptr(), bw.data_ptr(), bv.data_ptr(), nb.data_ptr(),
                                        fn.data_ptr(), fo.data_ptr(), ff.data_ptr(), nf.data_ptr(), st)
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    g = e0.elapsed_time(e1) / reps
    ov = oracle_py.OracleVocabulary(k, L, L1_NORM, TF_IDF, parent, leaf, desc, weight)
    k0, d0, _m = pipe.host_results(0)
    t = time.perf_counter()
    (ow, oval), ofv = ov.transform(d0, 4)
    c = time.perf_counter() - t
    assert int(nb[0]) == len(ow) and np.array_equal(bw[0, :len(ow)].cpu().numpy().astype(np.uint32), ow)
    mean_n = float(pipe.counts.float().mean().item())
    return {"row": "dbow2_transform", "workload": "256 frames x %.0f descriptors, vocabulary k=10 L=6 (%d nodes)" % (
            mean_n, len(parent) + 1),
            "gpu_ms_per_256_frames": round(g, 4), "gpu_us_per_frame": round(g * 1e3 / B, 3),
            "cpu_oracle_ms_per_frame": round(c * 1e3, 3), "cpu_threads": 1}
    # (pipe's buffers are torch tensors; its handles close with the process)


def bench_kfdb(torch, reps):
    import orbamd
    from orbamd.database import KeyFrameDatabase
    from orbamd.vocabulary import synth_vocabulary_full, L1_NORM, TF_IDF
    HBM_PEAK = 8.0e12  # B/s, the MI355X's HBM3E specification
    k, L, parent, leaf, desc, weight = synth_vocabulary_full(10, 6, 7)
    gv = orbamd.ORBVocabulary.from_arrays(k, L, L1_NORM, TF_IDF, parent, leaf, desc, weight)
    B, NB = 256, 16
    pipe = orbamd.device.BatchPipeline(torch, 640, 480, B)
    S, st = pipe.stride, pipe.stream_ptr()
    db = KeyFrameDatabase(NB * B, min(S, 4096))
    words = 0
    for b in range(NB):  # 16 batches of 256 frames, each agent's own texture
        pipe.extract(torch.from_numpy(orbamd.synth_frames(b, 0, B, 640, 480)).cuda())
        pipe.bow(gv, 4)
        for f in range(B):
            db.add_device(b * B + f, pipe.bow_word[f], pipe.bow_val[f], pipe.nbow[f:f + 1], st)
        words += int(pipe.nbow.sum().item())
    assert not db.check_error(st) and len(db) == NB * B
    dev = pipe.dev
    lib = orbamd.load()
    out = {}
    for Q in (1, 8):
        nc = torch.empty((Q, db.capacity), dtype=torch.int32, device=dev)
        sc = torch.empty((Q, db.capacity), dtype=torch.float32, device=dev)
        fw = torch.empty((Q, db.capacity), dtype=torch.int32, device=dev)

        def run():
            # the queries: rows 0 .. Q-1 of the last transform batch, in place
            rc = lib.orbdb_query_device(db._h, Q, pipe.bow_word.data_ptr(), 4 * S, pipe.bow_val.data_ptr(), 8 * S,
                                        pipe.nbow.data_ptr(), 4, nc.data_ptr(), sc.data_ptr(), fw.data_ptr(), st)
            assert rc == 0
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):  # five windows of `reps` queries: the spread goes into the row
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / reps)
        # query q is keyframe (NB-1)*B + q itself: every word common, score 1 up to rounding
        keys, slots = db.entries()
        own = slots[(NB - 1) * B:(NB - 1) * B + Q]
        q_i = torch.arange(Q, device=dev)
        own_t = torch.from_numpy(own.astype(np.int64)).to(dev)
        assert torch.equal(nc[q_i, own_t], pipe.nbow[:Q]) and bool(((sc[q_i, own_t] - 1).abs() < 1e-6).all())
        t = float(np.median(times))
        out[Q] = (t, min(times), max(times), 12.0 * words * Q / (t * 1e-3))
    row = {"row": "kfdb_query", "workload": "%d keyframes x %.0f words (12 B each), vocabulary k=10 L=6, queries of "
           "~%.0f words in place from a transform batch" % (NB * B, words / (NB * B), words / (NB * B)),
           "entry_bytes_per_query": 12 * words}
    for Q, (t, lo, hi, rate) in out.items():
        row["q%d_ms_per_launch" % Q] = round(t, 4)
        row["q%d_ms_min_max" % Q] = [round(lo, 4), round(hi, 4)]
        row["q%d_entry_bytes_per_s" % Q] = round(rate, 0)
        row["q%d_share_of_hbm_peak_8TBps" % Q] = round(rate / HBM_PEAK, 4)
    db.close()
    pipe.close()
    return row


def bench_undistort(torch, reps):
    import orbamd
    HBM_PEAK = 8.0e12  # B/s, the MI355X's HBM3E specification
    B = 1024
    cam = (715.092024, 719.025258, 334.298489, 256.326097, 0.085908, -0.07019499, 0.0062169, 0.010791)  # my.yaml
    pipe = orbamd.device.BatchPipeline(torch, 640, 480, B)
    st = pipe.stream_ptr()
    pipe.extract(torch.from_numpy(orbamd.synth_frames(0, 0, B, 640, 480)).cuda())
    torch.cuda.synchronize()
    pipe.check_error()
    nkp = int(pipe.counts.sum().item())
    kps_un = torch.empty_like(pipe.kps)
    kun = torch.empty((B, pipe.stride, 2), dtype=torch.float32, device=pipe.dev)
    row = {"row": "undistort_batch", "workload": "%d frames 640x480, %d keypoints (%.0f per frame, stride %d), "
           "my.yaml camera" % (B, nkp, nkp / B, pipe.stride), "launches_per_window": reps}
    for tag, k, per in (("kun", kun, 56), ("nokun", None, 48)):
        def run():
            pipe.ext.undistort_batch_device(cam, pipe.kps, pipe.counts, kps_un, k, st)
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):  # five windows of `reps` launches: the spread goes into the row
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / reps)
        t = float(np.median(times))
        rate = per * nkp / (t * 1e-3)
        row["%s_bytes_per_launch" % tag] = per * nkp
        row["%s_ms_per_launch" % tag] = round(t, 5)
        row["%s_ms_min_max" % tag] = [round(min(times), 5), round(max(times), 5)]
        row["%s_bytes_per_s" % tag] = round(rate, 0)
        row["%s_share_of_hbm_peak_8TBps" % tag] = round(rate / HBM_PEAK, 4)
    # the timed launches computed Frame::UndistortKeyPoints: frame 0 against the host unit
    from orbamd.frame import undistort_keypoints
    k0, _ = pipe.host_keypoints(0)
    got = kps_un[0, :len(k0)].cpu().numpy().copy().view(np.uint8).view(orbamd.kp_dtype).reshape(len(k0))
    row["frame0_equals_host_unit"] = got.tobytes() == undistort_keypoints(cam, k0).tobytes()
    assert row["frame0_equals_host_unit"]
    pipe.close()
    return row


def bench_track(torch, reps, B=1280):
    import orbamd
    from orbamd.device import STEREO_RIGS, BatchPipeline
    W, H = 640, 480
    rig = STEREO_RIGS["euroc"]
    pipe = BatchPipeline(torch, W, H, B, nfeatures=1000, stereo=rig)
    dev, S = pipe.dev, pipe.stride
    left = orbamd.synth_frames(0, 0, B, W, H)
    right = orbamd.synth_frames(0, 0, B, W, H, dx=8)
    pipe.extract(torch.from_numpy(np.concatenate([left, right])).to(dev))
    torch.cuda.synchronize()
    pipe.check_error()
    rng = np.random.default_rng(1)
    poses = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    poses[:, :3, 3] = np.cumsum(rng.normal(0, 0.005, (B, 3)), 0).astype(np.float32)  # a slow drift
    tposes = torch.from_numpy(poses).to(dev)
    flags = torch.zeros((B, S), dtype=torch.uint8, device=dev)
    cur = torch.arange(1, B, dtype=torch.int32, device=dev)
    last = torch.arange(0, B - 1, dtype=torch.int32, device=dev)
    out = torch.empty((B - 1, S), dtype=torch.int32, device=dev)
    nm = torch.zeros(B - 1, dtype=torch.int32, device=dev)
    th, mono, ori = 7.0, False, True  # Tracking.cc:871-877: th = 7 for a stereo camera
    pos = pipe.unproject(tposes, mp_flags=flags)

    def windows(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):  # five windows of n launches: the spread goes into the row
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / n)
        return float(np.median(times)), min(times), max(times)
    t_un = windows(lambda: pipe.unproject(tposes, mp_flags=flags), 10 * reps)
    t_tr = windows(lambda: pipe.track_pairs(cur, last, pos, flags, tposes, th, mono, ori, out, nm), reps)
    pipe.check_match_error()
    # the per-call entry over the same pairs, from host copies of the same arrays
    counts = pipe.counts[:B].cpu().numpy()
    kall = pipe.kps_un[:B].cpu().numpy().copy().view(np.uint8).view(orbamd.kp_dtype).reshape(B, S)
    dall, uall = pipe.desc[:B].cpu().numpy(), pipe.uright.cpu().numpy()
    pall, fall = pos.cpu().numpy(), flags.cpu().numpy()
    g = pipe.track_geom()
    views, mps = [], []
    for f in range(B):
        n = int(counts[f])
        F = orbamd.FrameView(kall[f, :n], dall[f, :n], pipe.scale, W, H, g.fx, g.fy, g.cx, g.cy, bf=g.bf,
                             uright=uall[f, :n])
        F.b = np.float32(g.b)
        views.append(F)
        mps.append(orbamd.MapPoints(n, desc=dall[f, :n], pos=pall[f, :n], has_obs=(fall[f, :n] & 8) != 0,
                                    skip=(fall[f, :n] & 1) == 0, octave=kall[f, :n]["octave"],
                                    angle=kall[f, :n]["angle"]))
    mt = orbamd.ORBmatcher(0.9, ori)
    for f in range(3):
        mt.SearchByProjectionLastFrame(views[f + 1], poses[f + 1], mps[f], poses[f], th, mono)
    res = []
    t0 = time.perf_counter()
    for f in range(B - 1):
        res.append(mt.SearchByProjectionLastFrame(views[f + 1], poses[f + 1], mps[f], poses[f], th, mono))
    t_call = time.perf_counter() - t0
    mt.close()
    out_h, nm_h = out.cpu().numpy(), nm.cpu().numpy()
    same = all(res[f][0] == nm_h[f] and np.array_equal(res[f][1], out_h[f, :len(res[f][1])]) for f in range(B - 1))
    nkp = int(counts.sum())
    row = {"row": "track", "workload": "C2 640x480 stereo, 1000 feat, %d frames (%.0f keypoints per frame, stride %d), "
           "%d consecutive pairs, th %.0f, check_ori" % (B, nkp / B, S, B - 1, th),
           "unproject_ms_per_launch": round(t_un[0], 5), "unproject_ms_min_max": [round(t_un[1], 5), round(t_un[2], 5)],
           "unproject_ns_per_keypoint": round(t_un[0] * 1e6 / nkp, 4),
           "track_ms_per_launch": round(t_tr[0], 4), "track_ms_min_max": [round(t_tr[1], 4), round(t_tr[2], 4)],
           "track_us_per_pair": round(t_tr[0] * 1e3 / (B - 1), 3),
           "per_call_ms_all_pairs": round(t_call * 1e3, 2), "per_call_us_per_pair": round(t_call * 1e6 / (B - 1), 2),
           "matches_per_pair": round(float(nm_h.mean()), 1), "batch_equals_per_call": bool(same)}
    assert same and nm_h.mean() > 50
    pipe.close()
    return row


def bench_local(torch, reps, B=256, M=4096):
    import orbamd
    from orbamd.device import STEREO_RIGS, BatchPipeline
    from orbamd.frame import is_in_frustum
    W, H = 640, 480
    rig = STEREO_RIGS["euroc"]
    pipe = BatchPipeline(torch, W, H, B, nfeatures=1000, stereo=rig)
    dev, S = pipe.dev, pipe.stride
    left = orbamd.synth_frames(0, 0, B, W, H)
    right = orbamd.synth_frames(0, 0, B, W, H, dx=8)
    pipe.extract(torch.from_numpy(np.concatenate([left, right])).to(dev))
    torch.cuda.synchronize()
    pipe.check_error()
    rng = np.random.default_rng(1)
    poses = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    poses[:, :3, 3] = np.cumsum(rng.normal(0, 0.0005, (B, 3)), 0).astype(np.float32)  # a slow drift
    tposes = torch.from_numpy(poses).to(dev)
    flags = torch.zeros((B, S), dtype=torch.uint8, device=dev)
    pos = pipe.unproject(tposes, mp_flags=flags)
    torch.cuda.synchronize()
    # the local map, built on the host (not timed): the keypoints with depth of frames spread over the batch, until M
    counts = pipe.counts[:B].cpu().numpy()
    kall = pipe.kps_un[:B].cpu().numpy().copy().view(np.uint8).view(orbamd.kp_dtype).reshape(B, S)
    dall, uall = pipe.desc[:B].cpu().numpy(), pipe.uright.cpu().numpy()
    pall, fall = pos.cpu().numpy(), flags.cpu().numpy()
    scale = np.asarray(pipe.scale, np.float32)
    tp, tn, tmin, tmax, td = [], [], [], [], []
    have = 0
    for f in ((i * 37) % B for i in range(B)):
        n = int(counts[f])
        ok = fall[f, :n] != 0
        P = pall[f, :n][ok]
        Ow = -(poses[f, :3, :3].astype(np.float64).T @ poses[f, :3, 3].astype(np.float64))
        po = P - Ow
        dist = np.linalg.norm(po, axis=1)
        tp.append(P)
        tn.append((po / dist[:, None]).astype(np.float32))
        mx = (dist * scale[np.clip(kall[f, :n]["octave"][ok], 0, len(scale) - 1)]).astype(np.float32)
        tmax.append(mx)
        tmin.append((mx / scale[-1]).astype(np.float32))
        td.append(dall[f, :n][ok])
        have += len(P)
        if have >= M:
            break
    assert have >= M
    tp, tn, tmin, tmax, td = (np.ascontiguousarray(np.concatenate(a)[:M]) for a in (tp, tn, tmin, tmax, td))
    tfl = np.full(M, 9, np.uint8)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d_pos, d_nrm, d_min, d_max, d_desc, d_fl = up(tp), up(tn), up(tmin), up(tmax), up(td), up(tfl)
    frame_mp = torch.full((B, S), -1, dtype=torch.int32, device=dev)
    out = torch.empty((B, S), dtype=torch.int32, device=dev)
    nm = torch.zeros(B, dtype=torch.int32, device=dev)
    ntm = torch.zeros(B, dtype=torch.int32, device=dev)
    th = 1.0  # Tracking.cc:1185: th = 1 for a stereo camera

    def windows(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):  # five windows of n launches: the spread goes into the row
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / n)
        return float(np.median(times)), min(times), max(times)
    t_fr = windows(lambda: pipe.frustum(tposes, d_pos, d_nrm, d_min, d_max), reps)
    t_lo = windows(lambda: pipe.track_local(tposes, d_pos, d_nrm, d_min, d_max, d_desc, d_fl, frame_mp, th, out, nm,
                                            ntm), reps)
    pipe.check_match_error()
    # the route without the batch entries: the host frustum unit per frame, then the per-call search from host arrays
    g = pipe.track_geom()
    lsf = pipe.log_scale_factor()
    views = []
    for f in range(B):
        n = int(counts[f])
        F = orbamd.FrameView(kall[f, :n], dall[f, :n], pipe.scale, W, H, g.fx, g.fy, g.cx, g.cy, bf=g.bf,
                             uright=uall[f, :n], occupied=np.zeros(n, np.uint8))
        F.b = np.float32(g.b)
        views.append(F)
    mt = orbamd.ORBmatcher(0.8, False)

    def host_route(f):
        t0 = time.perf_counter()
        iv, x, y, xr, lv, vc = is_in_frustum(g, lsf, poses[f], tp, tn, tmin, tmax)
        t1 = time.perf_counter()
        mps = orbamd.MapPoints(M, desc=td, has_obs=np.ones(M, np.uint8), track_in_view=iv, track_proj_x=x,
                               track_proj_y=y, track_proj_xr=xr, track_level=lv, track_view_cos=vc)
        r = mt.SearchByProjectionLocal(views[f], mps, th)
        return r, int(iv.sum()), t1 - t0, time.perf_counter() - t1
    for f in range(3):
        host_route(f)
    res = [host_route(f) for f in range(B)]
    mt.close()
    out_h, nm_h, ntm_h = out.cpu().numpy(), nm.cpu().numpy(), ntm.cpu().numpy()
    same = all(r[0][0] == nm_h[f] and r[1] == ntm_h[f] and np.array_equal(r[0][1], out_h[f, :len(r[0][1])])
               for f, r in enumerate(res))
    t_hf, t_hs = sum(r[2] for r in res), sum(r[3] for r in res)
    row = {"row": "local", "workload": "C2 640x480 stereo, 1000 feat, %d frames (%.0f keypoints per frame, stride %d), "
           "local map M = %d points, th %.0f" % (B, counts.sum() / B, S, M, th),
           "frustum_ms_per_launch": round(t_fr[0], 4), "frustum_ms_min_max": [round(t_fr[1], 4), round(t_fr[2], 4)],
           "frustum_ns_per_point": round(t_fr[0] * 1e6 / (B * M), 4),
           "local_ms_per_launch": round(t_lo[0], 4), "local_ms_min_max": [round(t_lo[1], 4), round(t_lo[2], 4)],
           "local_us_per_frame": round(t_lo[0] * 1e3 / B, 3),
           "host_frustum_us_per_frame": round(t_hf * 1e6 / B, 2), "per_call_search_us_per_frame": round(t_hs * 1e6 / B, 2),
           "host_route_us_per_frame": round((t_hf + t_hs) * 1e6 / B, 2),
           "in_view_per_frame": round(float(ntm_h.mean()), 1), "matches_per_frame": round(float(nm_h.mean()), 1),
           "batch_equals_host_route": bool(same), "query_compaction": "not measured: rejected points stay in place"}
    assert same and ntm_h.mean() > M // 4
    pipe.close()
    return row


def bench_newpoints(torch, reps, B=256):
    """LocalMapping::CreateNewMapPoints' per-match loop for the B pairs of a stereo batch in one launch
    (orbm_create_new_map_points_batch_device over the stereo BF triangulation matcher's rows), against the only route
    without it: the match rows copied back and the host unit (orbx_triangulate_matches) per pair."""
    import orbamd
    from orbamd.device import STEREO_RIGS, BatchPipeline
    from orbamd.frame import triangulate_matches
    from orbamd.matcher import compute_f12, epipole
    W, H = 640, 480
    rig = STEREO_RIGS["euroc"]
    pipe = BatchPipeline(torch, W, H, B, nfeatures=1000, stereo=rig)
    dev, S = pipe.dev, pipe.stride
    # frames 14 steps of the synthetic pan apart: a 28 px shift between neighbours, a baseline above the rig's
    left = np.concatenate([orbamd.synth_frames(0, 14 * f, 1, W, H) for f in range(B)])
    right = np.concatenate([orbamd.synth_frames(0, 14 * f, 1, W, H, dx=8) for f in range(B)])
    cam = pipe.track_camera()
    z = rig[0] / 8.0
    step = np.array([-28.0 * z / cam.fx, 0.0, -0.002])
    poses = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    poses[:, :3, 3] = (np.arange(B)[:, None] * step[None, :]).astype(np.float32)
    K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], np.float32)
    R = np.eye(3, dtype=np.float32)
    pipe.F12 = compute_f12(R, poses[1, :3, 3], R, poses[0, :3, 3], K, K)
    pipe.ex, pipe.ey = epipole(R, poses[0, :3, 3], -poses[1, :3, 3], cam.fx, cam.fy, cam.cx, cam.cy)
    tposes = torch.from_numpy(poses).to(dev)
    pipe.extract(torch.from_numpy(np.concatenate([left, right])).to(dev))
    pipe.match_pairs()
    torch.cuda.synchronize()
    pipe.check_error()

    def windows(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):  # five windows of n launches: the spread goes into the row
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / n)
        return float(np.median(times)), min(times), max(times)
    t_dev = windows(lambda: pipe.create_new_map_points(tposes), reps)
    t = pipe.create_new_map_points(tposes)
    torch.cuda.synchronize()
    pipe.check_match_error()
    # the route without the batch entry: the match rows back to the host, the host unit per pair
    g = pipe.tri_geom()
    counts = pipe.counts[:B].cpu().numpy()
    kall = pipe.kps_un[:B].cpu().numpy().copy().view(np.uint8).view(orbamd.kp_dtype).reshape(B, S)
    dall, uall, zall = pipe.desc[:B].cpu().numpy(), pipe.uright.cpu().numpy(), pipe.depth.cpu().numpy()
    q1, q2 = pipe.q1.cpu().numpy(), pipe.q2.cpu().numpy()

    def host_route():
        t0 = time.perf_counter()
        m = pipe.match.cpu().numpy()
        t1 = time.perf_counter()
        res = []
        for p in range(B):
            a, b = int(q1[p]), int(q2[p])
            n1, n2 = int(counts[a]), int(counts[b])
            res.append(triangulate_matches(g, 0, 1.0, poses[a], poses[b], kall[a, :n1], uall[a, :n1], zall[a, :n1],
                                           dall[a, :n1], kall[b, :n2], uall[b, :n2], zall[b, :n2], m[p, :n1]))
        return res, t1 - t0, time.perf_counter() - t1
    host_route()
    runs = [host_route() for _ in range(5)]
    t_copy = float(np.median([r[1] for r in runs]))
    t_host = float(np.median([r[2] for r in runs]))
    res = runs[-1][0]
    st, nn, tpos = t["status"].cpu().numpy(), t["nnew"].cpu().numpy(), t["pos"].cpu().numpy()
    same = all(r.nnew == nn[p] and np.array_equal(r.status, st[p, :len(r.status)]) and
               r.tab_pos.tobytes() == tpos[p * S:p * S + r.nnew].tobytes() for p, r in enumerate(res))
    nmatch = float((pipe.match.cpu().numpy() >= 0).sum()) / B
    row = {"row": "newpoints", "workload": "C2 640x480 stereo, 1000 feat, %d frames (%.0f keypoints per frame, stride "
           "%d), %d pairs (frame b against b - 1), stereo BF matcher rows" % (B, counts.sum() / B, S, B),
           "batch_ms_per_launch": round(t_dev[0], 4), "batch_ms_min_max": [round(t_dev[1], 4), round(t_dev[2], 4)],
           "batch_us_per_pair": round(t_dev[0] * 1e3 / B, 3),
           "host_copy_us_per_pair": round(t_copy * 1e6 / B, 2), "host_unit_us_per_pair": round(t_host * 1e6 / B, 2),
           "host_us_per_pair": round((t_copy + t_host) * 1e6 / B, 2),
           "matches_per_pair": round(nmatch, 1), "new_points_per_pair": round(float(nn.mean()), 1),
           "batch_equals_host_route": bool(same)}
    assert same and nn.sum() > 0
    pipe.close()
    return row


def bench_pose(torch, reps, B=256, per_frame=300):
    """Optimizer::PoseOptimization of the B frames of a stereo batch in one launch
    (orbm_pose_optimization_batch_device), against the only route without it: the host unit (orbx_pose_optimization)
    per frame over the same arrays read back."""
    import orbamd
    from orbamd.device import STEREO_RIGS, BatchPipeline
    from orbamd.frame import pose_optimization
    W, H = 640, 480
    rig = STEREO_RIGS["euroc"]
    pipe = BatchPipeline(torch, W, H, B, nfeatures=1000, stereo=rig)
    dev, S = pipe.dev, pipe.stride
    left = orbamd.synth_frames(0, 0, B, W, H)
    right = orbamd.synth_frames(0, 0, B, W, H, dx=8)
    cam = pipe.track_camera()
    z = rig[0] / 8.0
    rng = np.random.default_rng(11)
    true = np.tile(np.eye(4, dtype=np.float64), (B, 1, 1))
    true[:, 0, 3] = -2.0 * z / cam.fx * np.arange(B)
    start = np.empty((B, 4, 4), np.float32)
    for f in range(B):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        ang = np.radians(1.0)
        d = np.eye(4)
        d[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        t = rng.normal(size=3)
        d[:3, 3] = t / np.linalg.norm(t) * 0.03
        start[f] = (d @ true[f]).astype(np.float32)
    ttrue = torch.from_numpy(true.astype(np.float32)).to(dev)
    tstart = torch.from_numpy(start).to(dev)
    flags = torch.zeros((B, S), dtype=torch.uint8, device=dev)
    pipe.extract(torch.from_numpy(np.concatenate([left, right])).to(dev))
    pos = pipe.unproject(ttrue, mp_flags=flags).clone()
    valid = flags == 9
    keep = valid & (torch.cumsum(valid.to(torch.int32), 1) <= per_frame)
    idx = torch.arange(B * S, dtype=torch.int32, device=dev).view(B, S)
    mp_index = torch.where(keep, idx, torch.full_like(idx, -1)).contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    pos += torch.randn(pos.shape, generator=gen, device=dev) * 0.005
    gross = torch.rand((B, S), generator=gen, device=dev) < 0.05
    pos[..., 0] += gross.to(torch.float32) * 0.5
    out = torch.empty_like(tstart)
    torch.cuda.synchronize()
    pipe.check_error()

    def windows(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):  # five windows of n launches: the spread goes into the row
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / n)
        return float(np.median(times)), min(times), max(times)
    r = pipe.optimize_pose(tstart, pos, mp_index=mp_index, poses_out=out)
    run = lambda: pipe.optimize_pose(tstart, pos, mp_index=mp_index, poses_out=out, out=r)  # noqa: E731
    t_dev = windows(run, reps)
    r = run()
    torch.cuda.synchronize()
    pipe.check_match_error()
    g, inv = pipe.track_geom(), pipe.inv_level_sigma2()
    counts = pipe.counts[:B].cpu().numpy()
    kall = pipe.kps_un[:B].cpu().numpy().copy().view(np.uint8).view(orbamd.kp_dtype).reshape(B, S)
    uall, mall, hpos = pipe.uright.cpu().numpy(), mp_index.cpu().numpy(), pos.cpu().numpy().reshape(-1, 3)

    def host_route():
        t0 = time.perf_counter()
        res = [pose_optimization(g, inv, start[f], kall[f, :counts[f]], uall[f, :counts[f]], mall[f, :counts[f]], hpos)
               for f in range(B)]
        return res, time.perf_counter() - t0
    host_route()
    runs = [host_route() for _ in range(5)]
    t_host = float(np.median([x[1] for x in runs]))
    res = runs[-1][0]
    hT, ho, hn, hs = (r[k].cpu().numpy() for k in ("poses", "outlier", "ninliers", "status"))
    same = all(x.Tcw.tobytes() == hT[f].tobytes() and x.ninliers == hn[f] and x.status == hs[f] and
               np.array_equal(x.outlier[mall[f, :counts[f]] >= 0], ho[f, :counts[f]][mall[f, :counts[f]] >= 0])
               for f, x in enumerate(res))
    dg = np.array([x.diag for x in res])
    err = max(float(np.abs(x.Tcw.astype(np.float64) - true[f]).max()) for f, x in enumerate(res))
    row = {"row": "pose", "workload": "C2 640x480 stereo, 1000 feat, %d frames (%.0f keypoints per frame, stride %d), "
           "%.0f matched MapPoints per frame, start 3 cm / 1 deg off" % (B, counts.sum() / B, S, float(keep.sum()) / B),
           "batch_ms_per_launch": round(t_dev[0], 4), "batch_ms_min_max": [round(t_dev[1], 4), round(t_dev[2], 4)],
           "batch_us_per_frame": round(t_dev[0] * 1e3 / B, 3), "host_unit_us_per_frame": round(t_host * 1e6 / B, 2),
           "lm_iterations_per_frame": round(float(dg[:, 1:5].sum(1).mean()), 1),
           "rejected_trials_per_frame": round(float(dg[:, 5].mean()), 1),
           "inliers_per_frame": round(float(hn.mean()), 1), "max_pose_error": float("%.3g" % err),
           "workgroup": "128 lanes, 128-edge chunks (256 not tried)", "batch_equals_host_route": bool(same)}
    assert same and (hs == 0).all()
    pipe.close()
    return row


def main():
    import torch
    steps = int(os.environ.get("BENCH_ROWS_STEPS", "10"))
    only = os.environ.get("BENCH_ROWS_ONLY")
    rows = {"extract_host": lambda: bench_extract_host(100), "matcher_host": lambda: bench_matcher_host(100),
            "stereo": lambda: bench_stereo(torch, steps), "projection": lambda: bench_projection(50), "fuse": lambda: bench_fuse(50),
            "distinctive": lambda: bench_distinctive(torch, 10), "bow": lambda: bench_bow(torch, 10),
            "tri_nodes": lambda: bench_tri_nodes(torch, 10), "kfdb": lambda: bench_kfdb(torch, 200),
            "undistort": lambda: bench_undistort(torch, 200), "track": lambda: bench_track(torch, 10),
            "local": lambda: bench_local(torch, 10), "newpoints": lambda: bench_newpoints(torch, 10),
            "pose": lambda: bench_pose(torch, 10)}
    for name, fn in rows.items():
        if only and name not in only.split(","):
            continue
        r = fn()
        for line in (r if isinstance(r, list) else [r]):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

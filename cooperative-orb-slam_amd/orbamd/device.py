"""Device-resident batch pipeline (torch tensors as HBM buffers, HIP stream from torch).

One "step" of the hot path over a batch of B frames already in HBM:
  orbx_extract_batch_device  -> keypoints/descriptors/counts per frame
  orbm_triangulation_bf_batch_device -> SearchForTriangulation(frame b, frame b-1 mod B)
torch is plumbing only (allocation, streams, torch.distributed); all compute is in
liborbamd.so.
"""
import ctypes as C

import numpy as np

from ._lib import check, load
from .extractor import ORBextractor

# camera of the reference config (ORB_SLAM2/my.yaml:8-11)
FX, FY, CX, CY = 715.092024, 719.025258, 334.298489, 256.326097

# stereo rigs of the BASELINE stereo configs: Camera.bf and the baseline mb = mbf / fx (Frame.cc:501-503, Tracking.cc
# reads Camera.bf). EuRoC (EuRoC.yaml: fx 435.2047, bf 47.90639384423901) and KITTI 00-02 (KITTI00-02.yaml: fx 718.856,
# bf 386.1448)
STEREO_RIGS = {"euroc": (47.90639384423901, 47.90639384423901 / 435.2046959714599),
               "kitti": (386.1448, 386.1448 / 718.856)}


def default_geometry():
    """KF2 pose relative to KF1: R = I, t = (0.05, 0, 0.01); returns (F12, ex, ey)."""
    from .matcher import compute_f12, epipole
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]], np.float32)
    R1 = np.eye(3, dtype=np.float32)
    t1 = np.zeros(3, np.float32)
    R2 = np.eye(3, dtype=np.float32)
    t2 = np.array([0.05, 0.0, 0.01], np.float32)
    F12 = compute_f12(R1, t1, R2, t2, K, K)
    Cw = -R1.T @ t1  # KF1 camera centre
    ex, ey = epipole(R2, t2, Cw, FX, FY, CX, CY)
    return F12, ex, ey


class BatchPipeline:
    """Extract + match over batches of frames on one GPU.

    stereo=(mbf, mb): every frame is a rectified stereo pair (the stereo Frame constructor, ORB_SLAM2.1/src/Frame.cc:
    80-98): the extraction batch holds the B left images (images 0..B-1) and then the B right images (B..2B-1),
    one orbx_extract_batch_device over all 2B (the two ORBextractor instances share the parameters,
    Tracking.cc:119-125); Frame::ComputeStereoMatches gives every left keypoint its mvuRight / mvDepth
    (orbx_stereo_matches_batch_device), and SearchForTriangulation of frame b against b-1 takes the stereo branch
    (orbm_triangulation_bf_stereo_batch_device).

    camera=(fx, fy, cx, cy, k1, k2, p1, p2[, k3]) (orbamd.frame.make_camera): a distorted camera. Every extraction is
    followed on the same stream by Frame::UndistortKeyPoints on the device (orbx_undistort_batch_device) into kps_un
    (mvKeysUn, what every matcher here reads) and kun (their x, y: the keyframe slot's KUN section); kps stays
    mvKeys. camera=None: mvKeysUn = mvKeys, no launch, no extra buffer."""

    def __init__(self, torch, width=640, height=480, batch=64, nfeatures=1000, scale=1.2, nlevels=8, ini=20, mini=7,
                 device=0, check_ori=False, stereo=None, camera=None):
        self.torch = torch
        self.W, self.H, self.B = width, height, batch
        self.stereo = stereo
        self.nimg = 2 * batch if stereo else batch
        nimg = self.nimg
        self.ext = ORBextractor(nfeatures, scale, nlevels, ini, mini, device=device, max_width=width,
                                max_height=height, max_batch=nimg)
        self.lib = load()
        self.stride = self.ext.max_keypoints(width, height)
        dev = torch.device("cuda", device)
        self.dev = dev
        self.kps = torch.empty((nimg, self.stride, 6), dtype=torch.float32, device=dev)
        self.desc = torch.empty((nimg, self.stride, 32), dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(nimg, dtype=torch.int32, device=dev)
        self.camera = None
        self.kps_un, self.kun = self.kps, None  # mvKeysUn = mvKeys without a camera
        if camera is not None:
            from .frame import make_camera
            self.camera = make_camera(camera)
            self.kps_un = torch.empty_like(self.kps)
            self.kun = torch.empty((nimg, self.stride, 2), dtype=torch.float32, device=dev)
        self.match = torch.empty((batch, self.stride), dtype=torch.int32, device=dev)
        self.nmatch = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.q1 = torch.arange(batch, dtype=torch.int32, device=dev)
        self.q2 = ((self.q1 + batch - 1) % batch).to(torch.int32)
        if stereo:
            self.uright = torch.empty((batch, self.stride), dtype=torch.float32, device=dev)
            self.depth = torch.empty((batch, self.stride), dtype=torch.float32, device=dev)
            self.nstereo = torch.zeros(batch, dtype=torch.int32, device=dev)
            self.fr = (self.q1 + batch).to(torch.int32)
        h = C.c_void_p()
        check(self.lib.orbm_create(device, C.byref(h)), "orbm_create")
        self.mh = h
        self.F12, self.ex, self.ey = default_geometry()
        self.scale = self.ext.GetScaleFactors()
        self.sigma2 = self.ext.GetScaleSigmaSquares()
        self.check_ori = int(check_ori)

    def stream_ptr(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def extract(self, frames, stream=None, stereo=True):
        """frames: [nimg, H, W] device images (stereo: the B left images, then the B right ones); a stereo pipeline
        then runs ComputeStereoMatches for every pair on the same stream (stereo=False: the caller does)"""
        st = self.stream_ptr() if stream is None else stream
        self.ext.extract_batch_device(frames, self.kps, self.desc, self.counts, st)
        if self.camera is not None:
            self.ext.undistort_batch_device(self.camera, self.kps, self.counts, self.kps_un, self.kun, st)
        if self.stereo and stereo:
            self.stereo_matches(st)

    def stereo_matches(self, stream=None):
        """Frame::ComputeStereoMatches of every pair (left image b, right image B + b) on the device"""
        st = self.stream_ptr() if stream is None else stream
        mbf, mb = self.stereo
        check(self.lib.orbx_stereo_matches_batch_device(
            self.ext._h, self.ext._h, self.B, self.q1.data_ptr(), self.fr.data_ptr(), self.kps.data_ptr(),
            self.desc.data_ptr(), self.counts.data_ptr(), self.kps.data_ptr(), self.desc.data_ptr(),
            self.counts.data_ptr(), self.stride, float(mbf), float(mb), self.uright.data_ptr(), self.depth.data_ptr(),
            self.nstereo.data_ptr(), st), "orbx_stereo_matches_batch_device")

    def check_error(self, stream=None):
        st = self.stream_ptr() if stream is None else stream
        check(self.lib.orbx_check_error(self.ext._h, st), "orbx_check_error")

    def match_pairs(self, stream=None):
        st = self.stream_ptr() if stream is None else stream
        F = np.ascontiguousarray(self.F12.reshape(9))
        if self.stereo:
            check(self.lib.orbm_triangulation_bf_stereo_batch_device(
                self.mh, self.B, self.q1.data_ptr(), self.q2.data_ptr(), self.kps_un.data_ptr(), self.desc.data_ptr(),
                self.counts.data_ptr(), self.uright.data_ptr(), self.stride, F.ctypes.data, self.ex, self.ey,
                len(self.scale), self.scale.ctypes.data, self.sigma2.ctypes.data, 0, self.check_ori,
                self.match.data_ptr(), self.nmatch.data_ptr(), st), "orbm_triangulation_bf_stereo_batch_device")
            return
        check(self.lib.orbm_triangulation_bf_batch_device(
            self.mh, self.B, self.q1.data_ptr(), self.q2.data_ptr(), self.kps_un.data_ptr(), self.desc.data_ptr(),
            self.counts.data_ptr(), self.stride, F.ctypes.data, self.ex, self.ey, len(self.scale),
            self.scale.ctypes.data, self.sigma2.ctypes.data, self.check_ori, self.match.data_ptr(),
            self.nmatch.data_ptr(), st), "orbm_triangulation_bf_batch_device")

    def bow(self, vocabulary, levelsup=4, stream=None):
        """Frame::ComputeBoW of every extracted frame on the device (orbv_transform_batch_device); the
        FeatureVectors stay in self.fv_node / fv_off / fv_feat / nfv for match_pairs_nodes."""
        torch, dev, B, S = self.torch, self.dev, self.B, self.stride
        if getattr(self, "_bow_bufs", None) is None:
            z = lambda *sh, dt=torch.int32: torch.zeros(*sh, dtype=dt, device=dev)  # noqa: E731
            self.word, self.word_w, self.word_nid = z(B, S), z(B, S, dt=torch.float64), z(B, S)
            self.bow_word, self.bow_val, self.nbow = z(B, S), z(B, S, dt=torch.float64), z(B)
            self.fv_node, self.fv_off, self.fv_feat, self.nfv = z(B, S), z(B, S + 1), z(B, S), z(B)
            self._bow_bufs = True
        st = self.stream_ptr() if stream is None else stream
        check(self.lib.orbv_transform_batch_device(
            vocabulary._h, B, self.desc.data_ptr(), self.counts.data_ptr(), S, levelsup, self.word.data_ptr(),
            self.word_w.data_ptr(), self.word_nid.data_ptr(), self.bow_word.data_ptr(), self.bow_val.data_ptr(),
            self.nbow.data_ptr(), self.fv_node.data_ptr(), self.fv_off.data_ptr(), self.fv_feat.data_ptr(),
            self.nfv.data_ptr(), st), "orbv_transform_batch_device")
        info = vocabulary.info()
        self.max_nodes = int(min(S, info["k"] ** max(info["L"] - levelsup, 0)))

    def match_pairs_nodes(self, stream=None):
        """SearchForTriangulation over the common BoW nodes of each pair (after bow())."""
        st = self.stream_ptr() if stream is None else stream
        F = np.ascontiguousarray(self.F12.reshape(9))
        check(self.lib.orbm_triangulation_nodes_batch_device(
            self.mh, self.B, self.q1.data_ptr(), self.q2.data_ptr(), self.kps_un.data_ptr(), self.desc.data_ptr(),
            self.counts.data_ptr(), self.stride, self.fv_node.data_ptr(), self.fv_off.data_ptr(),
            self.fv_feat.data_ptr(), self.nfv.data_ptr(), self.max_nodes, F.ctypes.data, self.ex, self.ey,
            len(self.scale), self.scale.ctypes.data, self.sigma2.ctypes.data, self.check_ori, self.match.data_ptr(),
            self.nmatch.data_ptr(), st), "orbm_triangulation_nodes_batch_device")

    def search_by_bow_pairs(self, mode, qf, cf, mp_flags, nnratio, check_ori, out, nmatches, stream=None):
        """SearchByBoW over the device FeatureVectors of bow(): mode 1 = (KF,KF), 0 = (KF,F); qf / cf int32
        cuda [npairs]; mp_flags uint8 cuda [B, stride] (bit 0 MapPoint, bit 1 bad); out int32 [npairs, stride]."""
        st = self.stream_ptr() if stream is None else stream
        check(self.lib.orbm_search_by_bow_batch_device(
            self.mh, int(qf.numel()), int(mode), qf.data_ptr(), cf.data_ptr(), self.kps_un.data_ptr(),
            self.desc.data_ptr(), self.counts.data_ptr(), self.stride, mp_flags.data_ptr(), self.fv_node.data_ptr(),
            self.fv_off.data_ptr(), self.fv_feat.data_ptr(), self.nfv.data_ptr(), self.max_nodes, float(nnratio),
            int(check_ori), out.data_ptr(), nmatches.data_ptr(), st), "orbm_search_by_bow_batch_device")

    # ---- frame-to-frame tracking (include/orbslam_amd.h "Frame-to-frame tracking on a device batch") ----
    def track_camera(self):
        """the orbx_camera the tracking calls use: the pipeline's camera, or my.yaml's without distortion"""
        from .frame import make_camera
        return self.camera if self.camera is not None else make_camera((FX, FY, CX, CY, 0, 0, 0, 0))

    def track_geom(self):
        """orbm_track_geom of this pipeline: its camera (camera=None: my.yaml's, the image's own bounds), the stereo
        rig's mbf / mb (monocular: 0) and the extractor's scale factors"""
        from .frame import image_bounds, track_geom
        if getattr(self, "_track_geom", None) is None:
            cam = self.track_camera()
            b, gw, gh = image_bounds(cam, self.W, self.H)
            mbf, mb = self.stereo if self.stereo else (0.0, 0.0)
            self._track_geom = track_geom(cam.fx, cam.fy, cam.cx, cam.cy, mbf, mb, b, gw, gh, self.scale)
        return self._track_geom

    def unproject(self, poses, pos=None, mp_flags=None, valid_flags=9, stream=None):
        """Frame::UnprojectStereo (Frame.cc:667-681) of every keypoint of the B frames (stereo pipeline: kps_un and
        depth of the left images) on the device: poses float32 cuda [B, 4, 4] (mTcw); pos float32 cuda [B, stride, 3]
        (default: self.pos). With mp_flags (uint8 cuda [B, stride]) every row also gets valid_flags for z > 0 and 0
        otherwise (default 9: a MapPoint with observations, what track_pairs reads). Returns pos."""
        torch = self.torch
        if not self.stereo:
            raise RuntimeError("unproject needs a stereo pipeline (mvDepth)")
        if pos is None:
            if getattr(self, "pos", None) is None:
                self.pos = torch.zeros((self.B, self.stride, 3), dtype=torch.float32, device=self.dev)
            pos = self.pos
        st = self.stream_ptr() if stream is None else stream
        cam = self.track_camera()
        check(self.lib.orbx_unproject_stereo_batch_device(
            self.ext._h, C.byref(cam), self.B, self.kps_un.data_ptr(), self.depth.data_ptr(), self.counts.data_ptr(),
            self.stride, poses.data_ptr(), pos.data_ptr(), mp_flags.data_ptr() if mp_flags is not None else None,
            int(valid_flags), st), "orbx_unproject_stereo_batch_device")
        return pos

    def track_pairs(self, cur, last, pos, mp_flags, poses, th, mono, check_ori, out, nmatches, stream=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1328-1470) of every pair (cur[p],
        last[p]) over the pipeline's own kps_un, desc, counts and (stereo) uright: cur / last int32 cuda [npairs]
        (frames 0..B-1); pos float32 [B, stride, 3] and mp_flags uint8 [B, stride] (bit 0 MapPoint, bit 2 outlier,
        bit 3 observations) of every frame; poses float32 [B, 4, 4]; out int32 [npairs, stride], nmatches int32
        [npairs]. No feature of a current frame is occupied beforehand (Tracking.cc:879 clears mvpMapPoints)."""
        st = self.stream_ptr() if stream is None else stream
        g = self.track_geom()
        check(self.lib.orbm_search_by_projection_last_frame_batch_device(
            self.mh, int(cur.numel()), cur.data_ptr(), last.data_ptr(), self.B, self.kps_un.data_ptr(),
            self.desc.data_ptr(), self.counts.data_ptr(), self.stride,
            self.uright.data_ptr() if self.stereo else None, None, pos.data_ptr(), mp_flags.data_ptr(), poses.data_ptr(), C.byref(g), float(th), int(bool(mono)),
            int(bool(check_ori)), out.data_ptr(), nmatches.data_ptr(), st),
            "orbm_search_by_projection_last_frame_batch_device")

    # ---- local-map tracking (include/orbslam_amd.h "Local-map tracking on a device batch") ----
    def log_scale_factor(self):
        """mfLogScaleFactor = log(mfScaleFactor) of the pipeline's extractor (Frame.cc:72), as a float"""
        import math
        return float(np.float32(math.log(float(np.float32(self.ext.GetScaleFactor())))))

    def frustum(self, poses, pos, normal, min_dist, max_dist, viewing_cos_limit=0.5, stream=None):
        """Frame::isInFrustum (Frame.cc:274-330) of a device table of M MapPoints under each of the nf poses (float32
        cuda [nf, 4, 4]): pos / normal float32 cuda [M, 3], min_dist / max_dist float32 cuda [M] (raw mfMinDistance /
        mfMaxDistance). Returns the six tracking arrays as cuda tensors [nf, M]: (in_view uint8, proj_x, proj_y,
        proj_xr float32, level int32, view_cos float32)."""
        torch = self.torch
        nf, M = int(poses.shape[0]), int(pos.shape[0])
        z = lambda dt: torch.zeros((nf, M), dtype=dt, device=self.dev)  # noqa: E731
        out = (z(torch.uint8), z(torch.float32), z(torch.float32), z(torch.float32), z(torch.int32), z(torch.float32))
        st = self.stream_ptr() if stream is None else stream
        g = self.track_geom()
        check(self.lib.orbx_is_in_frustum_batch_device(
            self.mh, C.byref(g), self.log_scale_factor(), float(viewing_cos_limit), M, pos.data_ptr(),
            normal.data_ptr(), min_dist.data_ptr(), max_dist.data_ptr(), nf, poses.data_ptr(),
            *[t.data_ptr() for t in out], st), "orbx_is_in_frustum_batch_device")
        return out

    def track_local(self, poses, pos, normal, min_dist, max_dist, mp_desc, mp_flags, frame_mp, th, out, nmatches,
                    ntomatch, ranges=None, in_view=None, nnratio=0.8, viewing_cos_limit=0.5, stream=None):
        """Tracking::SearchLocalPoints (Tracking.cc:1143-1193) of the B frames over the pipeline's own kps_un, desc,
        counts and (stereo) uright: poses float32 cuda [B, 4, 4]; the local-map table pos / normal float32 [M, 3],
        min_dist / max_dist float32 [M], mp_desc uint8 [M, 32], mp_flags uint8 [M] (bit 1 bad, bit 3 observations);
        frame_mp int32 [B, stride] = the table index of every feature's MapPoint or -1 (e.g. mapped from track_pairs'
        match rows); ranges int32 [B, 2] = each frame's slice of the table (None: all of it); out int32 [B, stride],
        nmatches / ntomatch int32 [B]; in_view uint8 [B, M] (optional). th = 1, 3 (RGB-D) or 5 (after a
        relocalisation); nnratio = the ORBmatcher's (0.8 in SearchLocalPoints)."""
        st = self.stream_ptr() if stream is None else stream
        g = self.track_geom()
        M = int(pos.shape[0])
        check(self.lib.orbm_search_local_points_batch_device(
            self.mh, self.B, self.kps_un.data_ptr(), self.desc.data_ptr(), self.counts.data_ptr(), self.stride,
            self.uright.data_ptr() if self.stereo else None, poses.data_ptr(), C.byref(g), self.log_scale_factor(), M,
            pos.data_ptr(), normal.data_ptr(), min_dist.data_ptr(), max_dist.data_ptr(), mp_desc.data_ptr(),
            mp_flags.data_ptr(), ranges.data_ptr() if ranges is not None else None, frame_mp.data_ptr(), float(th),
            float(nnratio), float(viewing_cos_limit), out.data_ptr(), nmatches.data_ptr(), ntomatch.data_ptr(),
            in_view.data_ptr() if in_view is not None else None, st), "orbm_search_local_points_batch_device")

    # ---- new MapPoints (include/orbslam_amd.h "New MapPoints from triangulation matches") ----
    def tri_geom(self):
        """orbm_tri_geom of this pipeline: track_camera(), the stereo rig's mbf / mb (monocular: 0) and the extractor's
        mvScaleFactors / mvLevelSigma2; both keyframes of every pair use it"""
        from .frame import tri_geom
        if getattr(self, "_tri_geom", None) is None:
            cam = self.track_camera()
            mbf, mb = self.stereo if self.stereo else (0.0, 0.0)
            self._tri_geom = tri_geom(cam.fx, cam.fy, cam.cx, cam.cy, mbf, mb, self.scale, self.sigma2)
        return self._tri_geom

    def create_new_map_points(self, poses, median_depth2=None, match=None, q1=None, q2=None, stream=None):
        """The per-match loop of LocalMapping::CreateNewMapPoints (LocalMapping.cc:284-450) over the pipeline's own
        match rows (match_pairs / match_pairs_nodes; pair p = frame q1[p] against q2[p]) on the device: poses float32
        cuda [B, 4, 4] (mTcw); a monocular pipeline needs median_depth2 float32 cuda [npairs] (KF2's
        ComputeSceneMedianDepth(2)). Returns a dict of cuda tensors: status int8 [npairs, stride] (ORBM_TRI_*), pos3
        float32 [npairs, stride, 3], and the table of M = npairs * stride MapPoints track_local reads -- pos, normal
        [M, 3], min_dist, max_dist [M], desc uint8 [M, 32], flags uint8 [M], feat1, feat2 int32 [M] -- with pair p's
        new points in rows ranges[p, 0] .. ranges[p, 1] (int32 [npairs, 2], track_local's ranges) and nnew int32
        [npairs]. Only enqueues; the buffers are allocated once and reused."""
        torch = self.torch
        match = self.match if match is None else match
        q1 = self.q1 if q1 is None else q1
        q2 = self.q2 if q2 is None else q2
        P, S = int(q1.numel()), self.stride
        if not self.stereo and median_depth2 is None:
            raise RuntimeError("a monocular pipeline needs median_depth2")
        t = getattr(self, "_new_mp", None)
        if t is None or t["status"].shape[0] != P:
            z = lambda *sh, dt=torch.float32: torch.zeros(sh, dtype=dt, device=self.dev)  # noqa: E731
            t = dict(status=z(P, S, dt=torch.int8), pos3=z(P, S, 3), pos=z(P * S, 3), normal=z(P * S, 3),
                     min_dist=z(P * S), max_dist=z(P * S), desc=z(P * S, 32, dt=torch.uint8),
                     flags=z(P * S, dt=torch.uint8), feat1=z(P * S, dt=torch.int32), feat2=z(P * S, dt=torch.int32),
                     ranges=z(P, 2, dt=torch.int32), nnew=z(P, dt=torch.int32))
            self._new_mp = t
        st = self.stream_ptr() if stream is None else stream
        g = self.tri_geom()
        check(self.lib.orbm_create_new_map_points_batch_device(
            self.mh, P, q1.data_ptr(), q2.data_ptr(), self.B, self.kps_un.data_ptr(), self.counts.data_ptr(), S,
            self.uright.data_ptr() if self.stereo else None, self.depth.data_ptr() if self.stereo else None,
            self.desc.data_ptr(), poses.data_ptr(), match.data_ptr(), C.byref(g), 0 if self.stereo else 1,
            median_depth2.data_ptr() if median_depth2 is not None else None, t["status"].data_ptr(),
            t["pos3"].data_ptr(), t["pos"].data_ptr(), t["normal"].data_ptr(), t["min_dist"].data_ptr(),
            t["max_dist"].data_ptr(), t["desc"].data_ptr(), t["flags"].data_ptr(), t["feat1"].data_ptr(),
            t["feat2"].data_ptr(), t["ranges"].data_ptr(), t["nnew"].data_ptr(), st),
            "orbm_create_new_map_points_batch_device")
        return t

    # ---- pose optimisation (include/orbslam_amd.h "Pose optimisation") ----
    def inv_level_sigma2(self):
        """mvInvLevelSigma2 of the pipeline's extractor: 1.0f / mvLevelSigma2[i] (ORBextractor.cc:432)"""
        return (np.float32(1.0) / np.asarray(self.sigma2, np.float32)).astype(np.float32)

    def optimize_pose(self, poses, pos, mp_index=None, pairs=None, local=None, frames=None, poses_out=None,
                      mp_flags=None, frame_mp=None, out=None, stream=None):
        """Optimizer::PoseOptimization (Optimizer.cc:239-451) of one job per entry of frames (int32 cuda [njobs],
        default frames 0..B-1) over the pipeline's own kps_un, counts and (stereo) uright: poses float32 cuda
        [B, 4, 4] (mTcw), pos float32 cuda [M, 3] (or [B, stride, 3]) = the MapPoint positions, and each feature's
        MapPoint as one of
          mp_index  int32 cuda [njobs, stride]: the row of pos, or negative;
          pairs     (match, last): a track_pairs result, match[p, i] = the last-frame feature, last int32 [njobs]:
                    the row is last[p] * stride + match where match >= 0, else -1 (built with torch ops on the stream);
          local     a track_local result (frame_mp merged with its matches): the row is the entry itself.
        poses_out (default: poses, in place -- only with the default frames, where job j is frame j) receives the
        optimised poses. With mp_flags (uint8 [njobs, stride]) bit 2 becomes the outlier flag; with frame_mp (int32
        [njobs, stride]) an outlier's entry becomes -1 (Tracking's discard loop). Returns a dict of cuda tensors:
        poses, outlier uint8 [njobs, stride], ninliers, nmatches_map int32 [njobs], status int8 [njobs], mp_index.
        Only enqueues. Every call returns output tensors of its own, so an earlier result stays valid; out = the dict
        of an earlier call with the same job count writes into that call's tensors again (a steady-state loop that
        wants no allocation)."""
        torch = self.torch
        S = self.stride
        st = self.stream_ptr() if stream is None else stream
        if frames is None:
            frames = self.q1
            poses_out = poses if poses_out is None else poses_out
        elif poses_out is None:
            raise RuntimeError("a job list of its own needs poses_out")
        J = int(frames.numel())
        if pairs is not None:
            match, last = pairs
            mp_index = torch.where(match >= 0, last.to(torch.int32).view(-1, 1) * S + match,
                                   torch.full_like(match, -1)).contiguous()
        elif local is not None:
            mp_index = local.contiguous()
        if mp_index is None:
            raise RuntimeError("one of mp_index, pairs, local")
        if frame_mp is True:
            frame_mp = mp_index.clone()
        if out is not None:
            t = dict((k, out[k]) for k in ("outlier", "ninliers", "nmatches_map", "status"))
            if t["status"].shape[0] != J:
                raise RuntimeError("out belongs to another job count")
        else:
            z = lambda *sh, dt=torch.int32: torch.zeros(sh, dtype=dt, device=self.dev)  # noqa: E731
            t = dict(outlier=z(J, S, dt=torch.uint8), ninliers=z(J), nmatches_map=z(J), status=z(J, dt=torch.int8))
        g = self.track_geom()
        inv = np.zeros(16, np.float32)
        inv[:len(self.sigma2)] = self.inv_level_sigma2()
        pos2 = pos.view(-1, 3)
        check(self.lib.orbm_pose_optimization_batch_device(
            self.mh, J, frames.data_ptr(), self.B, self.kps_un.data_ptr(), self.counts.data_ptr(), S,
            self.uright.data_ptr() if self.stereo else None, C.byref(g), inv.ctypes.data, mp_index.data_ptr(),
            pos2.data_ptr(), int(pos2.shape[0]), poses.data_ptr(), poses_out.data_ptr(), t["outlier"].data_ptr(),
            mp_flags.data_ptr() if mp_flags is not None else None,
            frame_mp.data_ptr() if frame_mp is not None else None, t["ninliers"].data_ptr(),
            t["nmatches_map"].data_ptr(), t["status"].data_ptr(), st), "orbm_pose_optimization_batch_device")
        return dict(t, poses=poses_out, mp_index=mp_index, frame_mp=frame_mp)

    def step(self, frames, stream=None):
        self.extract(frames, stream)
        self.match_pairs(stream)

    # ---- cross-agent exchange (include/orbslam_amd.h "Cross-agent keyframe slot") ----
    def slot_bytes(self):
        return int(self.lib.orbx_slot_bytes(self.stride))

    def meta(self, frame_idx=0, agent=0):
        """orbx_kf_meta of frame frame_idx as a keyframe of agent `agent` (camera of my.yaml, the
        extractor's scale tables, identity pose)."""
        from .exchange import make_meta
        inv = self.ext.GetInverseScaleSigmaSquares()
        K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]], np.float32)
        return make_meta(agent=agent, mnId=frame_idx, nlevels=len(self.scale), scale=self.scale, sigma2=self.sigma2,
                         inv_sigma2=inv, scale_factor=self.ext.GetScaleFactor(), K=K, width=self.W, height=self.H)

    def kf_source(self, frame_idx, with_bow=False, uright=None, depth=None, mp_flags=None, mp_pos=None):
        """orbx_kf_source of frame frame_idx's device arrays (its BoW / FeatureVector from bow() with
        with_bow; optional per-keypoint uright/depth/MapPoint device tensors)."""
        from .exchange import kf_source
        f, S = frame_idx, self.stride
        if self.stereo and uright is None:  # a stereo keyframe carries its mvuRight / mvDepth
            uright, depth = self.uright[f], self.depth[f]
        kw = {}
        if with_bow:
            kw = dict(bow_word=self.bow_word[f], bow_value=self.bow_val[f], nbow=self.nbow[f:f + 1],
                      fv_node=self.fv_node[f], fv_off=self.fv_off[f], fv_feat=self.fv_feat[f], nfv=self.nfv[f:f + 1])
        kun = self.kun[f] if self.kun is not None else None  # a distorted camera: the slot carries mvKeysUn (KUN)
        return kf_source(self.kps[f], self.desc[f], self.counts[f:f + 1], kun=kun, uright=uright, depth=depth,
                         mp_flags=mp_flags, mp_pos=mp_pos, **kw)

    def pack(self, frame_idx, slot, meta, stream=None, with_bow=False, err=None, src=None):
        """orbx_pack_keyframe_device of frame frame_idx into the device slot."""
        from .exchange import pack_device
        st = self.stream_ptr() if stream is None else stream
        src = self.kf_source(frame_idx, with_bow) if src is None else src
        pack_device(src, meta, self.stride, slot, err, st)

    def match_slots(self, frame_idx, slots, nref, out_match, out_n, stream=None, use_bow=False, geoms=None,
                    query=None):
        """Cross-agent SearchForTriangulation of frame frame_idx against nref received slots
        (orbm_search_for_triangulation_slots_device); geoms = per-slot (F12, ex, ey), default the bench
        geometry for every slot."""
        from .exchange import match_slots_device, slot_geoms
        st = self.stream_ptr() if stream is None else stream
        if geoms is None:
            if getattr(self, "_geo_cache", (None, None))[0] != nref:
                self._geo_cache = (nref, slot_geoms([(self.F12, self.ex, self.ey)] * nref))
            geoms = self._geo_cache[1]
        q = self.kf_source(frame_idx, use_bow) if query is None else query
        match_slots_device(self.mh, q, self.stride, nref, slots, self.slot_bytes(), geoms, out_match, out_n,
                           use_bow=use_bow, max_nodes=getattr(self, "max_nodes", 0) if use_bow else 0, stream=st)

    def check_match_error(self, stream=None):
        st = self.stream_ptr() if stream is None else stream
        check(self.lib.orbm_check_error(self.mh, st), "orbm_check_error")

    def host_results(self, b):
        """(keypoints structured array, descriptors uint8 [n,32], match12 int32 [n]) of frame b (stereo: its left
        image)."""
        k, d = self.host_keypoints(b)
        m = self.match[b, :len(k)].cpu().numpy()
        return k, d, m

    def host_keypoints(self, i):
        """(keypoints, descriptors) of extraction image i (stereo: i >= B is the right image of frame i - B)"""
        from .extractor import kp_dtype
        n = int(self.counts[i].item())
        k = self.kps[i, :n].cpu().numpy().copy().view(np.uint8).view(kp_dtype).reshape(n)
        d = self.desc[i, :n].cpu().numpy()
        return k, d

    def host_keypoints_un(self, i):
        """mvKeysUn of extraction image i (Frame::UndistortKeyPoints; equal to its keypoints without a camera)"""
        from .extractor import kp_dtype
        n = int(self.counts[i].item())
        return self.kps_un[i, :n].cpu().numpy().copy().view(np.uint8).view(kp_dtype).reshape(n)

    def host_stereo(self, b):
        """(mvuRight float32 [n], mvDepth float32 [n], stereo matches kept) of stereo frame b"""
        n = int(self.counts[b].item())
        return (self.uright[b, :n].cpu().numpy(), self.depth[b, :n].cpu().numpy(), int(self.nstereo[b].item()))

    def close(self):
        if getattr(self, "mh", None):
            self.lib.orbm_destroy(self.mh)
            self.mh = None
        self.ext.close()

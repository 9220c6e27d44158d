"""Frame-level consumers of the extractor output over the C ABI.

* :func:`compute_stereo_matches` -- ``Frame::ComputeStereoMatches``
  (ORB_SLAM2.1/src/Frame.cc:470-641): mvuRight / mvDepth of the left keypoints, from the two
  extractors' device-resident pyramids.
* :func:`undistort_points`, :func:`undistort_keypoints`, :func:`image_bounds` --
  ``Frame::UndistortKeyPoints`` (Frame.cc:405-435) and ``Frame::ComputeImageBounds`` (Frame.cc:437-465, with the
  grid cell sizes of Frame.cc:213-214) on the host; the device batch form is
  ``ORBextractor.undistort_batch_device``.
* :func:`unproject_stereo` -- ``Frame::UnprojectStereo`` (Frame.cc:667-681) of a frame's keypoints on the host; the
  device batch form is ``BatchPipeline.unproject``. :func:`track_geom` builds the ``orbm_track_geom`` of
  ``BatchPipeline.track_pairs``.
* :func:`is_in_frustum` -- ``Frame::isInFrustum`` (Frame.cc:274-330, with ``MapPoint::PredictScale``) of a table of
  MapPoints on the host; the device batch forms are ``BatchPipeline.frustum`` and, inside
  ``Tracking::SearchLocalPoints``, ``BatchPipeline.track_local``.
"""
import ctypes as C

import numpy as np

from ._lib import KP_FIELDS, OrbmTrackGeom, OrbmTriGeom, OrbxCamera, check, load


def compute_stereo_matches(left, right, kpsL, descL, kpsR, descR, mbf, mb):
    """left/right: the two ORBextractor instances whose latest call produced (kpsL, descL) and
    (kpsR, descR). Returns (mvuRight float32 [N], mvDepth float32 [N], number of stereo matches)."""
    lib = load()
    nL, nR = len(kpsL), len(kpsR)
    kpsL = np.ascontiguousarray(kpsL)
    kpsR = np.ascontiguousarray(kpsR)
    dL = np.ascontiguousarray(descL if descL is not None else np.zeros((0, 32), np.uint8))
    dR = np.ascontiguousarray(descR if descR is not None else np.zeros((0, 32), np.uint8))
    ur = np.full(nL, -1.0, np.float32)
    dp = np.full(nL, -1.0, np.float32)
    ns = C.c_int(0)
    check(lib.orbx_compute_stereo_matches(left._h, right._h, kpsL.ctypes.data, dL.ctypes.data, nL, kpsR.ctypes.data,
                                          dR.ctypes.data, nR, float(mbf), float(mb), ur.ctypes.data, dp.ctypes.data,
                                          C.byref(ns)), "orbx_compute_stereo_matches")
    return ur, dp, ns.value


def stereo_matches_batch_device(left, right, fl, fr, kpsL, descL, cntL, kpsR, descR, cntR, mbf, mb, uright, depth,
                                nstereo, stream=0):
    """Device batch form (torch tensors): pair p = frame fl[p] of left's latest batch with frame fr[p] of
    right's. kps [B, stride, 6], desc [B, stride, 32], counts [B]; outputs uright/depth [P, stride], nstereo [P]."""
    lib = load()
    stride = descL.shape[1]
    check(lib.orbx_stereo_matches_batch_device(
        left._h, right._h, fl.shape[0], fl.data_ptr(), fr.data_ptr(), kpsL.data_ptr(), descL.data_ptr(),
        cntL.data_ptr(), kpsR.data_ptr(), descR.data_ptr(), cntR.data_ptr(), stride, float(mbf), float(mb),
        uright.data_ptr(), depth.data_ptr(), nstereo.data_ptr(), stream), "orbx_stereo_matches_batch_device")


def make_camera(camera):
    """orbx_camera from an OrbxCamera, a mapping with the keys fx, fy, cx, cy, k1, k2, p1, p2[, k3] or a sequence
    (fx, fy, cx, cy, k1, k2, p1, p2[, k3]); k3 = 0 for a 4-entry mDistCoef."""
    if isinstance(camera, OrbxCamera):
        return camera
    names = [k for k, _ in OrbxCamera._fields_]
    if hasattr(camera, "keys"):
        vals = [float(camera[k]) if k in camera.keys() else 0.0 for k in names]
        if not all(k in camera.keys() for k in names[:8]):
            raise ValueError("camera needs fx, fy, cx, cy, k1, k2, p1, p2")
    else:
        vals = [float(v) for v in camera]
        if len(vals) not in (8, 9):
            raise ValueError("camera = (fx, fy, cx, cy, k1, k2, p1, p2[, k3])")
        vals += [0.0] * (9 - len(vals))
    return OrbxCamera(*vals)


def undistort_points(camera, xy):
    """The cv::undistortPoints call of Frame::UndistortKeyPoints (Frame.cc:423) with its k1 == 0 copy: xy float32
    [n, 2] -> float32 [n, 2]."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.empty_like(xy)
    cam = make_camera(camera)
    check(load().orbx_undistort_points(C.byref(cam), len(xy), xy.ctypes.data, out.ctypes.data),
          "orbx_undistort_points")
    return out


def undistort_keypoints(camera, kps):
    """Frame::UndistortKeyPoints (Frame.cc:405-435): mvKeysUn of the keypoints (structured array of kp_dtype)."""
    kps = np.ascontiguousarray(kps, np.dtype(KP_FIELDS))
    out = np.empty_like(kps)
    cam = make_camera(camera)
    check(load().orbx_undistort_keypoints(C.byref(cam), len(kps), kps.ctypes.data, out.ctypes.data),
          "orbx_undistort_keypoints")
    return out


def image_bounds(camera, cols, rows):
    """Frame::ComputeImageBounds (Frame.cc:437-465) and Frame.cc:213-214: ((mnMinX, mnMaxX, mnMinY, mnMaxY) float32
    [4], mfGridElementWidthInv, mfGridElementHeightInv as numpy float32)."""
    b = np.empty(4, np.float32)
    gw, gh = C.c_float(), C.c_float()
    cam = make_camera(camera)
    check(load().orbx_image_bounds(C.byref(cam), int(cols), int(rows), b.ctypes.data, C.byref(gw), C.byref(gh)),
          "orbx_image_bounds")
    return b, np.float32(gw.value), np.float32(gh.value)


def unproject_stereo(camera, Tcw, kps_un, depth):
    """Frame::UnprojectStereo (Frame.cc:667-681) of every keypoint: kps_un = mvKeysUn (structured array of kp_dtype),
    depth = mvDepth float32 [n], Tcw = mTcw 4x4. Returns (pos float32 [n, 3], valid uint8 [n]); z <= 0 gives three
    zeros and valid 0. Only fx, fy, cx, cy of the camera are read."""
    kps = np.ascontiguousarray(kps_un, np.dtype(KP_FIELDS))
    n = len(kps)
    depth = np.ascontiguousarray(depth, np.float32).reshape(n)
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    pos = np.empty((n, 3), np.float32)
    valid = np.empty(n, np.uint8)
    cam = make_camera(camera)
    check(load().orbx_unproject_stereo(C.byref(cam), T.ctypes.data, n, kps.ctypes.data, depth.ctypes.data,
                                       pos.ctypes.data, valid.ctypes.data), "orbx_unproject_stereo")
    return pos, valid


def track_geom(fx, fy, cx, cy, bf, b, bounds, grid_w_inv, grid_h_inv, scale_factors):
    """orbm_track_geom: camera, mbf, mb, (mnMinX, mnMaxX, mnMinY, mnMaxY) and the grid inverses as image_bounds returns
    them, mvScaleFactors."""
    s = np.asarray(scale_factors, np.float32)
    if not 1 <= len(s) <= 16:
        raise ValueError("1 to 16 scale factors")
    g = OrbmTrackGeom()
    g.fx, g.fy, g.cx, g.cy, g.bf, g.b = (float(np.float32(v)) for v in (fx, fy, cx, cy, bf, b))
    g.min_x, g.max_x, g.min_y, g.max_y = (float(np.float32(v)) for v in bounds)
    g.grid_w_inv, g.grid_h_inv = float(np.float32(grid_w_inv)), float(np.float32(grid_h_inv))
    g.nlevels = len(s)
    for i, v in enumerate(s):
        g.scale_factors[i] = float(v)
    return g


def tri_geom(fx, fy, cx, cy, bf, b, scale_factors, level_sigma2):
    """orbm_tri_geom: camera, mbf, mb, mvScaleFactors and mvLevelSigma2 (1 to 16 levels) of both keyframes."""
    s = np.asarray(scale_factors, np.float32)
    q = np.asarray(level_sigma2, np.float32)
    if not 1 <= len(s) <= 16 or len(q) != len(s):
        raise ValueError("1 to 16 scale factors and as many sigma2")
    g = OrbmTriGeom()
    g.fx, g.fy, g.cx, g.cy, g.bf, g.b = (float(np.float32(v)) for v in (fx, fy, cx, cy, bf, b))
    g.nlevels = len(s)
    for i in range(len(s)):
        g.scale_factors[i], g.level_sigma2[i] = float(s[i]), float(q[i])
    return g


class NewMapPoints:
    """what orbx_triangulate_matches writes for one pair: status int8 [n1] (ORBM_TRI_*), pos3 float32 [n1, 3], and
    the nnew new MapPoints in idx1 order: tab_pos, tab_normal [nnew, 3], tab_min, tab_max [nnew], tab_desc uint8
    [nnew, 32], tab_flags uint8 [nnew], feat1, feat2 int32 [nnew]"""
    FIELDS = ("status", "pos3", "tab_pos", "tab_normal", "tab_min", "tab_max", "tab_desc", "tab_flags", "feat1",
              "feat2")


def triangulate_matches(geom, monocular, median_depth2, Tcw1, Tcw2, kps1, uright1, depth1, desc1, kps2, uright2,
                        depth2, match12):
    """The per-match body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:284-450, with the baseline test of
    :244-261 and MapPoint::UpdateNormalAndDepth) for one pair on the host: geom = an orbm_tri_geom (tri_geom), kps =
    mvKeysUn (structured arrays of kp_dtype), uright / depth = mvuRight / mvDepth float32 or None (monocular), desc1
    uint8 [n1, 32], match12 int32 [n1] = idx2 or negative. Returns a NewMapPoints. F12 and the epipole of the matcher
    before it are orbamd.matcher.compute_f12 / epipole."""
    kps1 = np.ascontiguousarray(kps1, np.dtype(KP_FIELDS))
    kps2 = np.ascontiguousarray(kps2, np.dtype(KP_FIELDS))
    n1, n2 = len(kps1), len(kps2)
    f = lambda a, n: None if a is None else np.ascontiguousarray(a, np.float32).reshape(n)  # noqa: E731
    ur1, d1, ur2, d2 = f(uright1, n1), f(depth1, n1), f(uright2, n2), f(depth2, n2)
    desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(n1, 32)
    m = np.ascontiguousarray(match12, np.int32).reshape(n1)
    T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
    T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    r = NewMapPoints()
    r.status, r.pos3 = np.zeros(n1, np.int8), np.zeros((n1, 3), np.float32)
    r.tab_pos, r.tab_normal = np.zeros((n1, 3), np.float32), np.zeros((n1, 3), np.float32)
    r.tab_min, r.tab_max = np.zeros(n1, np.float32), np.zeros(n1, np.float32)
    r.tab_desc, r.tab_flags = np.zeros((n1, 32), np.uint8), np.zeros(n1, np.uint8)
    r.feat1, r.feat2 = np.zeros(n1, np.int32), np.zeros(n1, np.int32)
    nnew = C.c_int(0)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    check(load().orbx_triangulate_matches(
        C.byref(geom), int(bool(monocular)), float(median_depth2), T1.ctypes.data, T2.ctypes.data, n1, p(kps1), p(ur1),
        p(d1), p(desc1), n2, p(kps2), p(ur2), p(d2), p(m), p(r.status), p(r.pos3), p(r.tab_pos), p(r.tab_normal),
        p(r.tab_min), p(r.tab_max), p(r.tab_desc), p(r.tab_flags), p(r.feat1), p(r.feat2), C.byref(nnew)),
        "orbx_triangulate_matches")
    r.nnew = nnew.value
    for k in NewMapPoints.FIELDS[2:]:
        setattr(r, k, getattr(r, k)[:r.nnew])
    return r


def is_in_frustum(geom, log_scale_factor, Tcw, pos, normal, min_dist, max_dist, viewing_cos_limit=0.5):
    """Frame::isInFrustum (Frame.cc:274-330) of n MapPoints under the pose Tcw (mTcw 4x4): geom = an orbm_track_geom
    (track_geom), log_scale_factor = mfLogScaleFactor, pos / normal float32 [n, 3], min_dist / max_dist float32 [n] (the
    raw mfMinDistance / mfMaxDistance). Returns the six tracking arrays of MapPoints: (in_view uint8, proj_x, proj_y,
    proj_xr float32, level int32, view_cos float32), each [n]; a rejected point has in_view 0 and zeros."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    normal = np.ascontiguousarray(normal, np.float32).reshape(n, 3)
    mind = np.ascontiguousarray(min_dist, np.float32).reshape(n)
    maxd = np.ascontiguousarray(max_dist, np.float32).reshape(n)
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    in_view = np.empty(n, np.uint8)
    x, y, xr, vc = (np.empty(n, np.float32) for _ in range(4))
    level = np.empty(n, np.int32)
    check(load().orbx_is_in_frustum(C.byref(geom), float(log_scale_factor), T.ctypes.data, float(viewing_cos_limit), n,
                                    pos.ctypes.data, normal.ctypes.data, mind.ctypes.data, maxd.ctypes.data,
                                    in_view.ctypes.data, x.ctypes.data, y.ctypes.data, xr.ctypes.data,
                                    level.ctypes.data, vc.ctypes.data), "orbx_is_in_frustum")
    return in_view, x, y, xr, level, vc


class PoseResult:
    """what orbx_pose_optimization writes for one frame: Tcw float32 [4, 4], outlier uint8 [n] (mvbOutlier; a feature
    without a MapPoint keeps the byte it came in with), ninliers, status (ORBM_POSE_*: 0 ok, 1 too few, 2 excluded)
    and diag int32 [8] (rounds, iterations per round, rejected trials, failed solves, small-angle exps)"""


def pose_optimization(geom, inv_level_sigma2, Tcw, kps_un, uright, mp_index, pos, outlier=None):
    """Optimizer::PoseOptimization (Optimizer.cc:239-451) of one frame on the host: geom = an orbm_track_geom
    (track_geom; fx, fy, cx, cy, bf are read), inv_level_sigma2 = mvInvLevelSigma2 (1 to 16 floats), Tcw = mTcw 4x4,
    kps_un = mvKeysUn (kp_dtype), uright = mvuRight float32 [n] or None (monocular), mp_index int32 [n] = the row of
    each feature's MapPoint in pos (float32 [M, 3]) or negative, outlier = the incoming mvbOutlier (default zeros).
    Returns a PoseResult."""
    kps = np.ascontiguousarray(kps_un, np.dtype(KP_FIELDS))
    n = len(kps)
    inv = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    ur = None if uright is None else np.ascontiguousarray(uright, np.float32).reshape(n)
    mp = np.ascontiguousarray(mp_index, np.int32).reshape(n)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    r = PoseResult()
    r.Tcw = np.array(Tcw, np.float32).reshape(16).copy()
    r.outlier = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(n).copy()
    r.diag = np.zeros(8, np.int32)
    ninl, st = C.c_int(0), C.c_int(0)
    inv16 = np.zeros(16, np.float32)
    inv16[:min(len(inv), 16)] = inv[:16]
    check(load().orbx_pose_optimization(
        C.byref(geom), inv16.ctypes.data, len(inv), r.Tcw.ctypes.data, n, kps.ctypes.data,
        None if ur is None else ur.ctypes.data, mp.ctypes.data, pos.ctypes.data, r.outlier.ctypes.data, C.byref(ninl),
        C.byref(st), r.diag.ctypes.data), "orbx_pose_optimization")
    r.Tcw = r.Tcw.reshape(4, 4)
    r.ninliers, r.status = ninl.value, st.value
    return r

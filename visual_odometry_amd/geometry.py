"""cv2.findEssentialMat / recoverPose / triangulatePoints look-alikes backed by HIP kernels
(reference call sites: src/image_pair.py:280-286, :304-308, :332-336)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

RANSAC = FM_RANSAC = 8
OPENCV_RNG_SEED = 0xFFFFFFFFFFFFFFFF


def _pts(p):
    p = np.ascontiguousarray(p, dtype=np.float64)
    if p.ndim == 3 and p.shape[1] == 1:
        p = p.reshape(-1, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("points must be an M x 2 array")
    return np.ascontiguousarray(p)


def findEssentialMat(points1, points2, cameraMatrix, method=RANSAC, prob=0.999, threshold=1.0, maxIters=1000,
                     seed=OPENCV_RNG_SEED, ctx=None):
    """Returns (E 3x3 float64, mask Mx1 uint8); (None, None) for fewer than 5 points, as cv2 does."""
    if method != RANSAC:
        raise NotImplementedError("only RANSAC (cv2.FM_RANSAC) is implemented")
    p1, p2 = _pts(points1), _pts(points2)
    if len(p1) != len(p2):
        raise ValueError("point sets differ in length")
    K = np.ascontiguousarray(cameraMatrix, dtype=np.float64).reshape(3, 3)
    M = len(p1)
    if M < 5:
        return None, None
    ctx = ctx or _lib.default_context()
    E = np.zeros((10, 9)); mask = np.zeros(M, np.uint8)
    ninl = C.c_int32(0); nmod = C.c_int32(0)
    rc = ctx.lib.vo_find_essential_ransac(ctx.handle, p1.ctypes.data, p2.ctypes.data, M, K.ctypes.data, float(prob),
                                          float(threshold), int(maxIters), int(seed), E.ctypes.data, mask.ctypes.data,
                                          C.addressof(ninl), C.addressof(nmod))
    if rc == _lib.VO_ERR_NO_MODEL:
        return None, None
    ctx.check(rc)
    return E[:nmod.value].reshape(-1, 3).copy(), mask.reshape(-1, 1)


def recoverPose(E, points1, points2, cameraMatrix, distanceThresh=50.0, ctx=None):
    """Returns (n_good, R 3x3, t 3x1, mask Mx1 with 0/255)."""
    E = np.ascontiguousarray(E, dtype=np.float64)
    if E.shape != (3, 3):
        raise ValueError("E must be 3x3")
    p1, p2 = _pts(points1), _pts(points2)
    K = np.ascontiguousarray(cameraMatrix, dtype=np.float64).reshape(3, 3)
    M = len(p1)
    ctx = ctx or _lib.default_context()
    R = np.zeros((3, 3)); t = np.zeros((3, 1)); mask = np.zeros(max(M, 1), np.uint8); ng = C.c_int32(0)
    ctx.check(ctx.lib.vo_recover_pose(ctx.handle, E.ctypes.data, p1.ctypes.data, p2.ctypes.data, M, K.ctypes.data,
                                      float(distanceThresh), R.ctypes.data, t.ctypes.data, mask.ctypes.data,
                                      C.addressof(ng)))
    return ng.value, R, t, mask[:M].reshape(-1, 1)


def triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2, ctx=None):
    """Returns the 4 x M homogeneous points (not normalised), float64."""
    P1 = np.ascontiguousarray(projMatr1, dtype=np.float64).reshape(3, 4)
    P2 = np.ascontiguousarray(projMatr2, dtype=np.float64).reshape(3, 4)
    x1 = np.ascontiguousarray(projPoints1, dtype=np.float64)
    x2 = np.ascontiguousarray(projPoints2, dtype=np.float64)
    if x1.ndim != 2 or x1.shape[0] != 2 or x1.shape != x2.shape:
        raise ValueError("projPoints must be 2 x M arrays of equal shape")
    M = x1.shape[1]
    X = np.zeros((4, M))
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_triangulate(ctx.handle, P1.ctypes.data, P2.ctypes.data, x1.ctypes.data, x2.ctypes.data, M,
                                     X.ctypes.data))
    return X


_EPILINE_TYPES = {np.dtype(np.float64): (0, np.float64), np.dtype(np.float32): (1, np.float32), np.dtype(np.int32): (2, np.float32)}


def epiline_points(points):
    """The N x 2 array computeCorrespondEpilines reads from `points` (N x 2, N x 1 x 2, 1 x N x 2 or a list of pairs) and its
    vo_correspond_epilines point_type.  float64, float32 and int32 keep their depth; a list and any other dtype go to float64."""
    p = np.asarray(points)
    if p.dtype not in _EPILINE_TYPES:
        p = p.astype(np.float64)
    if p.ndim == 3 and 1 in p.shape[:2]:
        p = p.reshape(-1, p.shape[2])
    if p.size == 0:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] not in (2, 3):
        raise ValueError("points must be an N x 2 array")
    if p.shape[1] == 3:
        raise NotImplementedError("homogeneous (three-column) points are not built (the reference passes keypoint.pt pairs)")
    return np.ascontiguousarray(p), _EPILINE_TYPES[p.dtype]


def computeCorrespondEpilines(points, whichImage, F, ctx=None):
    """cv2.computeCorrespondEpilines(points, whichImage, F) (src/feature_detection.py:118-125) -> lines [N, 1, 3]: float64 for
    float64 points, float32 for float32 and int32 points."""
    p, (ptype, out_dtype) = epiline_points(points)
    if whichImage not in (1, 2):
        raise ValueError("whichImage must be 1 or 2")
    Fm = np.ascontiguousarray(F, dtype=np.float64)
    if Fm.shape != (3, 3):
        raise ValueError("F must be 3x3")
    N = len(p)
    lines = np.zeros((max(N, 1), 3), out_dtype)
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_correspond_epilines(ctx.handle, p.ctypes.data, N, ptype, int(whichImage), Fm.ctypes.data, lines.ctypes.data))
    return lines[:N].reshape(N, 1, 3)


def dist_coeffs(distCoeffs):
    """cv2's distCoeffs argument as the C ABI takes it: a flat float64 array; None or an empty array is four zeros."""
    d = np.zeros(4) if distCoeffs is None else np.ascontiguousarray(distCoeffs, dtype=np.float64).ravel()
    return np.zeros(4) if d.size == 0 else d


def undistortPoints(src, cameraMatrix, distCoeffs, R=None, P=None, ctx=None):
    """cv2.undistortPoints(src, cameraMatrix, distCoeffs, R, P) with its default termination (five iterations) -> [N, 1, 2] of
    src's float type.  src: [N, 2], [N, 1, 2] or [1, N, 2], float32 or float64 (anything else is read as float64); distCoeffs:
    4, 5 or 8 values (k1 k2 p1 p2 [k3 [k4 k5 k6]]), None or empty = zeros; 12 and 14 (thin prism, tilt) raise
    NotImplementedError.  R: 3x3 or None; P: 3x3 or 3x4 (its left 3x3 is used, as cv2 does) or None: normalised coordinates come
    back.  The lens model the reference carries in src/image_and_keypoints.py:21-25 and never applies."""
    p = np.asarray(src)
    if p.dtype not in (np.float32, np.float64):
        p = p.astype(np.float64)
    if p.ndim == 3 and 1 in p.shape[:2]:
        p = p.reshape(-1, p.shape[2])
    if p.size == 0:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("src must be an N x 2, N x 1 x 2 or 1 x N x 2 array")
    p = np.ascontiguousarray(p)
    K = np.ascontiguousarray(cameraMatrix, dtype=np.float64).reshape(3, 3)
    d = dist_coeffs(distCoeffs)
    Rm = None if R is None else np.ascontiguousarray(np.asarray(R, np.float64).reshape(3, 3))
    Pm = None
    if P is not None:
        Pm = np.asarray(P, np.float64)
        if Pm.shape not in ((3, 3), (3, 4)):
            raise ValueError("P must be 3x3 or 3x4")
        Pm = np.ascontiguousarray(Pm[:, :3])
    N = len(p)
    out = np.zeros((max(N, 1), 2), p.dtype)
    ctx = ctx or _lib.default_context()
    rc = ctx.lib.vo_undistort_points(ctx.handle, p.ctypes.data, N, 0 if p.dtype == np.float64 else 1, K.ctypes.data, d.ctypes.data, len(d),
                                     _lib.ptr(Rm), _lib.ptr(Pm), out.ctypes.data)
    if rc == _lib.VO_ERR_UNSUPPORTED:
        raise NotImplementedError(ctx.last_error())
    ctx.check(rc)
    return out[:N].reshape(N, 1, 2)


def five_point(x1, x2, ctx=None):
    """All essential matrices through 5 normalised correspondences (stage test hook)."""
    x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(5, 2)
    x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(5, 2)
    E = np.zeros((10, 9)); n = C.c_int32(0)
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_stage_five_point(ctx.handle, x1.ctypes.data, x2.ctypes.data, E.ctypes.data, C.addressof(n)))
    return E[:n.value].reshape(-1, 3, 3).copy()


SOLVEPNP_ITERATIVE = 0


def solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs=None, useExtrinsicGuess=False, iterationsCount=100,
                   reprojectionError=8.0, confidence=0.99, flags=SOLVEPNP_ITERATIVE, seed=OPENCV_RNG_SEED, ctx=None):
    """cv2.solvePnPRansac as the reference calls it (src/visual_slam.py:231-235: positional objectPoints, imagePoints,
    cameraMatrix, zeros(4)) -> (retval, rvec 3x1, tvec 3x1, inliers n_inl x 1 int32 indices or None).
    Only the reference's configuration is built: zero distortion, no extrinsic guess, SOLVEPNP_ITERATIVE.
    A camera with a real lens: undistort the image points first (undistortPoints with P = cameraMatrix, or FrontEnd.undistort on
    resident keypoints) and pass zeros here.  That is not what cv2 computes with non-zero distCoeffs — cv2 measures the RANSAC
    error in distorted pixels — so non-zero coefficients stay refused instead of being rerouted."""
    if distCoeffs is not None and np.any(np.asarray(distCoeffs, np.float64) != 0):
        raise NotImplementedError("only zero distortion coefficients are built (the reference passes np.zeros(4))")
    if useExtrinsicGuess or flags != SOLVEPNP_ITERATIVE:
        raise NotImplementedError("only cv2.solvePnPRansac's defaults (no extrinsic guess, SOLVEPNP_ITERATIVE) are built")
    obj = np.ascontiguousarray(np.asarray(objectPoints, np.float64).reshape(-1, 3))
    img = np.ascontiguousarray(np.asarray(imagePoints, np.float64).reshape(-1, 2))
    if len(obj) != len(img):
        raise ValueError("objectPoints and imagePoints differ in length")
    K = np.ascontiguousarray(cameraMatrix, np.float64).reshape(3, 3)
    n = len(obj)
    rvec = np.zeros((3, 1)); tvec = np.zeros((3, 1)); mask = np.zeros(max(n, 1), np.uint8); ninl = C.c_int32(0)
    ctx = ctx or _lib.default_context()
    rc = ctx.lib.vo_solve_pnp_ransac(ctx.handle, obj.ctypes.data, img.ctypes.data, n, K.ctypes.data, int(iterationsCount),
                                     float(reprojectionError), float(confidence), int(seed), rvec.ctypes.data, tvec.ctypes.data,
                                     mask.ctypes.data, C.addressof(ninl))
    if rc == _lib.VO_ERR_NO_MODEL:
        return False, rvec, tvec, None                     # cv2: retval False
    ctx.check(rc)                                          # n < 4 raises, as cv2's assertion does
    return True, rvec, tvec, np.nonzero(mask[:n])[0].astype(np.int32).reshape(-1, 1)


def solve_pnp_ransac_batch(objectPoints, imagePoints, offsets, cameraMatrix, iterationsCount=100, reprojectionError=8.0,
                           confidence=0.99, seed=OPENCV_RNG_SEED, ctx=None):
    """B independent solvePnPRansac problems in one launch; problem b owns rows offsets[b]:offsets[b+1].
    Returns (status [B], rvec [B, 3], tvec [B, 3], mask [total] uint8, n_inliers [B])."""
    obj = np.ascontiguousarray(np.asarray(objectPoints, np.float64).reshape(-1, 3))
    img = np.ascontiguousarray(np.asarray(imagePoints, np.float64).reshape(-1, 2))
    off = np.ascontiguousarray(offsets, np.int32)
    B = len(off) - 1
    K = np.ascontiguousarray(cameraMatrix, np.float64).reshape(3, 3)
    rvec = np.zeros((B, 3)); tvec = np.zeros((B, 3)); mask = np.zeros(max(len(obj), 1), np.uint8)
    ninl = np.zeros(B, np.int32); status = np.zeros(B, np.int32)
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_solve_pnp_ransac_batch(ctx.handle, obj.ctypes.data, img.ctypes.data, off.ctypes.data, B, K.ctypes.data,
                                                int(iterationsCount), float(reprojectionError), float(confidence), int(seed),
                                                rvec.ctypes.data, tvec.ctypes.data, mask.ctypes.data, ninl.ctypes.data,
                                                status.ctypes.data))
    return status, rvec, tvec, mask[:len(obj)], ninl


def Rodrigues(src, ctx=None):
    """cv2.Rodrigues(src) -> (dst, None): 3-vector (3, 3x1 or 1x3) -> 3x3 matrix, 3x3 matrix -> 3x1 vector
    (src/visual_slam.py:243; the Jacobian cv2 also returns is not computed)."""
    a = np.ascontiguousarray(src, np.float64)
    ctx = ctx or _lib.default_context()
    if a.size == 9:
        out = np.zeros((3, 1))
        ctx.check(ctx.lib.vo_rodrigues(ctx.handle, a.ctypes.data, 1, out.ctypes.data))
    elif a.size == 3:
        out = np.zeros((3, 3))
        ctx.check(ctx.lib.vo_rodrigues(ctx.handle, a.ctypes.data, 0, out.ctypes.data))
    else:
        raise ValueError("Rodrigues takes a 3-vector or a 3x3 matrix")
    return out, None


def _one_frame_against_a_map(map_points, map_descriptors, keypoints_xy, descriptors, ctx):
    """A FrontEnd configured for one frame of host arrays in slot 0 and the map staged: what relocalize() and relocalize_guided() share."""
    from .frontend import FrontEnd
    d = np.asarray(descriptors)
    if d.ndim != 2 or d.shape[1] not in (32, 128):
        raise ValueError("descriptors must be [n, 32] (ORB) or [n, 128] (SIFT)")
    if d.dtype != np.uint8:
        u = d.astype(np.uint8)
        if not np.array_equal(u.astype(d.dtype), d):
            raise ValueError("descriptor rows must hold integer values 0..255")
        d = u
    xy = np.ascontiguousarray(keypoints_xy, dtype=np.float32).reshape(-1, 2)
    if len(xy) != len(d):
        raise ValueError("keypoints_xy must be [n, 2]")
    ctx = ctx or _lib.default_context()
    if d.shape[1] == 128:
        fe = FrontEnd(32, 32, max_frames=1, max_pairs=1, detector="sift", kp_cap=max(len(d), 1), ctx=ctx)
        fe.set_sift_rows(0, d, xy)
    else:
        fe = FrontEnd(64, 64, max_frames=1, max_pairs=1, nfeatures=max(len(d), 1), nlevels=1, ctx=ctx)
        fe.set_orb_rows(0, d, xy)
    fe.stage_map(map_descriptors, map_points)
    return fe


def relocalize(map_points, map_descriptors, keypoints_xy, descriptors, K, max_distance=0.0, iterations=100, reproj_err=8.0, confidence=0.99,
               seed=OPENCV_RNG_SEED, min_inliers=0, ctx=None, match="cross", ratio=0.75):
    """Place one frame in a map by its descriptors, from host arrays (FrontEnd.stage_map + set_*_rows + relocalize in one call):
    map_points [npt, 3] float64, map_descriptors [npt, D], keypoints_xy [n, 2], descriptors [n, D]; D = 32 (ORB rows, uint8:
    Hamming) or 128 (SIFT rows, integer values 0..255: L2).  What the reference's MatchWithMap is for and never does
    (src/visual_slam.py:211-217): bf.match(descriptors, map_descriptors) with crossCheck=True, `distance < max_distance` (0: no
    filter), cv2.solvePnPRansac on the matches; match='ratio' | 'cross+ratio' and ratio as FrontEnd.relocalize takes them (the
    result then has seconds = n.distance per match).  Returns dict(status, pose [3, 4] world -> camera in the map's gauge (zeros when
    status != 0), n_match, n_inl, matches = (map point, keypoint, distance float32, inlier mask)).
    The context is configured for this call (a small batch configuration sized to the frame); a caller with resident frames uses
    FrontEnd.relocalize instead."""
    fe = _one_frame_against_a_map(map_points, map_descriptors, keypoints_xy, descriptors, ctx)
    out = fe.relocalize([0], K, max_distance, iterations, reproj_err, confidence, seed, min_inliers, match=match, ratio=ratio)
    res = dict(status=int(out["status"][0]), pose=out["poses"][0], n_match=int(out["n_match"][0]), n_inl=int(out["n_inl"][0]),
               matches=fe.map_matches(0))
    if match != "cross":
        res["seconds"] = fe.map_match_seconds(0)
    return res


def relocalize_guided(map_points, map_descriptors, keypoints_xy, descriptors, K, prior, radius, ratio=0.0, max_distance=0.0, iterations=100,
                      reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED, min_inliers=0, ctx=None):
    """relocalize() by projection under a prior pose, from host arrays (FrontEnd.stage_map + set_*_rows + relocalize_guided in one
    call): prior [3, 4] world -> camera in the map's gauge; every map point in front of it takes the keypoint with the nearest
    descriptor within `radius` pixels of its projection.  Arguments and result as relocalize(), plus n_seen (map points with a
    keypoint in their window) and seconds (the second distance per match, FLT_MAX without one).  The context is configured for
    this call; a caller with resident frames uses FrontEnd.relocalize_guided instead."""
    P = np.ascontiguousarray(prior, dtype=np.float64)
    if P.shape != (3, 4):
        raise ValueError("prior must be [3, 4]")
    fe = _one_frame_against_a_map(map_points, map_descriptors, keypoints_xy, descriptors, ctx)
    out = fe.relocalize_guided([0], K, P[None], radius, ratio, max_distance, iterations, reproj_err, confidence, seed, min_inliers)
    return dict(status=int(out["status"][0]), pose=out["poses"][0], n_match=int(out["n_match"][0]), n_inl=int(out["n_inl"][0]),
                n_seen=int(out["n_seen"][0]), matches=fe.map_matches(0), seconds=fe.map_match_seconds(0))


def estimate_similarity_batch(src, dst, offsets, max_error, iterations=1000, confidence=0.99, seed=OPENCV_RNG_SEED, min_inliers=0, ctx=None):
    """B independent similarity problems in one launch (vo_sim3_ransac_batch); problem b owns rows offsets[b]:offsets[b+1] of src
    and dst.  Returns dict(status [B], scale [B], R [B, 3, 3], t [B, 3], n_inl [B], mask [total] uint8)."""
    b = np.ascontiguousarray(np.asarray(src, np.float64).reshape(-1, 3))
    a = np.ascontiguousarray(np.asarray(dst, np.float64).reshape(-1, 3))
    if len(a) != len(b):
        raise ValueError("src and dst must hold the same number of points")
    off = np.ascontiguousarray(offsets, np.int32)
    B = len(off) - 1
    opts = _lib.AlignOpts(0.0, float(max_error), int(iterations), float(confidence), int(seed), int(min_inliers))
    sim = np.zeros((B, 13)); mask = np.zeros(max(len(b), 1), np.uint8); ninl = np.zeros(B, np.int32); status = np.zeros(B, np.int32)
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_sim3_ransac_batch(ctx.handle, b.ctypes.data, a.ctypes.data, off.ctypes.data, B, C.addressof(opts), sim.ctypes.data,
                                           mask.ctypes.data, ninl.ctypes.data, status.ctypes.data))
    return dict(status=status, scale=sim[:, 0].copy(), R=sim[:, 1:10].reshape(B, 3, 3).copy(), t=sim[:, 10:].copy(), n_inl=ninl,
                mask=mask[:len(b)])


def estimate_similarity(src, dst, max_error, iterations=1000, confidence=0.99, seed=OPENCV_RNG_SEED, min_inliers=0, ctx=None):
    """The similarity dst ~ scale R src + t from 3D-3D correspondences with outliers (vo_sim3_ransac_batch, one problem): RANSAC
    over Umeyama's closed form on three points, then the same fit over the inliers.  src, dst [n, 3]; max_error is the inlier
    bound in dst's units — it has no default: it is in the caller's units and nobody can choose it for them.  Returns dict(status:
    0, VO_ERR_TOO_FEW (n < 3) or VO_ERR_NO_MODEL; scale, R [3, 3], t [3] (zeros when status != 0); n_inl; mask [n] uint8, the
    best RANSAC model's inliers)."""
    n = len(np.asarray(src, np.float64).reshape(-1, 3))
    o = estimate_similarity_batch(src, dst, [0, n], max_error, iterations, confidence, seed, min_inliers, ctx)
    return dict(status=int(o["status"][0]), scale=float(o["scale"][0]), R=o["R"][0], t=o["t"][0], n_inl=int(o["n_inl"][0]), mask=o["mask"])

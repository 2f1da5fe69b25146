"""The backend interface of visual_odometry_amd.cv2_surface on the project's CPU checkers: oracle.oracle (imported, not
edited), tests/ba_reference.lm and tests/epilines_reference.  Installed by the CPU tests with

    cv2_surface.backend = surface_oracle_backend.OracleBackend()

so that the reference's callers run through the same surface without a GPU.  Return shapes are the surface's (cv2's)."""
import numpy as np

import ba_reference as BR
import epilines_reference as ER
from oracle import oracle as O
from visual_odometry_amd.types import DMatch, KeyPoint


def _keypoints(a):
    return tuple(KeyPoint(x, y, s, an, r, o) for (x, y), s, an, r, o in
                 zip(a["xy"].tolist(), a["size"].tolist(), a["angle"].tolist(), a["response"].tolist(), a["octave"].tolist()))


class _Sift:
    def __init__(self, nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6):
        self.kw = dict(nfeatures=int(nfeatures), n_layers=int(nOctaveLayers), contrast_threshold=float(contrastThreshold),
                       edge_threshold=float(edgeThreshold), sigma=float(sigma))

    def detectAndCompute(self, image, mask=None):
        assert mask is None
        a = O.sift_detect_and_compute(image, **self.kw)
        return _keypoints(a), a["desc"].copy()


class _Orb:
    def __init__(self, nfeatures=500, **kw):
        self.params = O.orb_params(nfeatures=int(nfeatures), **kw)

    def detectAndCompute(self, image, mask=None):
        assert mask is None
        a = O.orb_detect_and_compute(image, self.params)
        return _keypoints(a), a["desc"]


class _Matcher:
    def __init__(self, normType, crossCheck):
        self.fn = {4: O.match_l2, 6: O.match_hamming}[normType]
        self.mode = 2 if crossCheck else 0

    def match(self, queryDescriptors, trainDescriptors):
        qi, ti, d = self.fn(queryDescriptors, trainDescriptors, self.mode)
        return [DMatch(a, b, c) for a, b, c in zip(qi.tolist(), ti.tolist(), d.tolist())]


class OracleBackend:
    def __init__(self):
        self.pnp_retvals = []            # every solvePnPRansac retval, in call order
        self.calls = []                  # names of the entries called, in order

    def SIFT_create(self, *a, **k):
        self.calls.append("SIFT_create")
        return _Sift(*a, **k)

    def ORB_create(self, *a, **k):
        self.calls.append("ORB_create")
        return _Orb(*a, **k)

    def BFMatcher(self, normType=4, crossCheck=False):
        self.calls.append("BFMatcher")
        return _Matcher(normType, crossCheck)

    def findEssentialMat(self, points1, points2, cameraMatrix, method, prob, threshold):
        self.calls.append("findEssentialMat")
        assert method == 8
        p1 = np.asarray(points1, np.float64).reshape(-1, 2)
        if len(p1) < 5:
            return None, None
        rc, E, mask, _ = O.find_essential_ransac(p1, points2, cameraMatrix, prob, threshold)
        if rc < 0:
            return None, None
        return E.reshape(-1, 3), mask.reshape(-1, 1)

    def recoverPose(self, E, points1, points2, cameraMatrix):
        self.calls.append("recoverPose")
        n, R, t, mask = O.recover_pose(E, points1, points2, cameraMatrix)
        return n, R, t, mask.reshape(-1, 1)

    def triangulatePoints(self, projMatr1, projMatr2, projPoints1, projPoints2):
        self.calls.append("triangulatePoints")
        return O.triangulate(projMatr1, projMatr2, np.ascontiguousarray(projPoints1, np.float64), np.ascontiguousarray(projPoints2, np.float64))

    def solvePnPRansac(self, objectPoints, imagePoints, cameraMatrix, distCoeffs, **k):
        self.calls.append("solvePnPRansac")
        assert not k and not np.any(np.asarray(distCoeffs))
        obj = np.asarray(objectPoints, np.float64).reshape(-1, 3)
        if len(obj) < 4:
            raise ValueError("solvePnPRansac needs at least 4 correspondences")      # cv2 raises cv2.error here
        rc, rvec, tvec, mask, _ = O.solve_pnp_ransac(obj, imagePoints, cameraMatrix)
        ok = rc == 0
        self.pnp_retvals.append(ok)
        return ok, rvec.reshape(3, 1), tvec.reshape(3, 1), (np.nonzero(mask)[0].astype(np.int32).reshape(-1, 1) if ok else None)

    def Rodrigues(self, src):
        self.calls.append("Rodrigues")
        out = O.rodrigues(src)
        return (out.reshape(3, 1) if out.size == 3 else out), None

    def computeCorrespondEpilines(self, points, whichImage, F):
        self.calls.append("computeCorrespondEpilines")
        p = np.asarray(points)
        if p.dtype not in ER.POINT_TYPES:
            p = p.astype(np.float64)
        return ER.correspond_epilines(p, whichImage, F)

    def resize(self, src, dsize, interpolation):
        self.calls.append("resize")
        fn = {1: O.resize_linear, 3: O.resize_area}[interpolation]
        return fn(src, int(dsize[0]), int(dsize[1]))

    def imdecode(self, buf):
        self.calls.append("imdecode")
        return O.jpeg_decode(buf)

    def bundle_adjust(self, poses, fixed, points, obs_cam, obs_pt, obs_xy, focal, cx, cy, iterations, huber_delta):
        self.calls.append("bundle_adjust")
        return BR.lm(poses, fixed, points, obs_cam, obs_pt, obs_xy, focal, cx, cy, iterations, huber_delta)

"""The `cv2` names the reference's in-scope callers use, on this package's HIP-backed modules.

    import visual_odometry_amd.cv2_surface as cv2          # dropin/initials.py does this for `from initials import *`

Carried names (reference call sites: src/visual_slam.py:16-19, :231-243, :303-372; src/image_pair.py:271-336;
src/frame_generator.py:25; src/image_and_keypoints.py:8-9, :42; src/feature_detection.py:118-125):
  constructors / constants  SIFT_create ORB_create BFMatcher NORM_L2 NORM_HAMMING FM_RANSAC RANSAC INTER_LINEAR INTER_AREA
  arithmetic                findEssentialMat recoverPose triangulatePoints solvePnPRansac Rodrigues computeCorrespondEpilines
                            undistortPoints (the lens model of src/image_and_keypoints.py:21-25, which the reference never applies)
                            resize imread imdecode line
  headless display          imshow waitKey destroyAllWindows
Any other attribute raises AttributeError naming this surface.  Arguments are positional in cv2's order.

Every arithmetic entry goes through one object, `backend`: by default HipBackend, the existing modules geometry, matcher,
detector, ingest (and map_filters for g2o_surface).  It is the only seam; the package itself never installs another one.
Importing this module loads no HIP library and creates no context: both wait for the first call that computes something.

The parity of these restatements with a cv2 build is unpinned, as everywhere in this package.
"""
from __future__ import annotations

import numpy as np

NORM_L2, NORM_HAMMING = 4, 6
FM_RANSAC = RANSAC = 8
INTER_LINEAR, INTER_AREA = 1, 3
IMREAD_COLOR = 1

ARITHMETIC = ("findEssentialMat", "recoverPose", "triangulatePoints", "solvePnPRansac", "Rodrigues", "computeCorrespondEpilines",
              "undistortPoints", "resize", "imread", "imdecode")


class HipBackend:
    """The default backend: each entry is the existing Python API of the same name (modules imported on first use)."""

    def SIFT_create(self, *a, **k):
        from . import detector
        return detector.SIFT_create(*a, **k)

    def ORB_create(self, *a, **k):
        from . import detector
        return detector.ORB_create(*a, **k)

    def BFMatcher(self, normType=NORM_L2, crossCheck=False):
        from . import matcher
        return matcher.BFMatcher(normType, crossCheck)

    def findEssentialMat(self, points1, points2, cameraMatrix, method, prob, threshold):
        from . import geometry
        return geometry.findEssentialMat(points1, points2, cameraMatrix, method, prob, threshold)

    def recoverPose(self, E, points1, points2, cameraMatrix):
        from . import geometry
        return geometry.recoverPose(E, points1, points2, cameraMatrix)

    def triangulatePoints(self, projMatr1, projMatr2, projPoints1, projPoints2):
        from . import geometry
        return geometry.triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2)

    def solvePnPRansac(self, objectPoints, imagePoints, cameraMatrix, distCoeffs, **k):
        from . import geometry
        return geometry.solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, **k)

    def Rodrigues(self, src):
        from . import geometry
        return geometry.Rodrigues(src)

    def computeCorrespondEpilines(self, points, whichImage, F):
        from . import geometry
        return geometry.computeCorrespondEpilines(points, whichImage, F)

    def undistortPoints(self, src, cameraMatrix, distCoeffs, R, P):
        from . import geometry
        return geometry.undistortPoints(src, cameraMatrix, distCoeffs, R, P)

    def resize(self, src, dsize, interpolation):
        from . import ingest
        return ingest.resize(src, dsize, interpolation)

    def imdecode(self, buf):
        from . import ingest
        return ingest.imdecode(buf)

    def bundle_adjust(self, poses, fixed, points, obs_cam, obs_pt, obs_xy, focal, cx, cy, iterations, huber_delta):
        from . import map_filters
        return map_filters.bundle_adjust(poses, fixed, points, obs_cam, obs_pt, obs_xy, focal, cx, cy, iterations, huber_delta)


backend = HipBackend()


def _touch():
    """Any surface call other than waitKey ends a run of consecutive waitKey calls."""
    global _idle_waits
    _idle_waits = 0


# ---- constructors
def SIFT_create(*args, **kwargs):
    _touch()
    return backend.SIFT_create(*args, **kwargs)


def ORB_create(*args, **kwargs):
    _touch()
    return backend.ORB_create(*args, **kwargs)


def BFMatcher(normType=NORM_L2, crossCheck=False):
    _touch()
    return backend.BFMatcher(normType, crossCheck)


# ---- arithmetic
def findEssentialMat(points1, points2, cameraMatrix, method=RANSAC, prob=0.999, threshold=1.0):
    _touch()
    return backend.findEssentialMat(points1, points2, cameraMatrix, method, prob, threshold)


def recoverPose(E, points1, points2, cameraMatrix):
    _touch()
    return backend.recoverPose(E, points1, points2, cameraMatrix)


def triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2):
    _touch()
    return backend.triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2)


def solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, **kwargs):
    _touch()
    return backend.solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, **kwargs)


def Rodrigues(src):
    _touch()
    return backend.Rodrigues(src)


def computeCorrespondEpilines(points, whichImage, F):
    _touch()
    return backend.computeCorrespondEpilines(points, whichImage, F)


def undistortPoints(src, cameraMatrix, distCoeffs, R=None, P=None):
    _touch()
    return backend.undistortPoints(src, cameraMatrix, distCoeffs, R, P)


def resize(src, dsize, interpolation=INTER_LINEAR):
    _touch()
    return backend.resize(src, dsize, interpolation)


def imdecode(buf, flags=IMREAD_COLOR):
    _touch()
    if flags != IMREAD_COLOR:
        raise NotImplementedError("cv2_surface.imdecode is built for IMREAD_COLOR")
    return backend.imdecode(buf)


def imread(filename, flags=IMREAD_COLOR):
    """cv2.imread(filename): None for a file that cannot be read, as cv2 returns."""
    _touch()
    try:
        with open(filename, "rb") as f:
            data = f.read()
    except OSError:
        return None
    if not data:
        return None
    try:
        return imdecode(data, flags)
    except ValueError:                  # not a JPEG file: cv2 returns None for what it cannot decode
        return None


def line(img, pt1, pt2, color, thickness=1):
    """cv2.line(img, pt1, pt2, color, thickness) for thickness 1 as a numpy rasteriser (src/image_pair.py:271): the longer axis
    is stepped one pixel at a time, the other rounded; points outside the image are clipped to its border.  Draws into img
    (made 3-channel if it is grey) and returns it.  Not cv2's Bresenham variant pixel for pixel: drawing is display only."""
    _touch()
    if thickness != 1:
        raise NotImplementedError("cv2_surface.line draws one-pixel lines (the reference passes thickness 1)")
    if img.ndim == 2:
        img = np.stack([img] * 3, axis=2)
    x0, y0 = int(pt1[0]), int(pt1[1])
    x1, y1 = int(pt2[0]), int(pt2[1])
    n = max(abs(x1 - x0), abs(y1 - y0), 1)
    xs = np.clip(np.rint(np.linspace(x0, x1, n + 1)).astype(int), 0, img.shape[1] - 1)
    ys = np.clip(np.rint(np.linspace(y0, y1, n + 1)).astype(int), 0, img.shape[0] - 1)
    c = np.asarray(color, np.float64).ravel()
    c = np.resize(c, img.shape[2]) if c.size < img.shape[2] else c[:img.shape[2]]
    img[ys, xs] = np.clip(c, 0, 255).astype(img.dtype)
    return img


# ---- headless display
shown = {}                  # window name -> the last image imshow was given
QUIT_AFTER_IDLE_WAITS = 3   # the default script: the third waitKey in a row with no other surface call in between answers 'q'
_idle_waits = 0
_key_script = None          # None: the default script; else an iterator or a callable(delay) -> key


def set_key_script(script=None):
    """script: None for the default; an iterable of key codes (then -1 for ever); or a callable(delay_ms) -> key code.

    The default makes VisualSlam.run() (src/visual_slam.py:338-374) process every file and then leave its closing
    `while True: waitKey(100)` loop.  Its call order per file is imread, resize, [.. imshow, .., waitKey(100) in
    match_current_and_previous_frame from the second frame on, then arithmetic of the viewer-free tail ..], waitKey(400000),
    and the next file starts with imread: inside the loop at most two waitKey calls are consecutive (waitKey(100) at :312 is
    followed by no surface call before :357), so the answer is -1 for the first two and ord('q') for the third, which only the
    closing loop reaches (:371-374)."""
    global _key_script, _idle_waits
    _idle_waits = 0
    _key_script = iter(script) if script is not None and not callable(script) else script


def imshow(winname, mat):
    _touch()
    shown[winname] = mat


def waitKey(delay=0):
    global _idle_waits
    if _key_script is not None:
        if callable(_key_script):
            return int(_key_script(delay))
        return int(next(_key_script, -1))
    _idle_waits += 1
    if _idle_waits >= QUIT_AFTER_IDLE_WAITS:
        _idle_waits = 0
        return ord("q")
    return -1


def destroyAllWindows():
    _touch()


def __getattr__(name):
    raise AttributeError(f"visual_odometry_amd.cv2_surface carries no cv2.{name}: it holds only the names the reference's "
                         "in-scope callers use (see its module docstring)")

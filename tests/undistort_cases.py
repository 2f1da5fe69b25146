"""A small 3-D scene seen by three cameras through a lens (not a test module): what tests/test_gpu_undistort.py stages and what
tests/test_undistort_cases_reference.py holds on the CPU.

Camera: the reference's at its working size (visual_slam.py:28-37 at scale 0.3: f = 802.8, 1152 x 648) with the reference's own
five coefficients (src/image_and_keypoints.py:21-25) times SCALE.  Cameras 0, 1, 2: centres one baseline apart on a line, each
turned by a few degrees about an axis of its own (tests/track_cases.py learnt that pure translations are a special configuration
of the five-point solver).  N points: chosen as ideal pixels spread over camera 1's frame at depths of 4 .. 12 baselines, so
that the distortion, which grows with the distance from the principal point, acts on them unevenly.  Every point owns one
distinct random 32-byte row, the same in every frame and in the same order: the strict cross-check is the identity permutation.

Three versions of every frame's float32 keypoints:
  ideal       the pinhole projections (the yardstick)
  distorted   the same through the lens: what a detector would report
  corrected   the checker's undistort_pixels(distorted): what vo_frames_undistort must leave in the slot

SCALE = 5: with the coefficients as they are (SCALE 1: the keypoints move by 2 px in the median, 7 px at most) pair (0, 1) of
the distorted frames keeps all 60 inliers under findEssentialMat's 1 px — a smooth lens is nearly consistent with SOME essential
matrix over one baseline, a wrong one; at 3 it loses 2, at 5 it loses 10 — the figures are in
tests/test_undistort_cases_reference.py, which asserts them with the oracle."""
import numpy as np

import hamming_reference as HR
import undistort_reference as U
from twoview import rot
from visual_odometry_amd import synth

K = synth.reference_camera_matrix()
W, H = 1152, 648
SCALE = 5.0
DIST = U.REFERENCE_DIST * SCALE
N = 60
N_FRAMES = 3
STEP = 1.0


def _build():
    rng = np.random.default_rng(20261021)
    R = [rot(rng.normal(size=3), rng.uniform(0.03, 0.08)) for _ in range(N_FRAMES)]
    C = [np.array([k * STEP, 0.0, 0.0]) for k in range(N_FRAMES)]
    uv = rng.uniform([40, 40], [W - 40, H - 40], (N, 2))
    z = rng.uniform(4.0, 12.0, N)
    rays = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], np.ones(N)], 1) * z[:, None]
    X = rays @ R[1] + C[1]                                  # x_cam = R (X - C)
    rows = HR.rand_rows(rng, N)
    assert len(np.unique(rows, axis=0)) == N
    return R, C, X, rows


ROT, CENTRE, X, ROWS = _build()
PAIRS = [[0, 1], [1, 2]]


def project64(k):
    c = (X - CENTRE[k]) @ ROT[k].T
    return np.stack([K[0, 0] * c[:, 0] / c[:, 2] + K[0, 2], K[1, 1] * c[:, 1] / c[:, 2] + K[1, 2]], axis=1)


def ideal(k):
    return project64(k).astype(np.float32)


def distorted(k, dist=DIST):
    return U.distort_pixels(project64(k), K, dist).astype(np.float32)


def corrected(k, dist=DIST):
    return U.undistort_pixels(distorted(k, dist), K, dist)


def relative_pose(a, b):
    """(R, unit t) with x_b = R x_a + t, the convention of cv2.recoverPose."""
    return synth.relative_pose(ROT[a], CENTRE[a], ROT[b], CENTRE[b])


def oracle_pose(O, p1, p2):
    """findEssentialMat + recoverPose of the oracle on matched pixels -> (status, inlier mask, [R|t] 3 x 4)."""
    p1 = np.asarray(p1, np.float64); p2 = np.asarray(p2, np.float64)
    rc, E, mask, _ = O.find_essential_ransac(p1, p2, K)
    if rc != 0:
        return rc, None, None
    inl = mask > 0
    _, R, t, _ = O.recover_pose(E[0], p1[inl], p2[inl], K)
    return rc, inl, np.hstack([R, t.reshape(3, 1)])


def coordinate_error(dist=DIST):
    """The most a corrected float32 coordinate can differ from the yardstick's, in pixels: the round-trip residual of five sweeps on
    these points (measured with the checker in float64) plus three float32 roundings of a coordinate below 2048 px — the
    yardstick's own, the distorted keypoint's (carried through an inverse map whose slope is about 1), the corrected result's —
    of half an ulp = 2^-14 px each."""
    residual = 0.0
    for k in range(N_FRAMES):
        p = project64(k)
        residual = max(residual, float(np.abs(U.undistort_points(U.distort_pixels(p, K, dist), K, dist, None, K) - p).max()))
    return residual + 3 * 2.0 ** -14, residual


def pose_margin(O, a=0, b=1, dist=DIST, h=1e-3):
    """How far [R|t] of pair (a, b) can move (largest entry) when every one of its 4 N coordinates moves by at most
    coordinate_error(): to first order sum_i |d[R|t] / dc_i| * delta, the derivatives by one-sided differences of h px with the
    oracle.  findEssentialMat does not refine: its E comes from ONE five-point sample, so all but 20 of the derivatives vanish
    — the sum is the conditioning of that sample — as long as h moves no point across the 1 px threshold, which the caller
    checks through the mask."""
    delta, _ = coordinate_error(dist)
    p = [ideal(a).astype(np.float64), ideal(b).astype(np.float64)]
    rc, mask0, Rt0 = oracle_pose(O, p[0], p[1])
    assert rc == 0
    total = np.zeros((3, 4))
    for side in range(2):
        for i in range(N):
            for c in range(2):
                q = [p[0].copy(), p[1].copy()]
                q[side][i, c] += h
                rc, mask, Rt = oracle_pose(O, q[0], q[1])
                assert rc == 0 and np.array_equal(mask, mask0)
                total += np.abs(Rt - Rt0) / h
    return float(total.max()) * delta, delta

#!/usr/bin/env python3
"""k_undistort_frames and k_undistort_points through their stage bracket (docs/kernels/k_undistort_points.md):
    python tests/scripts/bench_undistort.py
257 ORB slots of 2000 staged keypoints; an upload between the launches clears the once-per-detection marks."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import undistort_reference as U  # noqa: E402
from visual_odometry_amd import geometry, synth  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd  # noqa: E402

F, N, REPS = 257, 2000, 20
K = synth.reference_camera_matrix()
fe = FrontEnd(64, 64, max_frames=F, max_pairs=1, nfeatures=N, nlevels=1)
rng = np.random.default_rng(0)
rows = rng.integers(0, 256, (N, 32), dtype=np.uint8)
xy = rng.uniform([0, 0], [1152, 648], (N, 2)).astype(np.float32)
for s in range(F):
    fe.set_orb_rows(s, rows, xy)
frames = np.zeros((F, 64, 64), np.uint8)
fe.undistort(0, F, K, U.REFERENCE_DIST)          # warm-up, and the result is the checker's
assert fe.features(F - 1)["xy"].tobytes() == U.undistort_pixels(xy, K, U.REFERENCE_DIST).tobytes()
fe.profile(True)
for _ in range(REPS):
    fe.upload(frames)
    fe.undistort(0, F, K, U.REFERENCE_DIST)
ms, n = fe.profile_read()["undistort_points"]
print(f"k_undistort_frames: {F} slots x {N} keypoints (kp_cap {fe.kp_cap}): {1e3 * ms / n:.1f} us per launch over {n} launches; "
      f"{fe.stage_bytes('undistort_points', F) / 1e6:.1f} MB algorithmic")
pts = rng.uniform([0, 0], [1152, 648], (F * N, 2))
fe.profile(True)
for _ in range(5):
    geometry.undistortPoints(pts, K, U.REFERENCE_DIST, None, K, ctx=fe.ctx)
ms, n = fe.profile_read()["undistort_points"]
print(f"k_undistort_points: {F * N} f64 points: {1e3 * ms / n:.1f} us per launch over {n} launches (kernel only, copies excluded)")

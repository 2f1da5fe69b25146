"""Checker for the map statistics (vo_map_statistics, vo_slam_stats): Map.show_map_statistics (src/map.py:234-297) in plain Python.

stats(map_dict, K) works on the three dense lists as FrontEnd.slam_map() returns them (cam_pose [ncam, 3, 4], points [npt, 3],
obs_cam / obs_pt [nobs] positions in those lists, obs_xy [nobs, 2]).  The per-observation errors come from
oracle.reprojection_sqerr, which is byte-equal to k_reprojection / k_slam_filter (tests/test_gpu_next_rows.py); everything
after them is re-typed from the reference: the sum is calculate_reprojection_error's loop (:79-95) — one += per observation in
list order, starting from 0.0 — the histogram show_number_of_observations_per_point's two defaultdicts (:245-254) and the matrix
show_observation_matrix's list comprehensions (:267-297).  Camera and point ids are the list positions: ids grow with the
position in the reference, so cam1 < cam2 is index order.

stats_of_records(cameras, points, observations, K) is the same walk on Observation-like records with arbitrary (growing) ids,
as the reference holds them; tests/test_map_stats_reference.py checks the two against each other."""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HIST = 64                      # VO_STATS_HIST: bin 63 = 63 observations or more
MAX_CAMERAS = 64               # VO_BA_MAX_CAMERAS


def poses_4x4(cam_pose):
    p = np.asarray(cam_pose, np.float64).reshape(-1, 3, 4)
    out = np.zeros((len(p), 4, 4))
    out[:, :3] = p
    out[:, 3, 3] = 1.0
    return out


def _sqerr(poses44, points, obs_cam, obs_pt, obs_xy, K):
    from oracle import oracle as O
    if len(obs_cam) == 0:
        return []
    err, _ = O.reprojection_sqerr(poses44, points, obs_cam, obs_pt, obs_xy, K, np.inf)
    return err.tolist()


def _fold(errors, high_threshold):
    total_error = 0.0
    max_error = 0.0
    n_high = 0
    for sqerror in errors:                                   # map.py:80-95
        if sqerror > high_threshold:
            n_high += 1
        if sqerror > max_error:                              # (a NaN never becomes the maximum)
            max_error = sqerror
        total_error += sqerror
    return total_error, max_error, n_high


def _histogram(point_ids, observation_point_ids):
    observations_per_point = collections.defaultdict(lambda: 0)      # map.py:246-248
    for point_id in observation_point_ids:
        observations_per_point[point_id] += 1
    counts = collections.defaultdict(lambda: 0)                      # :250-252
    for count in observations_per_point.values():
        counts[count] += 1
    hist = np.zeros(HIST, np.int32)
    for key in sorted(counts.keys()):
        hist[min(key, HIST - 1)] += counts[key]
    # the addition: points of the list that no observation names (the defaultdict above never sees them)
    hist[0] += sum(1 for point_id in point_ids if point_id not in observations_per_point)
    return hist


def _matrix(camera_ids, point_ids, observations):
    """observations: (camera_id, point_id) in list order -> [ncam, ncam] by position in the camera list"""
    observations_of_point = collections.defaultdict(lambda: [])     # map.py:274-276
    for camera_id, point_id in observations:
        observations_of_point[point_id].append(camera_id)
    obs_matrix = collections.defaultdict(lambda: collections.defaultdict(lambda: 0))
    for point_id in point_ids:                                       # :283-294
        cameras_that_see_point = [camera_id for camera_id in observations_of_point[point_id]]
        combinations = [(cam1, cam2) for cam1 in cameras_that_see_point for cam2 in cameras_that_see_point if cam1 < cam2]
        for (cam1, cam2) in combinations:
            obs_matrix[cam1][cam2] += 1
    row = {camera_id: i for i, camera_id in enumerate(camera_ids)}
    out = np.zeros((len(camera_ids), len(camera_ids)), np.int32)
    for cam1, value1 in obs_matrix.items():
        for cam2, value2 in value1.items():
            out[row[cam1], row[cam2]] = value2
    return out


def stats(m, K, high_threshold=10.0):
    """dict(total_sqerr, mean_sqerr, max_sqerr (Python floats), n_high, obs_hist [64] i32, obs_matrix [ncam, ncam] i32, cam_frame)"""
    poses = poses_4x4(m["cam_pose"])
    points = np.asarray(m["points"], np.float64).reshape(-1, 3)
    oc = [int(v) for v in np.asarray(m["obs_cam"]).ravel()]
    op = [int(v) for v in np.asarray(m["obs_pt"]).ravel()]
    xy = np.asarray(m["obs_xy"], np.float64).reshape(-1, 2)
    total, mx, n_high = _fold(_sqerr(poses, points, oc, op, xy, K), high_threshold)
    return dict(total_sqerr=total, mean_sqerr=total / len(oc) if len(oc) > 0 else 0.0, max_sqerr=mx, n_high=n_high,
                obs_hist=_histogram(range(len(points)), op), obs_matrix=_matrix(range(len(poses)), range(len(points)), zip(oc, op)),
                cam_frame=np.asarray(m.get("cam_frame", np.arange(len(poses))), np.int32))


def stats_of_records(cameras, points, observations, K, high_threshold=10.0):
    """The same on records: cameras with .camera_id and .pose() (4 x 4), points with .point_id and .point, observations with
    .camera_id, .point_id, .image_coordinates — walked as the reference walks them, through id dictionaries."""
    camera_dict = {camera.camera_id: i for i, camera in enumerate(cameras)}          # map.py:73-78
    point_dict = {point.point_id: i for i, point in enumerate(points)}
    poses = np.array([camera.pose() for camera in cameras], np.float64).reshape(-1, 4, 4)
    pts = np.array([point.point for point in points], np.float64).reshape(-1, 3)
    errors = _sqerr(poses, pts, [camera_dict[o.camera_id] for o in observations], [point_dict[o.point_id] for o in observations],
                    np.array([o.image_coordinates for o in observations], np.float64).reshape(-1, 2), K)
    total, mx, n_high = _fold(errors, high_threshold)
    return dict(total_sqerr=total, mean_sqerr=total / len(observations) if len(observations) > 0 else 0.0, max_sqerr=mx, n_high=n_high,
                obs_hist=_histogram([p.point_id for p in points], [o.point_id for o in observations]),
                obs_matrix=_matrix([c.camera_id for c in cameras], [p.point_id for p in points],
                                   [(o.camera_id, o.point_id) for o in observations]))


def same(got, want, keys=("total_sqerr", "max_sqerr", "n_high", "obs_hist", "obs_matrix"), what=""):
    """byte-equal doubles, array_equal integers"""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k in ("total_sqerr", "max_sqerr", "mean_sqerr"):
            assert np.float64(g).tobytes() == np.float64(w).tobytes(), (what, k, float(g), float(w))
        else:
            assert g.shape == w.shape and np.array_equal(g, w), (what, k, g, w)


def order_example(reverse=False):
    """Identity pose, K = I, the point (0, 0, 1): an observation at (u, 0) has sqerr = u * u exactly.  [2^27, then 300 x 1.0] sums to
    2^54 in list order (every 2^54 + 1 rounds back: the ulp there is 4) and to 2^54 + 300 reversed; a blocked or tree sum gives
    2^54 + 300 for both."""
    u = [float(2 ** 27)] + [1.0] * 300
    if reverse:
        u = u[::-1]
    n = len(u)
    return dict(cam_pose=np.eye(4)[None, :3], points=np.array([[0.0, 0.0, 1.0]]), obs_cam=np.zeros(n, np.int32), obs_pt=np.zeros(n, np.int32),
                obs_xy=np.stack([np.array(u), np.zeros(n)], axis=1)), np.eye(3)


def random_map(seed=5, ncam=6, npt=40, nobs=150):
    """A seeded map in front of cameras near the origin: duplicates of a point in one camera, point 0 without an observation, point 1
    with exactly one.  -> (map dict, K)"""
    rng = np.random.default_rng(seed)
    K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])
    cam_pose = np.zeros((ncam, 3, 4))
    for c in range(ncam):
        a = 0.05 * c
        cam_pose[c, :, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
        cam_pose[c, :, 3] = [-0.3 * c, 0.02 * c, 0.0]
    points = np.column_stack([rng.uniform(-2, 2, npt), rng.uniform(-1.5, 1.5, npt), rng.uniform(4, 9, npt)])
    obs_pt = rng.integers(2, npt, nobs).astype(np.int32)
    obs_cam = rng.integers(0, ncam, nobs).astype(np.int32)
    obs_pt[7] = 1                                                             # point 1: one observation; point 0: none
    a, b = ncam - 2, ncam - 1
    obs_pt[20:24] = 5; obs_cam[20:24] = [a, a, b, a]                          # point 5: three times in the last camera but one
    proj = np.zeros((nobs, 2))
    for i in range(nobs):
        x = K @ (cam_pose[obs_cam[i]] @ np.append(points[obs_pt[i]], 1.0))
        proj[i] = x[:2] / x[2]
    obs_xy = proj + rng.normal(0, 1.5, (nobs, 2))                             # errors on both sides of 10
    return dict(cam_pose=cam_pose, points=points, obs_cam=obs_cam, obs_pt=obs_pt, obs_xy=obs_xy), K

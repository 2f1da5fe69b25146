"""No GPU: the checker of the map statistics (tests/map_stats_reference.py) against a second, object-level re-typing that walks
Observation-like records as src/map.py does, and the order example that pins the sum."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_stats_reference as R  # noqa: E402


class Camera:
    def __init__(self, camera_id, T):
        self.camera_id, self.T = camera_id, T

    def pose(self):
        return self.T


class Point:
    def __init__(self, point_id, point):
        self.point_id, self.point = point_id, point


class Observation:
    def __init__(self, point_id, camera_id, image_coordinates):
        self.point_id, self.camera_id, self.image_coordinates = point_id, camera_id, image_coordinates


def records(m):
    """ids that grow with the list position but are not the positions, as the reference's global counters give them"""
    cam_id = [10 + 3 * i for i in range(len(m["cam_pose"]))]
    pt_id = [100 + 7 * i for i in range(len(m["points"]))]
    cameras = [Camera(cam_id[i], T) for i, T in enumerate(R.poses_4x4(m["cam_pose"]))]
    points = [Point(pt_id[i], X) for i, X in enumerate(m["points"])]
    observations = [Observation(pt_id[p], cam_id[c], xy) for c, p, xy in zip(m["obs_cam"], m["obs_pt"], m["obs_xy"])]
    return cameras, points, observations


def test_the_array_checker_is_the_object_walk():
    m, K = R.random_map()
    a, b = R.stats(m, K), R.stats_of_records(*records(m), K)
    R.same(a, b, ("total_sqerr", "mean_sqerr", "max_sqerr", "n_high", "obs_hist", "obs_matrix"))
    # the map has what it was built to have
    assert a["obs_hist"][0] >= 1 and a["obs_hist"][1] >= 1 and a["obs_hist"].sum() == len(m["points"])
    assert (a["obs_hist"] * np.arange(R.HIST)).sum() == len(m["obs_cam"])
    assert 0 < a["n_high"] < len(m["obs_cam"]) and a["max_sqerr"] > 10.0
    assert not np.tril(a["obs_matrix"]).any() and a["obs_matrix"].sum() > 0
    # point 5 is seen three times by camera 4 and once by camera 5 in rows 20..23: the same-camera observations pair with nothing
    only5 = dict(m, obs_cam=m["obs_cam"][20:24], obs_pt=m["obs_pt"][20:24], obs_xy=m["obs_xy"][20:24])
    s5 = R.stats(only5, K)
    assert s5["obs_matrix"][4, 5] == 3 and s5["obs_matrix"].sum() == 3 and s5["obs_hist"][4] == 1 and s5["obs_hist"][0] == len(m["points"]) - 1


def test_the_sum_is_in_list_order():
    m, K = R.order_example()
    r, K2 = R.order_example(reverse=True)
    assert R.stats(m, K)["total_sqerr"] == float(2 ** 54)
    assert R.stats(r, K2)["total_sqerr"] == float(2 ** 54 + 300)
    assert R.stats(m, K)["max_sqerr"] == float(2 ** 54) and R.stats(m, K)["n_high"] == 1
    assert R.stats(m, K)["obs_hist"][R.HIST - 1] == 1 and not R.stats(m, K)["obs_matrix"].any()


def test_the_empty_map_is_all_zeros():
    m = dict(cam_pose=np.zeros((0, 3, 4)), points=np.zeros((0, 3)), obs_cam=np.zeros(0, np.int32), obs_pt=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2)))
    s = R.stats(m, np.eye(3))
    assert s["total_sqerr"] == 0.0 and s["mean_sqerr"] == 0.0 and s["max_sqerr"] == 0.0 and s["n_high"] == 0
    assert not s["obs_hist"].any() and s["obs_matrix"].shape == (0, 0)

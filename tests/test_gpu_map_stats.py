"""GPU: vo_map_statistics (map_filters.map_statistics / show_map_statistics) — Map.show_map_statistics (src/map.py:234-297) on the
device — against tests/map_stats_reference.py on chosen maps.  Every comparison is exact: array_equal on the integers, byte
equality on the two doubles.  The maps are the smallest at which k_slam_stats can go wrong: the boundaries of its 256-lane rounds
and of the hand-over between its two LDS buffers, a list order that a blocked or tree sum would not survive, duplicates in one
camera, points without observations, the open-ended bin, the camera limit and observations that name nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_stats_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])


def gpu(m, K, high_threshold=10.0):
    from visual_odometry_amd import map_filters
    return map_filters.map_statistics(R.poses_4x4(m["cam_pose"]), m["points"], m["obs_cam"], m["obs_pt"], m["obs_xy"], K, high_threshold)


def check(m, K, high_threshold=10.0, what=""):
    got, want = gpu(m, K, high_threshold), R.stats(m, K, high_threshold)
    R.same(got, want, ("total_sqerr", "mean_sqerr", "max_sqerr", "n_high", "obs_hist", "obs_matrix"), what)
    assert got["obs_hist"].dtype == np.int32 and got["obs_matrix"].dtype == np.int32
    assert (got["n_cam"], got["n_pts"], got["n_obs"]) == (len(m["cam_pose"]), len(m["points"]), len(m["obs_cam"]))
    return got


def empty(ncam=0, npt=0):
    return dict(cam_pose=np.tile(np.eye(4)[:3], (ncam, 1, 1)), points=np.tile([0.0, 0.0, 1.0], (npt, 1)), obs_cam=np.zeros(0, np.int32),
                obs_pt=np.zeros(0, np.int32), obs_xy=np.zeros((0, 2)))


def test_the_empty_map_is_all_zeros():
    got = check(empty(), K)
    assert got["total_sqerr"] == 0.0 and got["max_sqerr"] == 0.0 and got["mean_sqerr"] == 0.0 and got["n_high"] == 0
    assert not got["obs_hist"].any() and got["obs_matrix"].shape == (0, 0)
    got = check(empty(3, 5), K)                                   # cameras and points, no observation: every point in bin 0
    assert got["obs_hist"][0] == 5 and got["obs_hist"].sum() == 5 and not got["obs_matrix"].any() and got["total_sqerr"] == 0.0


def test_one_observation():
    m, k = R.random_map(nobs=150)
    one = dict(m, obs_cam=m["obs_cam"][:1], obs_pt=m["obs_pt"][:1], obs_xy=m["obs_xy"][:1])
    got = check(one, k)
    assert got["total_sqerr"] == got["max_sqerr"] == got["mean_sqerr"] > 0 and got["obs_hist"][1] == 1 and not got["obs_matrix"].any()


@pytest.mark.parametrize("nobs", [255, 256, 257, 513])
def test_round_boundaries(nobs):
    """3 cameras; the observation counts around the 256-lane rounds and the hand-over between the two buffers (513: three rounds)"""
    m, k = R.random_map(seed=nobs, ncam=3, npt=40, nobs=nobs)
    got = check(m, k, what=nobs)
    assert got["n_high"] > 0 and got["obs_matrix"].sum() > 0 and (got["obs_hist"] * np.arange(R.HIST)).sum() == nobs


@pytest.mark.parametrize("npt", [255, 257])
def test_point_list_boundaries(npt):
    """one observation per point: the scan over the points crosses (or just misses) a 256-point round"""
    m, k = R.random_map(seed=npt, ncam=3, npt=npt, nobs=npt)
    m["obs_pt"] = np.random.default_rng(npt).permutation(npt).astype(np.int32)
    got = check(m, k, what=npt)
    assert got["obs_hist"][1] == npt and got["obs_hist"].sum() == npt and not got["obs_matrix"].any()


def test_the_sum_is_in_list_order():
    m, k = R.order_example()
    r, _ = R.order_example(reverse=True)
    a, b = check(m, k), check(r, k)
    assert a["total_sqerr"] == float(2 ** 54)                     # every 2^54 + 1 rounds back
    assert b["total_sqerr"] == float(2 ** 54 + 300)               # a blocked or tree sum gives this for both
    assert a["max_sqerr"] == b["max_sqerr"] == float(2 ** 54) and a["n_high"] == b["n_high"] == 1
    assert a["obs_hist"][63] == 1 and not a["obs_matrix"].any()   # 301 observations of one point in one camera pair with nothing


def test_duplicates_in_one_camera_and_a_point_without_observations():
    m = empty(4, 3)
    a, b = 1, 3
    m.update(obs_cam=np.array([a, b, a], np.int32), obs_pt=np.array([1, 1, 1], np.int32), obs_xy=np.array([[3.0, 0.0], [0.0, 0.0], [0.0, 4.0]]))
    got = check(m, np.eye(3))
    assert got["obs_matrix"][a, b] == 2 and got["obs_matrix"].sum() == 2 and not np.diag(got["obs_matrix"]).any()
    assert got["obs_hist"][3] == 1 and got["obs_hist"][0] == 2 and got["obs_hist"].sum() == 3
    assert got["total_sqerr"] == 25.0 and got["max_sqerr"] == 16.0 and got["n_high"] == 1


def test_one_point_seen_by_all_64_cameras():
    m = empty(64, 2)
    m.update(obs_cam=np.arange(64, dtype=np.int32)[::-1].copy(), obs_pt=np.ones(64, np.int32), obs_xy=np.zeros((64, 2)))
    got = check(m, np.eye(3))
    assert np.array_equal(got["obs_matrix"], np.triu(np.ones((64, 64), np.int32), 1)) and got["obs_matrix"].sum() == 2016
    assert got["obs_hist"][63] == 1 and got["obs_hist"][0] == 1 and got["obs_hist"].sum() == 2      # 64 >= 63


def test_65_cameras_are_unsupported():
    with pytest.raises(NotImplementedError):
        gpu(empty(65, 1), K)


@pytest.mark.parametrize("cam,pt", [(3, 0), (0, -1), (-1, 0), (0, 2)])
def test_an_observation_of_nothing_is_invalid(cam, pt):
    from visual_odometry_amd import _lib
    m = empty(3, 2)
    m.update(obs_cam=np.array([0, cam], np.int32), obs_pt=np.array([0, pt], np.int32), obs_xy=np.zeros((2, 2)))
    with pytest.raises(_lib.VoError) as e:
        gpu(m, K)
    assert e.value.code == _lib.VO_ERR_INVALID


def test_the_threshold_is_strict():
    """errors 9, 10 (exactly on it), 16 and 25 around high_threshold = 10, a NaN among them: sqerr > threshold, and e > m for the maximum"""
    m = empty(1, 1)
    m.update(obs_cam=np.zeros(5, np.int32), obs_pt=np.zeros(5, np.int32), obs_xy=np.array([[3.0, 0.0], [1.0, 3.0], [0.0, 4.0], [3.0, 4.0], [0.0, 0.0]]))
    got = check(m, np.eye(3))
    assert got["n_high"] == 2 and got["max_sqerr"] == 25.0 and got["total_sqerr"] == 9.0 + 10.0 + 16.0 + 25.0
    assert check(m, np.eye(3), high_threshold=9.0)["n_high"] == 3 and check(m, np.eye(3), high_threshold=25.0)["n_high"] == 0
    nan = dict(m, obs_xy=np.array([[3.0, 0.0], [np.nan, 3.0], [0.0, 4.0], [3.0, 4.0], [0.0, 0.0]]))
    got = gpu(nan, np.eye(3))
    assert np.isnan(got["total_sqerr"]) and got["max_sqerr"] == 25.0 and got["n_high"] == 2


def test_the_object_form_is_the_array_form():
    from visual_odometry_amd import map_filters
    from test_map_stats_reference import records
    m, k = R.random_map()
    a = map_filters.show_map_statistics(*records(m), k)
    R.same(a, gpu(m, k), ("total_sqerr", "mean_sqerr", "max_sqerr", "n_high", "obs_hist", "obs_matrix"))
    R.same(a, R.stats_of_records(*records(m), k), ("total_sqerr", "mean_sqerr", "max_sqerr", "n_high", "obs_hist", "obs_matrix"))

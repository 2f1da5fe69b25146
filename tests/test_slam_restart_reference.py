"""No GPU: what tests/test_gpu_slam_restart.py builds on.  The free-running checker with restarts (tests/slam_restart_reference.py
on oracle features) on the chains that test cuts from synth.sequence(7, 640, 480, step=4.0) / 1000 features / max_cameras = 4:
where the segments start, which status ended tracking, and that every pair inside a segment localises — so the GPU test's table
does not rest on the device alone.  And the pure helper of FrontEnd.slam_chains(restart=True): flat outputs -> segments."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_restart_reference as R  # noqa: E402

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
TOO_FEW, NO_MODEL = -3, -4
CHAINS = dict(L=[0, 1, 2, 3, None, 2, 3, 4, 5, 6], A=[0, 1, 2, 3, 4, 5, 6], HEAD=[None, 0, 1, 2], TAIL=[0, 1, 2, 3, None])


@pytest.fixture(scope="module")
def chains(oracle):
    """name -> (pair inputs, K); run(name, **opts) -> the checker's results"""
    from visual_odometry_amd import synth
    oracle.set_dk_early_exit(True)
    try:
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        p = oracle.orb_params(nfeatures=NFEAT)
        feats = [oracle.orb_detect_and_compute(f, p) for f in seq["frames"]]
        blank = oracle.orb_detect_and_compute(np.full_like(seq["frames"][0], 127), p)
        assert len(blank["desc"]) == 0                                       # a blank frame has no keypoints: its pairs fail on their own
        pins = {name: R.pair_inputs_from_oracle(oracle, [blank if f is None else feats[f] for f in frames], seq["K"]) for name, frames in CHAINS.items()}
    finally:
        oracle.set_dk_early_exit(False)

    def run(name, **opts):
        oracle.set_dk_early_exit(True)
        try:
            return R.run(oracle, pins[name], seq["K"], {"max_cameras": MAX_CAMERAS, **opts})
        finally:
            oracle.set_dk_early_exit(False)
    return run


def _table(res):
    return [r["status"] for r in res], [r["segment"] for r in res], [r["cause"] for r in res]


def test_a_lost_stretch_gives_two_segments(chains):
    res = chains("L")
    F = R.FAILED
    assert _table(res) == ([0, 0, 0, F, F, 0, 0, 0, 0], [0, 0, 0, -1, -1, 1, 1, 1, 1], [0, 0, 0, 0, 0, F, 0, 0, 0])
    assert [r["n_corr"] for r in res] == [0, 203, 202, 0, 0, 0, 181, 213, 132]  # segment 1 is sequence B of test_slam_chains_reference.py
    assert [r.get("evicted") is not None for r in res] == [False] * 8 + [True]  # the camera limit works inside the restarted segment
    assert res[-1]["state"]["cam_frame"] == [6, 7, 8, 9]                         # indices along the whole chain (rule 5)
    assert min(f for f, _ in res[-1]["state"]["pt_feature"]) >= 5                # nothing of segment 0 is left (rule 4)
    assert res[4]["state"]["cam_frame"] == [0, 1, 2, 3] == res[2]["state"]["cam_frame"]   # the map stays while the sequence is lost (rule 1)


def test_a_vanishing_reprojection_error_restarts_at_every_pair(chains):
    res = chains("A", reproj_err=1e-9)
    assert _table(res) == ([0] * 6, [0, 1, 2, 3, 4, 5], [0] + [NO_MODEL] * 5)
    assert [r["n_corr"] for r in chains("A")] == [0, 203, 202, 181, 213, 246]    # the pairs themselves are fine
    assert all(r["state"]["cam_frame"] == [p, p + 1] for p, r in enumerate(res))


def test_a_map_that_runs_dry_restarts_with_too_few(chains):
    res = chains("A", max_point_norm=1e-6, max_cameras=3)
    assert _table(res) == ([0] * 6, [0, 0, 0, 1, 1, 1], [0, 0, 0, TOO_FEW, 0, 0])
    assert [len(r["state"]["points"]) > 0 for r in res] == [True, True, False, True, True, False]   # the eviction at pairs 2 and 5 empties the map
    assert [r["n_corr"] for r in res][3] == 0 and min(r["n_corr"] for r in (res[1], res[2], res[4], res[5])) > 50


def test_lost_head_and_lost_tail(chains):
    F = R.FAILED
    res = chains("HEAD")
    assert _table(res) == ([F, 0, 0], [-1, 0, 0], [0, F, 0]) and res[-1]["state"]["cam_frame"] == [1, 2, 3]
    res = chains("TAIL")
    assert _table(res) == ([0, 0, 0, F], [0, 0, 0, -1], [0, 0, 0, 0]) and res[-1]["state"]["cam_frame"] == [0, 1, 2, 3]
    assert res[-1]["state"] is res[-2]["state"]                                  # the map a chain that ends lost leaves (rule 6)


def _flat(P):
    pp = np.arange((P + 1) * 12, dtype=np.float64).reshape(P + 1, 12)
    return pp, -pp, 1000 + np.arange(P * 12, dtype=np.float64).reshape(P, 12), -(1000 + np.arange(P * 12, dtype=np.float64).reshape(P, 12))


@pytest.mark.parametrize("segment, want", [
    ([0, 0, 0], [(0, 3)]),                                                       # one segment from the first pair
    ([-1, -1, 0, 0], [(2, 2)]),                                                  # lost head
    ([0, 0, -1, -1], [(0, 2)]),                                                  # lost tail
    ([0, 1, 1, -1, 2], [(0, 1), (1, 2), (4, 1)]),                                # one-pair segments, a restart in the same step, a lost stretch
    ([-1, -1], []),                                                              # nothing ever localised
])
def test_split_segments(segment, want):
    from visual_odometry_amd.frontend import split_segments
    P = len(segment)
    pp, pl, sp, sl = _flat(P)
    out = split_segments(np.array(segment, np.int32), pp, pl, sp, sl)
    assert [(s["first_pair"], s["n_pairs"]) for s in out] == want
    for s in out:
        a, n = s["first_pair"], s["n_pairs"]
        assert s["poses_pnp"].shape == s["poses"].shape == (n + 1, 3, 4)
        assert np.array_equal(s["poses_pnp"][0].ravel(), sp[a]) and np.array_equal(s["poses"][0].ravel(), sl[a])      # the first camera's own row
        assert np.array_equal(s["poses_pnp"][1:].reshape(n, 12), pp[a + 1:a + n + 1]) and np.array_equal(s["poses"][1:].reshape(n, 12), pl[a + 1:a + n + 1])
    if out:
        pp[:] = 0                                                                # copies
        assert out[0]["poses_pnp"][1:].any()


def test_split_segments_refuses_what_the_library_cannot_return():
    from visual_odometry_amd.frontend import split_segments
    pp, pl, sp, sl = _flat(3)
    with pytest.raises(ValueError):
        split_segments([0, 2, 2], pp, pl, sp, sl)                                # segments are numbered in order of start
    with pytest.raises(ValueError):
        split_segments([0, 0], pp, pl, sp, sl)                                   # 2 pairs, 4 pose rows

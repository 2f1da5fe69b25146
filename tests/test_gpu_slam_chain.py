"""GPU: vo_slam_chain (FrontEnd.slam_chain) — the localisation chain with the map's per-frame bundle adjustment, filter and camera
limit on the device — against tests/slam_reference.py, stage by stage ON IDENTICAL INPUTS: every comparison starts the checker
from the device's own snapshot of the previous stage (slam_chain(snapshot=(pair, stage)) + slam_map(1)), so that a discrete
decision (a RANSAC winner, an observation at the filter threshold, an LM accept at the rounding floor) cannot be turned by
drift accumulated over earlier frames.

Sequence: synth.sequence(7, 640, 480, step=4.0) / 1000 features, the chain test's small shape, with max_cameras = 4 so that pairs
3, 4 and 5 each evict a camera.  The free-running checker on the CPU (tests/test_slam_reference.py) localises every pair of it,
evicts at pairs 3, 4, 5, and every eviction removes points left with one observation (201 / 224 / 224) and keeps a point without
any — so this sequence is used, not the larger fallback.

Bundle adjustment against the numpy LM (tests/ba_reference.lm) follows the rule of tests/test_gpu_bundle_adjust.py: same
iterations and trials, every quantity within 100 x the order floor of two summation orders, floored at 1e-12 relative; t and
X divided by |t| of the last camera where fewer than two cameras are fixed (scale is free).  On the CPU chain two summation
orders of the numpy LM agree for every pair at 8 iterations, for pairs 1-5 at 14 and for pairs 2, 3, 4 at 40; pair 0 (two
cameras, converges in about 10 iterations) and pair 1 reach the rounding floor before iteration 40 and pair 5 at iteration 37,
where accept / reject is decided by the last bit of chi2.  Tested: pairs 0, 1 and 3 (the pairs of the bookkeeping test) and 4 (a
second evicting pair) — pair 0 after 8, pairs 1 and 3 after 14, pair 4 after the reference's 40 iterations; none is left out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_reference as BA  # noqa: E402
import slam_reference as S  # noqa: E402
from test_gpu_chain import _advances_along_a_line  # noqa: E402
from test_pnp_control_reference import CHAIN_PNP  # noqa: E402

pytestmark = pytest.mark.gpu

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
OUT_KEYS = ("poses_pnp", "poses", "chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")


def _pair_inputs(fe, res, X, n_pairs):
    """Every pair's input for the checker from what the device's pair path produced (frames numbered along the chain)."""
    feats = [fe.features(f)["xy"].astype(np.float64) for f in range(n_pairs + 1)]
    out = []
    for p in range(n_pairs):
        qi, ti, _, mask = fe.pair_matches(p)
        inl = mask > 0
        pr = dict(frame1=p, frame2=p + 1, q=qi[inl], t=ti[inl], p1=feats[p][qi[inl]], p2=feats[p + 1][ti[inl]])
        if p == 0:
            pr.update(R=res["R"][0].reshape(3, 3).copy(), t_rel=res["t"][0].copy(), X=X[0][:, :int(inl.sum())].copy())
        out.append(pr)
    return out


class Run:
    """The resident pair results of the sequence and slam_chain runs on them, cached by their options."""

    def __init__(self):
        from visual_odometry_amd import synth
        from visual_odometry_amd.frontend import FrontEnd
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        self.K = seq["K"]
        self.fe = FrontEnd(H, W, max_frames=N, max_pairs=N - 1, nfeatures=NFEAT)
        self.fe.upload(seq["frames"]); self.fe.detect(0, N)
        res, X = self.fe.run_pairs([[k, k + 1] for k in range(N - 1)], self.K, want_points=True)
        assert res["status"].tolist() == [0] * (N - 1)
        self.pin = _pair_inputs(self.fe, res, X, N - 1)
        self.cache = {}

    def chain(self, snapshot=None, **opts):
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (snapshot, tuple(sorted(opts.items())))
        if key not in self.cache:
            out = self.fe.slam_chain(N - 1, self.K, snapshot=snapshot, **opts)
            self.cache[key] = (out, self.fe.slam_map(1) if snapshot is not None else self.fe.slam_map(0))
        return self.cache[key]

    def snap(self, pair, stage, **opts):
        return self.chain(snapshot=(pair, stage), **opts)[1]

    def mapper(self, upto):
        """VisualSlam.feature_mapper after the pairs before `upto`."""
        s = S.empty_state()
        for pr in self.pin[:upto]:
            S.update_feature_mapper(s, pr)
        return s["mapper"]


@pytest.fixture(scope="module")
def run():
    return Run()


def _same_map(a, b, keys=S.MAP_KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def _problem(m):
    return m["cam_pose"], m["cam_fixed"], m["points"], m["obs_cam"], m["obs_pt"], m["obs_xy"]


@pytest.mark.parametrize("free_cameras", [2, 1, 3])
def test_bookkeeping_is_the_hosts_exactly(run, free_cameras):
    """k_slam_ba_prepare: the existing vo_bundle_adjust (host bookkeeping) on the map before BA returns the bytes the resident
    BA left — the same kernel on the same lists.  Pairs 0, 1 and the first evicting pair."""
    from visual_odometry_amd import map_filters as mf
    K = run.K
    for p in (0, 1, 3):
        out, before = run.chain(snapshot=(p, 1), free_cameras=free_cameras)
        after = run.snap(p, 2, free_cameras=free_cameras)
        assert int((~before["cam_fixed"]).sum()) == (1 if p == 0 else min(free_cameras, p + 2))
        g = mf.bundle_adjust(*_problem(before), K[0, 0], K[0, 2], K[1, 2], iterations=40, huber_delta=1.0, ctx=run.fe.ctx)
        assert g["status"] == 0
        assert np.array_equal(g["poses"].reshape(-1, 3, 4), after["cam_pose"]) and np.array_equal(g["points"], after["points"])
        assert (g["chi2_before"], g["chi2_after"]) == tuple(out["chi2"][p]) and g["chi2_after"] < g["chi2_before"]
        assert (g["iterations"], g["trials"]) == (out["ba_iterations"][p], out["ba_trials"][p])
        _same_map(before, after, ("cam_frame", "cam_fixed", "pt_feature", "obs_cam", "obs_pt", "obs_xy"))
        assert not np.array_equal(before["points"], after["points"])


def test_map_building_follows_the_reference(run, oracle, kernel_dk_rule):
    """add_information_to_map with its observations, freeze_nonlast_cameras, and the PnP that reads the refined map: the
    checker's step from the device's map after pair p - 1 gives the device's map before pair p's bundle adjustment."""
    K = run.K
    out, first = run.chain(snapshot=(0, 1))
    r = S.step(oracle, S.empty_state(), run.pin[0], K, dict(max_cameras=MAX_CAMERAS), stages=True)
    _same_map(r["stage"][1], first, ("cam_frame", "cam_fixed", "pt_feature", "points", "obs_cam", "obs_pt", "obs_xy"))
    assert np.abs(r["stage"][1]["cam_pose"] - first["cam_pose"]).max() < 1e-6
    assert np.array_equal(out["poses_pnp"][:2], first["cam_pose"]) and first["cam_fixed"].tolist() == [True, False]
    assert out["n_pts"][0] == len(first["points"]) == len(run.pin[0]["q"]) and out["n_obs"][0] == 2 * out["n_pts"][0]
    for p in range(1, N - 1):
        prev = run.snap(p - 1, 4)
        out, cur = run.chain(snapshot=(p, 1))
        state = S.to_lists(prev, mapper=run.mapper(p))
        r = S.step(oracle, state, run.pin[p], K, dict(max_cameras=MAX_CAMERAS), follow=out["poses_pnp"][p + 1], stages=True)
        want = r["stage"][1]
        assert r["status"] == 0 == out["status"][p] and (r["n_corr"], r["n_inl"]) == (out["n_corr"][p], out["n_inl"][p])
        assert np.abs(r["pose_pnp"] - out["poses_pnp"][p + 1]).max() < 1e-6
        _same_map(want, cur, ("cam_frame", "cam_fixed", "pt_feature", "obs_cam", "obs_pt", "obs_xy"))
        n_old = len(prev["points"])
        assert len(cur["points"]) > n_old and len(cur["obs_cam"]) > len(prev["obs_cam"])
        assert np.array_equal(cur["points"][:n_old], prev["points"]) and np.array_equal(cur["cam_pose"][:-1], prev["cam_pose"])
        assert np.array_equal(cur["cam_pose"][-1], out["poses_pnp"][p + 1])
        assert np.abs(want["points"][n_old:] - cur["points"][n_old:]).max() < 1e-6
        # both kinds of inlier occur: observations of existing points (one each) and new points (two each)
        added = len(cur["obs_cam"]) - len(prev["obs_cam"])
        assert added > 2 * (len(cur["points"]) - n_old) > 0


def test_pnp_options_reach_the_kernel(run, oracle, kernel_dk_rule):
    """iterations / reproj_err / confidence / seed none of which is a default (bundle adjustment, filter and camera limit on):
    every pair localises, and the checker's step with the same options from the device's map after pair p - 1 localises pair p
    as the device did, by the rule of the test above."""
    K = run.K
    opts = dict(max_cameras=MAX_CAMERAS, **CHAIN_PNP)
    default, got = run.chain()[0], run.chain(**CHAIN_PNP)[0]
    assert got["status"].tolist() == [0] * (N - 1)
    assert got["n_inl"].tolist() != default["n_inl"].tolist()              # the options reached the kernel
    for p in range(1, N - 1):
        prev = run.snap(p - 1, 4, **CHAIN_PNP)
        out, cur = run.chain(snapshot=(p, 1), **CHAIN_PNP)
        state = S.to_lists(prev, mapper=run.mapper(p))
        r = S.step(oracle, state, run.pin[p], K, opts, follow=out["poses_pnp"][p + 1], stages=True)
        assert r["status"] == 0 == out["status"][p] and (r["n_corr"], r["n_inl"]) == (out["n_corr"][p], out["n_inl"][p]), p
        assert np.abs(r["pose_pnp"] - out["poses_pnp"][p + 1]).max() < 1e-6, p
        _same_map(r["stage"][1], cur, ("cam_frame", "cam_fixed", "pt_feature", "obs_cam", "obs_pt", "obs_xy"))


def test_filter_is_the_reprojection_oracle(run, oracle):
    K = run.K
    dropped = kept = 0
    for p in range(1, N - 1):
        a, b = run.snap(p, 2), run.snap(p, 3)
        keep = S.reprojection_keep(oracle, a, K, 1.0)
        for k in ("obs_cam", "obs_pt", "obs_xy"):
            assert np.array_equal(a[k][keep], b[k]), (p, k)
        _same_map(a, b, ("cam_frame", "cam_pose", "cam_fixed", "pt_feature", "points"))          # points are not removed here
        dropped += int((~keep).sum()); kept += int(keep.sum())
    assert dropped > 0 and kept > 0
    a, b = run.snap(0, 2), run.snap(0, 3)                                                          # no filter after initialize_map
    _same_map(a, b)


def test_camera_limit_is_remove_camera_from_map(run):
    removed = zero_kept = 0
    for p in range(0, N - 1):
        a, b = run.snap(p, 3), run.snap(p, 4)
        s = S.to_lists(a)
        info = S.limit_number_of_camera_in_map(s, MAX_CAMERAS)
        assert (info is not None) == (p >= 3)
        _same_map(S.to_arrays(s), b)
        if info:
            removed += info["points_removed"]; zero_kept += info["zero_observation_points_kept"]
            per_point = np.bincount(b["obs_pt"], minlength=len(b["points"]))
            assert not (per_point == 1).any() and (per_point == 0).sum() == info["zero_observation_points_kept"]
    assert removed > 0 and zero_kept > 0
    out, final = run.chain()
    assert out["n_cam"].tolist() == [2, 3, 4, 4, 4, 4] and final["cam_frame"].tolist() == [3, 4, 5, 6]
    # a removed point leaves mappointdict: its feature id is not a map point any more, and every camera's last pose is reported
    assert len({tuple(v) for v in final["pt_feature"]}) == len(final["points"]) == out["n_pts"][-1]
    assert np.array_equal(out["poses"][3:], final["cam_pose"]) and np.abs(out["poses"][:3]).max() > 0


@pytest.mark.parametrize("pair,iterations", [(0, 8), (1, 14), (3, 14), (4, 40)])
def test_bundle_adjustment_against_the_numpy_lm(run, pair, iterations):
    K = run.K
    out, before = run.chain(snapshot=(pair, 1), ba_iterations=iterations)
    after = run.snap(pair, 2, ba_iterations=iterations)
    prob, kw = _problem(before), dict(f=K[0, 0], cx=K[0, 2], cy=K[1, 2], iterations=iterations, delta=1.0)
    normalise = int(before["cam_fixed"].sum()) < 2
    ref = BA.lm(*prob, **kw)
    alt = BA.lm(*prob, order=np.random.default_rng(1000 + pair).permutation(len(before["obs_cam"])), **kw)
    assert ref["accepts"] == alt["accepts"], "not a parity case: two CPU summation orders take different accept / reject decisions"
    qr, qa = (BA.quantities(r["poses"], r["points"], r["chi2_after"], normalise) for r in (ref, alt))
    floor = {k: float(np.abs(qr[k] - qa[k]).max()) for k in qr}
    tol = BA.tolerances(ref, floor, normalise)
    qg = BA.quantities(after["cam_pose"], after["points"], out["chi2"][pair, 1], normalise)
    diff = {k: float(np.abs(qg[k] - qr[k]).max()) for k in qg}
    print("pair", pair, "it/trials", out["ba_iterations"][pair], out["ba_trials"][pair], "chi2", ref["chi2_before"], "->", ref["chi2_after"],
          "| floor", floor, "| tol", tol, "| gpu - ref", diff)
    assert (out["ba_iterations"][pair], out["ba_trials"][pair]) == (ref["iterations"], ref["trials"])
    assert abs(out["chi2"][pair, 0] - ref["chi2_before"]) <= 1e-12 * ref["chi2_before"]
    for k in diff:
        assert diff[k] <= tol[k], (k, diff[k], tol[k])


def test_links_to_the_chain_without_a_map_step(run):
    """BA, filter and limit switched off: vo_tracks_pnp_batch's poses and counts, byte for byte; two calls: identical bytes."""
    K = run.K
    out, m = run.chain(ba_iterations=0, filter_threshold=0.0, max_cameras=N)
    lc = run.fe.localize_chain(N - 1, K)
    assert np.array_equal(out["poses_pnp"], lc["poses"]) and np.array_equal(out["poses"], lc["poses"])
    for k in ("n_corr", "n_inl", "status"):
        assert np.array_equal(out[k], lc[k]), k
    assert np.array_equal(out["n_pts"], lc["n_map"]) and out["n_cam"].tolist() == list(range(2, N + 1))
    assert not out["chi2"].any() and not out["ba_iterations"].any() and len(m["points"]) == lc["n_map"][-1]
    a = run.fe.slam_chain(N - 1, K, max_cameras=MAX_CAMERAS, snapshot=(4, 2)); ma, sa = run.fe.slam_map(0), run.fe.slam_map(1)
    b = run.fe.slam_chain(N - 1, K, max_cameras=MAX_CAMERAS, snapshot=(4, 2)); mb, sb = run.fe.slam_map(0), run.fe.slam_map(1)
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), k
    _same_map(ma, mb); _same_map(sa, sb)
    assert a["status"].tolist() == [0] * (N - 1) and (a["chi2"][:, 1] < a["chi2"][:, 0]).all()
    # the snapshot does not alter the run
    c, mc = run.chain()
    for k in OUT_KEYS:
        assert np.array_equal(a[k], c[k]), k
    _same_map(ma, mc)


def test_a_shorter_chain_is_a_prefix(run):
    from visual_odometry_amd.frontend import FrontEnd
    from visual_odometry_amd import synth
    n = 4
    seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
    fe = FrontEnd(H, W, max_frames=N, max_pairs=N - 1, nfeatures=NFEAT)
    fe.upload(seq["frames"]); fe.detect(0, N)
    fe.run_pairs([[k, k + 1] for k in range(n)], run.K, want_points=True)
    short = fe.slam_chain(n, run.K, max_cameras=MAX_CAMERAS)
    full, _ = run.chain()
    for k in OUT_KEYS:
        if k not in ("poses_pnp", "poses"):
            assert np.array_equal(short[k], full[k][:n]), k
    assert np.array_equal(short["poses_pnp"], full["poses_pnp"][:n + 1])
    _same_map(fe.slam_map(0), run.snap(n - 1, 4))
    fe.ctx.close()


def test_rejections_and_a_chain_that_stops():
    from visual_odometry_amd import _lib, synth
    from visual_odometry_amd.frontend import FrontEnd, MATCH_RATIO
    seq = synth.sequence(4, 640, 480, cache_dir="/tmp")
    K = seq["K"]
    c = _lib.Context(0)
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=3, nfeatures=500, ctx=c)
    fe.upload(seq["frames"]); fe.detect(0, 4)
    chain = [[0, 1], [1, 2], [2, 3]]

    def refused(code, n=3, **kw):
        with pytest.raises(_lib.VoError) as e:
            fe.slam_chain(n, K, **kw)
        assert e.value.code == code, (e.value.code, code)

    fe.run_pairs(chain, K, opts=fe.make_opts(match_mode=MATCH_RATIO, want_points=True))
    refused(_lib.VO_ERR_UNSUPPORTED)                                       # ratio matches are not one-to-one
    assert fe.localize_chain(3, K)["status"][0] == 0                       # what vo_tracks_pnp_batch accepts has not changed
    fe.run_pairs(chain[:2], K, want_points=False)
    refused(_lib.VO_ERR_INVALID, n=2)                                      # no triangulated points in HBM
    fe.run_pairs([[0, 1], [2, 3]], K, want_points=True)
    refused(_lib.VO_ERR_INVALID, n=2)                                      # not a chain
    fe.run_pairs(chain, K, want_points=True)
    refused(_lib.VO_ERR_INVALID, n=2)                                      # all pairs of the run, not a part of them
    refused(_lib.VO_ERR_UNSUPPORTED, max_cameras=_lib.VO_BA_MAX_CAMERAS)   # max_cameras + 1 cameras before the limit
    refused(_lib.VO_ERR_INVALID, free_cameras=0)
    refused(_lib.VO_ERR_UNSUPPORTED, free_cameras=_lib.VO_BA_MAX_FREE + 1)
    refused(_lib.VO_ERR_INVALID, max_cameras=1)
    refused(_lib.VO_ERR_INVALID, snapshot=(3, 1))
    with pytest.raises(_lib.VoError):                                      # a refused call leaves no map behind
        fe.slam_map(0)
    out = fe.slam_chain(3, K, max_cameras=_lib.VO_BA_MAX_CAMERAS - 1, free_cameras=_lib.VO_BA_MAX_FREE)
    assert out["status"].tolist() == [0, 0, 0] and out["n_cam"].tolist() == [2, 3, 4]
    assert len(fe.slam_map(0)["cam_frame"]) == 4
    with pytest.raises(_lib.VoError):                                      # no snapshot was asked for
        fe.slam_map(1)
    # a chain that cannot continue: frame 2 is blank, pair (1, 2) fails in vo_pairs_run, the chain stops there with today's statuses
    frames = seq["frames"].copy(); frames[2] = 127
    fe.upload(frames); fe.detect(0, 4)
    res, _ = fe.run_pairs(chain, K, want_points=True)
    assert res["status"][1] != 0
    lc = fe.localize_chain(3, K)
    out = fe.slam_chain(3, K, snapshot=(2, 4))
    assert out["status"].tolist() == lc["status"].tolist() == [0, res["status"][1], _lib.VO_ERR_NOT_CONFIGURED]
    assert np.all(out["poses"][2:] == 0) and np.all(out["poses_pnp"][2:] == 0) and np.abs(out["poses"][:2]).max() > 0
    m = fe.slam_map(0)
    assert out["n_cam"].tolist() == [2, 2, 2] and out["n_pts"].tolist() == [len(m["points"])] * 3 and out["n_obs"].tolist() == [len(m["obs_cam"])] * 3
    assert m["cam_frame"].tolist() == [0, 1] and len(m["obs_cam"]) == 2 * len(m["points"]) > 0
    assert m["obs_cam"].max() == 1 and m["obs_pt"].max() == len(m["points"]) - 1
    for k in S.MAP_KEYS:
        assert np.array_equal(m[k], fe.slam_map(1)[k]), k                  # the snapshot of a stopped chain: the map as it stands
    assert out["chi2"][0, 1] < out["chi2"][0, 0] and not out["chi2"][1:].any()
    # a configure call forgets both maps, like the last run
    f2 = FrontEnd(480, 640, max_frames=2, max_pairs=1, nfeatures=500, ctx=c)
    for which in (0, 1):
        with pytest.raises(_lib.VoError) as e:
            f2.slam_map(which)
        assert e.value.code == _lib.VO_ERR_INVALID
    with pytest.raises(_lib.VoError):
        f2.slam_chain(1, K)
    c.close()


def test_physical_sense_with_the_defaults(oracle):
    """1280 x 720, 5 frames, 2000 features, the reference's defaults: with bundle adjustment after every frame the cameras advance
    along a line in steps of about one unit (the free-running checker on the CPU satisfies the same rule on this sequence)."""
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    n = 5
    seq = synth.sequence(n, 1280, 720, step=4.0, cache_dir="/tmp")
    fe = FrontEnd(720, 1280, max_frames=n, max_pairs=n - 1, nfeatures=2000)
    fe.upload(seq["frames"]); fe.detect(0, n)
    fe.run_pairs([[k, k + 1] for k in range(n - 1)], seq["K"], want_points=True)
    out = fe.slam_chain(n - 1, seq["K"])
    assert out["status"].tolist() == [0] * (n - 1) and out["n_cam"].tolist() == [2, 3, 4, 5]
    assert (out["chi2"][:, 1] < out["chi2"][:, 0]).all() and out["ba_iterations"].min() >= 1
    _advances_along_a_line(out["poses"])
    fe.ctx.close()

"""GPU: the localisation chain (k_chain_link / init / gather, k_pnp_ransac on gathered points, k_chain_pose / triangulate / insert) and
the resident map step (k_slam_add / filter / limit and their _seqs forms) on feature tracks the test CHOSE: descriptor rows and
keypoint positions go into the slots through FrontEnd.set_orb_rows, built by tests/track_cases.py so that every pair's match list
and E inliers are known and the tracks have a stated structure — full-length tracks, births, deaths, a skipped frame, a track cut
by an E outlier; inlier rank != match index on both sides of the wave and round edges (63 .. 65, 255 .. 257, 511 .. 513 inliers);
0 .. 6 gathered correspondences; a failed pair inside the chain; points beyond max_point_norm whose tracks go on; evictions under
max_cameras = 3 with re-born points; two queries that share a train row (MATCH_NEAREST).  tests/test_track_cases_reference.py
holds on the CPU that each case reaches what it is named for and that the cases tell six slips of the bookkeeping apart.

Compared:
  localize_chain against reference_chain(follow = the device's poses): status, n_corr, n_inl, n_map equal, poses within 1e-6;
  slam_chain with bundle adjustment, filter and limit off against localize_chain: byte for byte (one-to-one cases);
  slam_chain stage by stage from the device's own snapshots (the method of tests/test_gpu_slam_chain.py): stage 1 against
    slam_reference.step on the stage-4 snapshot of the pair before (lists equal, new points within 1e-6), stage 3 against
    reprojection_keep on the stage-2 snapshot, stage 4 against limit_number_of_camera_in_map on the stage-3 snapshot, both equal;
    ba_iterations = 0 but for the eviction case's second run, where the next pair's gather reads what the bundle adjustment wrote back;
  slam_chains: three cases of different lengths in one call, forwards and reversed, each sequence byte for byte its own slam_chain.
The device runs the 300-sweep root finder (set_poly_solver("opencv300")) against the oracle's, so the cases are on the device the
cases the CPU file pinned.  The frame is 64 x 64 with one pyramid level, kp_cap 264 (768 for the round edges); one run_pairs per
case and front end.

k_chain_insert took its decision and wrote in one pass; it now decides against the map as it was before the loop, as the reference
and k_slam_add do.  The slip was found by reading, and only `many_to_one` can show it (two waves of one round); the window is a few
instructions wide.  No case differed before the change: with the one-pass kernel `many_to_one` gave n_map = [256, 262, 262] on an
MI355X too (one run; a run is not repeated to make a race show).

The whole file takes 3.7 - 4.5 s on an MI355X (measured, two runs, the oracle's side included); the slowest test 0.4 s."""
import numpy as np
import pytest

import slam_reference as S
import track_cases as TC
from test_gpu_chain import reference_chain

pytestmark = pytest.mark.gpu

H = W = 64
OUT_KEYS = ("poses_pnp", "poses", "chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")
LISTS = ("cam_frame", "cam_fixed", "pt_feature", "obs_cam", "obs_pt", "obs_xy")
NAMES = list(TC.cases())
ONE_TO_ONE = [n for n, c in TC.cases().items() if c.match_mode == TC.MATCH_CROSSCHECK]
STAGED = [n for n in ONE_TO_ONE if TC.cases()[n].want["status"][0] == 0 and TC.cases()[n].group != "failed_pair"]
BOOKKEEPING = dict(ba_iterations=0, filter_threshold=1.0, max_cameras=4)     # for the cases that bring no options of their own


@pytest.fixture
def faithful(oracle):
    assert not oracle.get_dk_early_exit()
    return oracle


class Launch:
    """A front end whose slots hold one or more cases, and ONE run_pairs over all their pairs (sequence after sequence)."""

    def __init__(self, O, cases):
        from visual_odometry_amd import _lib
        from visual_odometry_amd.frontend import FrontEnd
        assert (TC.VO_OK, TC.VO_ERR_TOO_FEW, TC.VO_ERR_NO_MODEL, TC.VO_ERR_NOT_CONFIGURED) == (_lib.VO_OK, _lib.VO_ERR_TOO_FEW, _lib.VO_ERR_NO_MODEL, _lib.VO_ERR_NOT_CONFIGURED)
        assert len({(c.nfeatures, c.match_mode) for c in cases}) == 1
        self.cases = cases
        n_frames, n_pairs = sum(c.n for c in cases), sum(c.n - 1 for c in cases)
        self.fe = fe = FrontEnd(H, W, max_frames=n_frames, max_pairs=n_pairs, nfeatures=cases[0].nfeatures, nlevels=1)
        assert fe.kp_cap == cases[0].kp_cap
        fe.ctx.set_poly_solver("opencv300")
        pairs, self.first_pair, slot = [], [], 0
        for c in cases:
            for k, f in enumerate(TC.frames(O, c)):
                fe.set_orb_rows(slot + k, f["desc"], f["xy"])
            self.first_pair.append(len(pairs))
            pairs += [[slot + k, slot + k + 1] for k in range(c.n - 1)]
            slot += c.n
        from visual_odometry_amd import frontend
        assert (frontend.MATCH_CROSSCHECK, frontend.MATCH_NEAREST) == (TC.MATCH_CROSSCHECK, TC.MATCH_NEAREST)
        opts = fe.make_opts(match_mode=cases[0].match_mode, want_points=True)
        res, X = fe.run_pairs(pairs, TC.K, opts, want_points=True)
        self.res, self.X = res.copy(), X.copy()
        for c, first in zip(cases, self.first_pair):                       # the pair path gave the intended matches and E inliers
            for k in range(c.n - 1):
                qi, ti = TC.matches(c, k)
                q, t, _, mask = fe.pair_matches(first + k)
                assert np.array_equal(q, qi) and np.array_equal(t, ti), (c.name, k)
                ok = len(qi) >= 5
                assert (int(self.res["status"][first + k]) == 0) == ok, (c.name, k)
                if ok:
                    assert np.array_equal(mask > 0, TC.e_inliers(c, k)), (c.name, k)

    def close(self):
        self.fe.ctx.close()


def _pair_inputs(O, L, c):
    """Every pair's input for the checker from what the device's pair path produced (tests/test_gpu_slam_chain.py does the same)."""
    fr, out = TC.frames(O, c), []
    for p in range(c.n - 1):
        qi, ti, _, mask = L.fe.pair_matches(p)
        inl = mask > 0
        pr = dict(frame1=p, frame2=p + 1, q=qi[inl], t=ti[inl], p1=fr[p]["xy"][qi[inl]].astype(np.float64), p2=fr[p + 1]["xy"][ti[inl]].astype(np.float64))
        if p == 0:
            pr.update(R=L.res["R"][0].reshape(3, 3).copy(), t_rel=L.res["t"][0].copy(), X=L.X[0][:, :int(inl.sum())].copy())
        out.append(pr)
    return out


def _status(want):
    return [TC.VO_ERR_NOT_CONFIGURED if s is None else s for s in want]


# ------------------------------------------------------------------ the chain
@pytest.mark.parametrize("name", NAMES)
def test_localize_chain_is_the_dict_walk(faithful, name):
    c = TC.cases()[name]
    L = Launch(faithful, [c])
    try:
        got = L.fe.localize_chain(c.n - 1, TC.K)
        want = reference_chain(faithful, TC.feats(faithful, c), c.pairs, TC.K, follow=got["poses"],
                               match_mode=2 if c.match_mode == TC.MATCH_CROSSCHECK else 0, failed_pairs=True)
        print(name, {k: got[k].tolist() for k in ("status", "n_corr", "n_inl", "n_map")})
        assert [int(v) for v in L.res["n_inl"]] == want["E_inl"] == c.want["E_inl"]
        assert got["status"].tolist() == _status(want["status"]) == _status(c.want["status"])
        assert got["n_corr"].tolist() == want["n_corr"] == c.want["n_corr"]
        assert got["n_inl"].tolist() == want["n_inl"]
        assert got["n_map"].tolist() == want["n_map"] == c.want["n_map"]
        for k in range(c.n):
            assert np.abs(got["poses"][k] - want["poses"][k]).max() < 1e-6, (name, k)
            if k >= 1 and got["status"][k - 1] != 0:
                assert not got["poses"][k].any()
    finally:
        L.close()


@pytest.mark.parametrize("name", ONE_TO_ONE)
def test_slam_chain_without_a_map_step_is_localize_chain(faithful, name):
    c = TC.cases()[name]
    L = Launch(faithful, [c])
    try:
        lc = L.fe.localize_chain(c.n - 1, TC.K)
        out = L.fe.slam_chain(c.n - 1, TC.K, ba_iterations=0, filter_threshold=0.0, max_cameras=c.n)
        assert out["poses_pnp"].tobytes() == lc["poses"].tobytes() and out["poses"].tobytes() == lc["poses"].tobytes()
        for k in ("n_corr", "n_inl", "status"):
            assert out[k].tobytes() == lc[k].tobytes(), k
        assert out["n_pts"].tobytes() == lc["n_map"].tobytes()
        assert len(L.fe.slam_map(0)["points"]) == lc["n_map"][-1]
    finally:
        L.close()


# ------------------------------------------------------------------ the map step, stage by stage
def _same_map(a, b, keys=S.MAP_KEYS, what=""):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k)


def _stages(O, c, opts):
    """Every pair's four stages on identical inputs.  Returns per localised pair the eviction info of the device's own stage-3 map
    and, per pair, how many zero-observation points the pair before left that this pair gathered."""
    L = Launch(O, [c])
    try:
        fe, n = L.fe, c.n - 1
        pin = _pair_inputs(O, L, c)

        def snap(p, stage):
            out = fe.slam_chain(n, TC.K, snapshot=(p, stage), **opts)
            return out, fe.slam_map(1)

        step_opts = dict(opts, ba_iterations=0)                            # stage 1 does not read them; the numpy LM is not run for it
        out, first = snap(0, 1)
        r = S.step(O, S.empty_state(), pin[0], TC.K, step_opts, stages=True)
        _same_map(r["stage"][1], first, LISTS + ("points",), (c.name, 0))
        assert np.abs(r["stage"][1]["cam_pose"] - first["cam_pose"]).max() < 1e-6
        evicted, gathered_zero = [], []
        mapper = S.empty_state()
        for p in range(n):
            S.update_feature_mapper(mapper, pin[p])
            if p >= 1:
                _, prev = snap(p - 1, 4)
                out, cur = snap(p, 1)
                state = S.to_lists(prev, mapper={k: v for k, v in mapper["mapper"].items() if k[0] <= p})
                r = S.step(O, state, pin[p], TC.K, step_opts, follow=out["poses_pnp"][p + 1], stages=True)
                assert r["status"] == out["status"][p] and (r["n_corr"], r["n_inl"]) == (out["n_corr"][p], out["n_inl"][p]), (c.name, p)
                if r["status"] != 0:
                    assert all(s == TC.VO_ERR_NOT_CONFIGURED for s in out["status"][p + 1:])
                    _same_map(prev, cur, what=(c.name, p))               # a pair that is not localised leaves the map as it was
                    break
                assert np.abs(r["pose_pnp"] - out["poses_pnp"][p + 1]).max() < 1e-6, (c.name, p)
                want = r["stage"][1]
                _same_map(want, cur, LISTS, (c.name, p))
                n_old = len(prev["points"])
                assert np.array_equal(cur["points"][:n_old], prev["points"]) and np.array_equal(cur["cam_pose"][:-1], prev["cam_pose"])
                assert np.array_equal(cur["cam_pose"][-1], out["poses_pnp"][p + 1])
                assert np.abs(want["points"][n_old:] - cur["points"][n_old:]).max(initial=0.0) < 1e-6, (c.name, p)
                zero = set(np.flatnonzero(np.bincount(prev["obs_pt"], minlength=n_old) == 0).tolist())
                gathered_zero.append(int(np.isin(cur["obs_pt"][len(prev["obs_cam"]):], list(zero)).sum()) if zero else 0)
            _, a = snap(p, 2)
            _, b = snap(p, 3)
            if p >= 1 and opts["filter_threshold"] > 0:
                keep = S.reprojection_keep(O, a, TC.K, opts["filter_threshold"])
                for k in ("obs_cam", "obs_pt", "obs_xy"):
                    assert np.array_equal(a[k][keep], b[k]), (c.name, p, k)
                _same_map(a, b, ("cam_frame", "cam_pose", "cam_fixed", "pt_feature", "points"), (c.name, p))
            else:
                _same_map(a, b, what=(c.name, p))
            _, d = snap(p, 4)
            s = S.to_lists(b)
            info = S.limit_number_of_camera_in_map(s, opts["max_cameras"])
            _same_map(S.to_arrays(s), d, what=(c.name, p))
            evicted.append(info and (info["points_removed"], info["zero_observation_points_kept"]))
        return out, evicted, gathered_zero
    finally:
        L.close()


@pytest.mark.parametrize("name", [n for n in STAGED if not TC.cases()[n].opts.get("ba_iterations")])
def test_map_step_stage_by_stage(faithful, name):
    c = TC.cases()[name]
    opts = dict(BOOKKEEPING); opts.update(c.opts)
    out, evicted, _ = _stages(faithful, c, opts)
    print(name, out["status"].tolist(), out["n_pts"].tolist(), evicted)
    if c.opts:                                                             # the eviction case: what the CPU file pinned, on the device
        m = c.want["map"]
        assert out["status"].tolist() == m["status"] and out["n_corr"].tolist() == m["n_corr"] and out["n_pts"].tolist() == m["n_pts"]
        assert evicted == m["evicted"]
        assert sum(e[0] for e in evicted if e) > 0 and out["n_pts"][3] > out["n_pts"][2]     # points went, and their tracks got new ones


def test_eviction_with_bundle_adjustment_feeds_the_next_gather(faithful):
    """The eviction case with the bundle adjustment on: the next pair's gather reads the cameras and points the adjustment wrote
    back (stage 1 from the stage-4 snapshot holds exactly that), points without an observation survive an eviction and are
    gathered by the pair after it."""
    c = TC.cases()["eviction_with_ba"]
    out, evicted, gathered_zero = _stages(faithful, c, dict(BOOKKEEPING, **c.opts))
    print(out["status"].tolist(), out["n_corr"].tolist(), out["n_pts"].tolist(), evicted, gathered_zero, out["ba_iterations"].tolist())
    assert out["ba_iterations"][:3].min() >= 1 and (out["chi2"][:3, 1] < out["chi2"][:3, 0]).all()
    assert sum(e[1] for e in evicted if e) > 0 and sum(gathered_zero) > 0


# ------------------------------------------------------------------ several cases in one call
def test_slam_chains_three_cases_of_different_lengths(faithful):
    """eviction (6 pairs), max_point_norm (5) and n_corr_3 (3: its pair 1 is not localised, which ends that sequence alone) in one
    run_pairs and one slam_chains call, forwards and reversed: every sequence is byte for byte its own slam_chain."""
    cases = [TC.cases()[n] for n in ("eviction", "max_point_norm", "n_corr_3")]
    opts = dict(BOOKKEEPING, **cases[0].opts)
    alone = {}
    for c in cases:
        L = Launch(faithful, [c])
        try:
            alone[c.name] = (L.fe.slam_chain(c.n - 1, TC.K, **opts), L.fe.slam_map(0))
        finally:
            L.close()
    assert alone["n_corr_3"][0]["status"].tolist() == [0, TC.VO_ERR_TOO_FEW, TC.VO_ERR_NOT_CONFIGURED]
    assert alone["eviction"][0]["status"].tolist() == [0] * 6 and alone["max_point_norm"][0]["status"].tolist() == [0] * 5
    for order in (cases, cases[::-1]):
        L = Launch(faithful, order)
        try:
            outs = L.fe.slam_chains([c.n - 1 for c in order], TC.K, **opts)
            for i, c in enumerate(order):
                for k in OUT_KEYS:
                    assert outs[i][k].tobytes() == alone[c.name][0][k].tobytes(), (c.name, k)
                m = L.fe.slam_map(0, seq=i)
                for k in S.MAP_KEYS:
                    assert m[k].tobytes() == alone[c.name][1][k].tobytes(), (c.name, k)
        finally:
            L.close()

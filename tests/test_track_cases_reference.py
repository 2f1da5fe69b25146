"""CPU: every case of tests/track_cases.py reaches what it is there for, from the oracle and the two dict walks alone
(reference_chain of tests/test_gpu_chain.py, tests/slam_reference.py) — the intended match lists, the E inliers per pair, n_corr /
status / n_map along the chain, and points, observations, cameras and evictions of the map step — and the cases DISCRIMINATE: for
each of six plausible slips of the bookkeeping (MUTANTS) at least one case's expected output differs from the true walk's.
tests/test_gpu_tracks_chosen.py runs the same cases on the device; a case that drifts off its path fails here instead of passing
for nothing there.

Margins, as conditions: every keypoint moved off its line is an E outlier by 5 px and every one moved along it is moved at
least 10 px further than the threshold it is meant to fail (solvePnPRansac's 8 px, the filter's 1 px); no triangulated norm of any
case lies within max_point_norm (1 +- 1e-3); every camera the chain finds lies within 0.02 baselines of the path the scene was
built on, which is what shows that the baseline gives the five-point solver and the triangulation enough parallax."""
import numpy as np
import pytest

import slam_reference as S
import track_cases as TC
from test_gpu_chain import reference_chain

NAMES = list(TC.cases())
BA_OFF = dict(ba_iterations=0, filter_threshold=0.0, max_cameras=18)


def _opts(c):
    o = dict(BA_OFF); o.update(c.opts)
    return o


@pytest.fixture
def O(oracle):
    assert not oracle.get_dk_early_exit()
    return oracle


_CHAIN, _RUN = {}, {}


def chain_of(O, c):
    if c.name not in _CHAIN:
        _CHAIN[c.name] = reference_chain(O, TC.feats(O, c), c.pairs, TC.K, match_mode=2 if c.match_mode == TC.MATCH_CROSSCHECK else 0, failed_pairs=True)
    return _CHAIN[c.name]


def run_of(O, c):
    if c.name not in _RUN:
        _RUN[c.name] = S.run(O, TC.pair_inputs(O, c), TC.K, _opts(c))
    return _RUN[c.name]


def true_centre(k):
    """Camera k's centre in the chain's world: frame 1's camera, unit = pair 0's baseline."""
    return TC.ROT[1] @ np.array([(k - 1) * TC.STEP, 0.0, 0.0]) / TC.STEP


def test_every_group_of_the_issue_is_there():
    assert {c.group for c in TC.cases().values()} == {"tracks", "rank", "n_corr", "failed_pair", "max_norm", "eviction", "many_to_one"}
    assert sorted(c.want["E_inl"][0] for c in TC.group("rank")) == [63, 64, 65, 255, 256, 257, 511, 512, 513]
    assert all(c.kp_cap == (264 if c.want["E_inl"][0] <= 65 else 768) for c in TC.group("rank"))
    assert sorted(c.want["n_corr"][1] for c in TC.group("n_corr")) == [0, 1, 2, 3, 4, 4, 5, 6]
    assert {c.want["status"][1] for c in TC.group("n_corr") if c.want["n_corr"][1] in (4, 5, 6)} >= {0}
    assert all(c.n <= 8 and c.kp_cap in (264, 768) for c in TC.cases().values())
    assert [c.match_mode for c in TC.group("many_to_one")] == [TC.MATCH_NEAREST]
    assert all(c.match_mode == TC.MATCH_CROSSCHECK for c in TC.cases().values() if c.group != "many_to_one")


@pytest.mark.parametrize("name", NAMES)
def test_slots_give_the_intended_match_lists(O, name):
    c = TC.cases()[name]
    fr = TC.frames(O, c)                                                   # asserts the match lists against the oracle's matcher
    for k, f in enumerate(fr):
        assert f["desc"].dtype == np.uint8 and f["xy"].dtype == np.float32 and len(f["desc"]) == len(f["xy"]) <= c.kp_cap
        assert len(np.unique(f["desc"], axis=0)) == len(f["desc"])
        if k + 1 < c.n:
            qi, ti = TC.matches(c, k)
            assert np.array_equal(fr[k]["ids"][qi][fr[k]["ids"][qi] >= 0], fr[k + 1]["ids"][ti][fr[k]["ids"][qi] >= 0])
            assert len(qi) < 2 or not np.array_equal(qi, ti)             # a gather by the query index would take other points
            # a pair has leftover rows on one side at most (cross-check matching has no distance bound)
            assert c.match_mode == TC.MATCH_NEAREST or len(qi) == min(len(fr[k]["ids"]), len(fr[k + 1]["ids"]))


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_is_named_for(O, name):
    c = TC.cases()[name]
    w = c.want
    fr = TC.frames(O, c)
    r = chain_of(O, c)
    print(name, {k: r[k] for k in ("E_inl", "status", "n_corr", "n_inl", "n_map")})
    assert r["E_inl"] == w["E_inl"]
    for k in range(c.n - 1):                                               # the E inliers are the keypoints that were not moved off their line
        qi, ti = TC.matches(c, k)
        if len(qi) >= 5:
            p1 = fr[k]["xy"][qi].astype(np.float64); p2 = fr[k + 1]["xy"][ti].astype(np.float64)
            rc, _, mask, _ = O.find_essential_ransac(p1, p2, TC.K)
            assert rc == 0 and np.array_equal(mask > 0, TC.e_inliers(c, k)), (name, k)
    assert r["status"] == w["status"] and r["n_corr"] == w["n_corr"] and r["n_map"] == w["n_map"]
    if "n_inl" in w:
        assert r["n_inl"] == w["n_inl"]
    for k, P in enumerate(r["poses"]):                                     # the chain follows the path the scene was built on
        if r["status"][max(k - 1, 0)] == 0 and not w.get("off_path"):
            assert np.linalg.norm(-P[:, :3].T @ P[:, 3] - true_centre(k)) < 0.02, (name, k)
    if c.match_mode != TC.MATCH_CROSSCHECK or any(s != 0 for s in w["status"][:1]):
        return
    # the map step's checker on the same pairs
    res = run_of(O, c)
    n_ok = sum(1 for s in w["status"] if s == 0)
    if not c.opts:                                                         # no bundle adjustment, filter or limit: the chain's numbers
        assert [x["status"] for x in res] == [s for s in w["status"] if s is not None][:len(res)]
        assert [x["n_corr"] for x in res] == w["n_corr"][:len(res)] and [len(x["state"]["points"]) for x in res][:n_ok] == w["n_map"][:n_ok]
    else:
        got = dict(status=[x["status"] for x in res], n_corr=[x["n_corr"] for x in res], n_pts=[len(x["state"]["points"]) for x in res],
                   evicted=[x["evicted"] and (x["evicted"]["points_removed"], x["evicted"]["zero_observation_points_kept"]) for x in res])
        print(name, got)
        assert got == w["map"]
    for x in res[1:]:                                                      # no triangulated norm near the threshold
        if x["X"] is not None:
            with np.errstate(all="ignore"):
                n = np.linalg.norm(x["X"][:3], axis=0)
            assert not (np.abs(n - 50.0) <= 50.0 * 1e-3).any(), (name, n[np.abs(n - 50.0) <= 0.05])


def test_moved_keypoints_clear_their_thresholds(O):
    """Off the line: OFF_LINE px, 5 past the E threshold.  Along the line, where the keypoint is meant to fail solvePnPRansac's 8 px
    and the filter's 1 px: at least 18 px."""
    assert TC.OFF_LINE - 1.0 >= 2.0
    for c in TC.cases().values():
        for (f, i), (kind, d) in c.moved.items():
            u = TC.line_direction(f, c.X[i])
            if kind == "off":
                assert abs(d @ u) < 1e-9 and abs(np.linalg.norm(d) - TC.OFF_LINE) < 1e-9
            else:
                assert abs(d[0] * u[1] - d[1] * u[0]) < 1e-6 * max(1.0, np.linalg.norm(d)), (c.name, f, i)
                if c.group == "eviction":
                    assert np.linalg.norm(d) >= 8.0 + 10.0


def test_max_point_norm_case_drops_and_goes_on(O):
    """Born after pair 0, where the norm test applies (initialize_map has none): five points 80 baselines away are dropped at every
    pair; five that look 120 baselines away at pair 1 and the one without parallax are dropped there, and every later pair stores a
    point for each of the six under its own featureid1, because their root (1, .) never gets one."""
    c = TC.cases()["max_point_norm"]
    res = run_of(O, c)
    far = [np.sort(np.linalg.norm(x["X"][:3], axis=0)[~(np.linalg.norm(x["X"][:3], axis=0) <= 50.0)]) for x in res[1:]]
    assert [len(f) for f in far] == [11, 5, 5, 5]
    assert np.all(np.abs(far[0][:5] - 80.0) < 0.5) and np.all(np.abs(far[0][5:10] - 120.0) < 0.5) and far[0][10] > 1e5
    for f in far[1:]:
        assert np.all(np.abs(f - 80.0) < 0.5)
    pts = [x["state"]["pt_feature"] for x in res]
    assert [len(p) for p in pts] == c.want["n_map"] == [30, 36, 42, 48, 54]
    for p in (2, 3, 4):
        new = pts[p][len(pts[p - 1]):]
        assert len(new) == 6 and all(f == p for f, _ in new)            # keyed by this pair's first frame: not a track root
        assert all(S.track_feature_back_in_time(res[p]["state"], fid)[0] == 1 for fid in new)


# ------------------------------------------------------------------ the cases discriminate
def walk(O, pin, K, opts, mutant=None):
    """slam_reference.run without bundle adjustment, re-typed with one switch per slip.  Returns per pair
    (status, n_corr, n_pts, pt_feature, points)."""
    o = dict(S.DEFAULTS); o.update(opts)
    s, ghost, out = S.empty_state(), {}, []
    for p, pr in enumerate(pin):
        f1, f2, n = pr["frame1"], pr["frame2"], len(pr["q"])
        col = (lambda i: int(pr["mi"][i]) % n) if mutant == "column_by_match_index" else (lambda i: i)
        if mutant == "links_for_outliers":
            for q, t in zip(pr["q_all"], pr["t_all"]):
                s["mapper"][(f2, int(t))] = (f1, int(q))
        S.update_feature_mapper(s, pr)
        if p == 0:
            S.initialize_map(s, dict(pr, X=pr["X"][:, [col(i) for i in range(n)]]))
            if o["ba_iterations"] > 0:
                S.optimize_map(s, K, o["ba_iterations"], o["huber_delta"])
            out.append((0, 0, len(s["points"]), list(s["pt_feature"]), np.array(s["points"])))
            continue
        mpd = {fid: i for i, fid in enumerate(s["pt_feature"])}
        obj, img = [], []
        for t, kp2 in zip(pr["t"], pr["p2"]):
            fid = S.track_feature_back_in_time(s, (f2, int(t)))
            if fid in mpd:
                obj.append(s["points"][mpd[fid]]); img.append(kp2)
            elif fid in ghost:
                obj.append(ghost[fid]); img.append(kp2)
        rc, rvec, tvec, _, _ = O.solve_pnp_ransac(np.array(obj).reshape(-1, 3), np.array(img).reshape(-1, 2), K) if len(obj) >= 4 else (-3, None, None, None, 0)
        if rc != 0:
            out.append((rc, len(obj), len(s["points"]), list(s["pt_feature"]), np.array(s["points"])))
            break
        T1 = s["cam_pose"][s["cam_frame"].index(f1)]
        T2 = np.hstack([O.rodrigues(rvec), tvec.reshape(3, 1)])
        s["cam_frame"].append(f2); s["cam_pose"].append(T2); s["cam_fixed"].append(False)
        X = O.triangulate(S._KP(K, T1), S._KP(K, T2), pr["p1"].T, pr["p2"].T)
        X = X / X[3]
        live = mutant == "live_map_later_wave_first"
        snapshot = {fid: i for i, fid in enumerate(s["pt_feature"])}
        c1, c2 = s["cam_frame"].index(f1), s["cam_frame"].index(f2)
        for i in (reversed(range(n)) if live else range(n)):
            x = X[:3, col(i)]
            if not np.linalg.norm(x) <= o["max_point_norm"]:
                continue
            fid = S.track_feature_back_in_time(s, (f2, int(pr["t"][i])))
            known = {f: j for j, f in enumerate(s["pt_feature"])} if live else snapshot
            if fid in known:
                S._observe(s, known[fid], c2, pr["p2"][i])
            elif fid in ghost:
                continue
            else:
                s["pt_feature"].append(fid if mutant == "keyed_by_root" else (f1, int(pr["q"][i]))); s["points"].append(np.array(x))
                S._observe(s, len(s["points"]) - 1, c1, pr["p1"][i]); S._observe(s, len(s["points"]) - 1, c2, pr["p2"][i])
        S.freeze_nonlast_cameras(s, o["free_cameras"])
        if o["ba_iterations"] > 0:
            S.optimize_map(s, K, o["ba_iterations"], o["huber_delta"])
        if o["filter_threshold"] > 0:
            S.remove_observations_above_threshold(O, s, K, o["filter_threshold"])
        before = dict(zip(s["pt_feature"], s["points"]))
        if S.limit_number_of_camera_in_map(s, o["max_cameras"]) is not None:
            if mutant == "zero_observation_points_removed":
                seen = set(s["obs_pt"])
                new = {pt: k for k, pt in enumerate(sorted(seen))}
                s["pt_feature"] = [v for i, v in enumerate(s["pt_feature"]) if i in seen]; s["points"] = [v for i, v in enumerate(s["points"]) if i in seen]
                s["obs_pt"] = [new[v] for v in s["obs_pt"]]
            if mutant == "in_map_kept_at_eviction":
                ghost.update({f: x for f, x in before.items() if f not in set(s["pt_feature"])})
        out.append((0, len(obj), len(s["points"]), list(s["pt_feature"]), np.array(s["points"])))
    return out


MUTANTS = ("keyed_by_root", "live_map_later_wave_first", "column_by_match_index", "in_map_kept_at_eviction",
           "zero_observation_points_removed", "links_for_outliers")
_WALKABLE = [c.name for c in TC.cases().values() if c.group != "failed_pair"]


def _differs(a, b):
    if len(a) != len(b):
        return True
    for x, y in zip(a, b):                                                 # the map as a dict: the order of the points does not count
        if x[:3] != y[:3] or sorted(x[3]) != sorted(y[3]) or len(set(x[3])) != len(x[3]) or len(set(y[3])) != len(y[3]):
            return True
        i, j = sorted(range(len(x[3])), key=x[3].__getitem__), sorted(range(len(y[3])), key=y[3].__getitem__)
        if not np.allclose(x[4][i], y[4][j], rtol=0, atol=1e-6, equal_nan=True):
            return True
    return False


@pytest.mark.parametrize("name", _WALKABLE)
def test_the_walk_with_no_slip_is_the_checker(O, name):
    c = TC.cases()[name]
    if c.match_mode != TC.MATCH_CROSSCHECK:
        r = chain_of(O, c)
        w = walk(O, TC.pair_inputs(O, c), TC.K, _opts(c))
        assert [x[1] for x in w] == r["n_corr"] and [x[2] for x in w] == r["n_map"]
        return
    res = run_of(O, c)
    w = walk(O, TC.pair_inputs(O, c), TC.K, _opts(c))
    assert len(w) == len(res)
    for x, y in zip(w, res):
        assert x[0] == y["status"] and x[1] == y["n_corr"] and x[3] == y["state"]["pt_feature"]
        assert np.array_equal(x[4], np.array(y["state"]["points"]).reshape(x[4].shape), equal_nan=True)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_slip_changes_some_cases_expected_output(O, mutant):
    caught = []
    for name in _WALKABLE:
        c = TC.cases()[name]
        if c.group == "rank" and c.want["E_inl"][0] > 65 and mutant != "column_by_match_index":
            continue                                                       # the large rank cases: only for what they are for
        pin = TC.pair_inputs(O, c)
        if _differs(walk(O, pin, TC.K, _opts(c)), walk(O, pin, TC.K, _opts(c), mutant)):
            caught.append(name)
    print(mutant, caught)
    assert caught, mutant
    expected = {"keyed_by_root": "max_point_norm", "live_map_later_wave_first": "many_to_one", "column_by_match_index": "rank_64",
                "in_map_kept_at_eviction": "eviction", "zero_observation_points_removed": "eviction_with_ba",
                "links_for_outliers": "tracks_cut_by_an_outlier"}
    assert expected[mutant] in caught

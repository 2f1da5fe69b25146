"""CPU: every case of tests/two_view_cases.py reaches what it is named for, from the oracle alone — the status, the number of
stacked models of the five-correspondence cases, the four candidates' counts and the winner of recoverPose, the inlier and
iteration counts, the intended match list.  tests/test_gpu_pairs_chosen.py runs the same cases through the batched tail on
the device; a case that drifts off its path fails here instead of passing for nothing there."""
import numpy as np
import pytest

import two_view_cases as T

NAMES = list(T.cases())
# what a group's cases must state, so that none is checked for less than it is there for
REQUIRED = {
    "few": {"status", "n_inl"}, "five_no_model": {"status", "models", "n_inl"}, "five_stacked": {"status", "models", "n_inl"},
    "five_one_model": {"status", "models", "n_inl", "counts", "best", "n_good"}, "many_no_model": {"status", "n_inl", "iters"},
}
POSED = {"status", "n_inl", "counts", "best", "n_good", "iters"}


def test_every_group_of_the_issue_is_there():
    groups = {c.group for c in T.cases().values()}
    assert groups == set(REQUIRED) | {"winner", "tie", "threshold", "block", "wave", "non_square"}
    assert sorted(c.M for c in T.group("few")) == [0, 1, 2, 3, 4]
    assert {c.want["best"] for c in T.group("winner") if c.K is T.K60} == {0, 1, 2, 3}
    assert sorted(c.M for c in T.group("block")) == [255, 256, 257, 511, 512, 512, 513, 513, T.BLOCK_KP_CAP]
    assert sorted(c.M for c in T.group("wave")) == [63, 64, 65]
    assert T.cases()["non_square"].K[1, 1] == 1.07 * T.cases()["non_square"].K[0, 0]
    assert T.cases()["ten_equal_points"].M == 10 and len(np.unique(T.cases()["ten_equal_points"].p1, axis=0)) == 1


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_is_named_for(oracle, name):
    assert not oracle.get_dk_early_exit()
    c = T.cases()[name]
    w = c.want
    assert set(w) >= REQUIRED.get(c.group, POSED), name
    assert c.p1.dtype == np.float32 and c.p2.dtype == np.float32
    e = T.expected(oracle, c)
    assert e["status"] == w["status"] and e["n_match"] == c.M and e["n_inl"] == w["n_inl"]
    assert int((e["mask"] > 0).sum()) == e["n_inl"]
    if "models" in w:
        assert c.M == 5 and len(e["models"]) == w["models"] and e["ransac_iters"] == 0
    if "iters" in w:
        assert e["ransac_iters"] == w["iters"]
    if c.group in ("winner", "tie", "threshold", "block", "non_square"):
        assert e["n_inl"] == c.M                             # scenes without noise or outliers: every point an inlier
    if w["status"] != T.VO_OK:
        assert "counts" not in w and e["n_good"] == 0
        return
    assert len(e["models"]) == 1
    assert list(e["counts"]) == w["counts"] and e["best"] == w["best"]
    n_good = w["n_good"] if isinstance(w["n_good"], dict) else {50.0: w["n_good"]}
    assert 50.0 in n_good
    for dist, want in n_good.items():
        e = T.expected(oracle, c, dist)
        good, best = e["counts"], e["best"]
        assert good[best] == want == e["n_good"], (name, dist, list(good))
        # the winner is the first candidate that no other exceeds
        assert best == int(np.argmax(good)) and all(good[best] >= g for g in good)
        ng, R, t, pm = oracle.recover_pose(e["E"], e["q1"], e["q2"], c.K, dist)
        assert ng == good[best] and np.array_equal(R, e["R"]) and np.array_equal(t, e["t"]) and np.array_equal(pm, e["pose_mask"])
        assert int((pm > 0).sum()) == ng and e["X"].shape == (4, e["n_inl"])
    if c.group == "threshold":
        assert sorted(n_good) == sorted(T.DIST_THRESHOLDS)
        assert not T.expected(oracle, c, 1.0)["counts"].any() and T.expected(oracle, c, 1.0)["best"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_slots_give_the_intended_match_list(oracle, name):
    c = T.cases()[name]
    for detector in ("orb", "sift") if c.K is T.K64 else ("orb",):
        rows1, xy1, rows2, xy2, qi, ti = T.slots(oracle, c, detector)
        assert rows1.shape == (c.M, 32 if detector == "orb" else 128) and rows1.dtype == np.uint8
        assert len(np.unique(rows1, axis=0)) == c.M
        assert np.array_equal(qi, np.arange(c.M)) and sorted(ti) == list(range(c.M))
        assert c.M < 2 or not np.array_equal(ti, qi)         # a gather by the query index would take other points
        assert np.array_equal(rows2[ti], rows1) and np.array_equal(xy2[ti], c.p2) and xy1 is c.p1
        if c.M >= 6 and c.group != "many_no_model":
            assert not np.array_equal(xy2[qi], c.p2)


def test_winner_and_tie_cases_cover_the_tie_order(oracle):
    """What `>=` against `>` in the first line of the tie order, a swap of good[c] and good[c + 2], or a missing negation of t
    would change: ties inside each pair of candidates (c, c + 2), and splits that move the winner across the pair."""
    seen = {(tuple(c.want["counts"]), c.want["best"]) for c in T.group("tie")}
    assert ((20, 0, 20, 0), 0) in seen and ((0, 20, 0, 20), 1) in seen
    assert ((19, 0, 21, 0), 2) in seen and ((21, 0, 19, 0), 0) in seen
    assert ((0, 19, 0, 21), 3) in seen and ((0, 21, 0, 19), 1) in seen
    for c in T.group("winner", "tie"):
        e = T.expected(oracle, c)
        assert abs(np.linalg.norm(e["t"]) - 1) < 1e-12 and abs(np.linalg.det(e["R"]) - 1) < 1e-12
        assert e["t"].any()                                                # a lost negation would show: t is not its own negative

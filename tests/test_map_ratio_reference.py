"""CPU: tests/map_ratio_reference.py — the statement vo_map_localize / vo_map_align are held to in map-match modes 1 and 2 on the GPU
(tests/test_gpu_map_ratio.py) — against a plain two-loop matcher that calls no oracle code, on every chosen case; and every case
against what it is there for, so that no GPU test can pass on empty lists."""
import numpy as np
import pytest

import map_align_reference as A
import map_ratio_reference as M
import relocalize_reference as RR

DETECTORS = ("sift", "orb")


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def _both(rows, map_rows, mode, **kw):
    got, want = M.match(rows, map_rows, mode, **kw), M.match_loops(rows, map_rows, mode, **kw)
    assert _same(got, want), (mode, kw)
    return got


def _rejected_by_the_rule(rows, map_rows):
    """Query rows the ratio rule alone turns away (mode 1 without a distance bound)."""
    return len(rows) - len(M.match(rows, map_rows, 1)[0]) if len(map_rows) >= 2 else 0


@pytest.mark.parametrize("detector", DETECTORS)
def test_the_oracle_composition_equals_the_plain_loops_on_every_size(oracle, detector):
    shared = differs = 0
    for npt in M.MAP_SIZES:
        m, pts, frames = M.call_frames(detector, npt)
        kept = {1: 0, 2: 0}; rejected = 0
        for n in M.FRAME_SIZES:
            rows = frames[n][0]
            if n == 300 and npt not in (3, 257):                           # (the loops are slow: the 300-row frames on two maps)
                lists = {mode: M.match(rows, m, mode) for mode in (1, 2)}
            else:
                lists = {mode: _both(rows, m, mode) for mode in (1, 2)}
            for mode, (qi, ti, d, d2) in lists.items():
                assert np.all(np.diff(qi) > 0) and len(qi) == len(ti) == len(d) == len(d2)
                assert d.dtype == d2.dtype == np.float32 and np.all(M.ratio_keeps(d, d2, M.RATIO)) and np.all(d <= d2)
                kept[mode] += len(qi)
            rejected += _rejected_by_the_rule(rows, m)
            shared += len(lists[1][1]) - len(set(lists[1][1].tolist()))
            assert len(set(lists[2][1].tolist())) == len(lists[2][1])      # the cross-check is one to one
            zero = RR.match_map(rows, m)
            differs += int(not _same(lists[2][:3], zero) and not _same(lists[2], lists[1]))
        if npt < 2:
            assert kept == {1: 0, 2: 0}                                     # the rule: a map of 0 or 1 rows gives no match
        else:
            assert kept[1] > 0 and kept[2] > 0 and rejected > 0, (detector, npt, kept, rejected)
    assert shared > 0 and differs > 0


@pytest.mark.parametrize("detector", DETECTORS)
def test_every_placement_is_what_its_name_says(oracle, detector):
    c = M.placement_case(detector)
    m, f = c["map_rows"], c["rows"]
    idx, dist = M.knn2(f, m)
    C = RR.CHUNK[detector]
    for i, name in enumerate(c["names"]):
        first, seconds, d1, d2 = M.PLACEMENTS[name]
        lo = min((first,) + seconds) if d1 == d2 else first
        assert idx[i, 0] == lo and dist[i, 0] == np.float32(d1) and dist[i, 1] == np.float32(d2), (name, idx[i], dist[i])
        T = RR.distance_table(f[i:i + 1], m)[0]
        assert sorted(np.flatnonzero(T <= np.float32(d2)).tolist()) == sorted((first,) + seconds), name      # nothing else is as near
        s = seconds[0]
        if name.startswith("tie for second"):                              # the tie is between the two seconds
            first, s, seconds = seconds[0], seconds[1], seconds[1:]
        if "one lane" in name:
            assert abs(first - s) == 16 and first // 128 == s // 128
        if "two lanes" in name:
            assert first // 16 == s // 16 and first != s
        if "two groups" in name:
            assert first // 16 != s // 16 and first % 16 != s % 16 and first // 128 == s // 128
        if "two chunks" in name:
            assert abs(first - s) >= 128 and first // 128 != s // 128
        if "256 apart" in name or "three chunks" in name or ("tie" in name and "two chunks" in name):
            assert abs(first - max(seconds)) >= 256 and first // C != max(seconds) // C
        if "before" in name:
            assert s < first
        if "after" in name:
            assert s > first
    for mode in (1, 2):
        qi, ti, d, d2 = _both(f, m, mode)
        kept = dict(zip(qi.tolist(), zip(ti.tolist(), d.tolist(), d2.tolist())))
        for i, name in enumerate(c["names"]):
            first, seconds, a, b = M.PLACEMENTS[name]
            if "tie for nearest" in name or name == "bound: 3 against 4":
                assert i not in kept, (mode, name)
            else:
                assert kept[i] == (first, float(a), float(b)), (mode, name)
    # mode 1: two query rows keep map row 32; the cross-check of mode 2 leaves it to the nearer one
    q1 = M.match(f, m, 1); q2 = M.match(f, m, 2)
    i, j, row = M.SHARED
    assert q1[1][q1[0] == i].tolist() == [row] and q1[1][q1[0] == j].tolist() == [row]
    assert q2[1][q2[0] == j].tolist() == [row] and i not in q2[0]
    assert len(q1[0]) == len(M.PLACEMENTS) - 3 + 1 and len(q2[0]) == len(q1[0]) - 1
    # a tie for nearest: kept only by a ratio above 1, with the lower index and n.distance == m.distance
    for ratio, there in ((1.0, False), (1.5, True)):
        qi, ti, d, d2 = _both(f, m, 1, ratio=ratio)
        for name in ("tie for nearest, one lane", "tie for nearest, two chunks"):
            i = c["names"].index(name)
            first, seconds, _, _ = M.PLACEMENTS[name]
            assert (i in qi) == there
            if there:
                assert ti[qi == i] == min(first, *seconds) and d[qi == i] == d2[qi == i] == 1
    # the distance bound and the ratio bound at once: 3.0 turns the (3, 5) row away and leaves the others
    k35, k34 = c["names"].index("bound: 3 against 5"), c["names"].index("bound: 3 against 4")
    for mode in (1, 2):
        free, bound = _both(f, m, mode), _both(f, m, mode, max_distance=3.0)
        assert k35 in free[0] and free[2][free[0] == k35] == 3 and k35 not in bound[0] and k34 not in free[0]
        assert set(free[0].tolist()) - set(bound[0].tolist()) == {k35} and len(bound[0]) > 10


@pytest.mark.parametrize("detector", DETECTORS)
def test_the_long_map(oracle, detector):
    c = M.long_map_case(detector)
    npt = len(c["map_rows"])
    assert npt == 65536
    far = 2 if detector == "sift" else 4                                   # four elements / bits moved
    for mode in (1, 2):
        qi, ti, d, d2 = M.match(c["rows"], c["map_rows"], mode)
        assert qi.tolist() == [0, 1] and ti.tolist() == [npt - 1, 0] and d.tolist() == [1, 1] and d2.tolist() == [far, far]
    assert _same(M.match(c["rows"][:3], c["map_rows"], 1), M.match_loops(c["rows"][:3], c["map_rows"], 1))
    T = RR.distance_table(c["rows"][:2], c["map_rows"])
    assert np.flatnonzero(T[0] <= far).tolist() == [0, npt - 1] and np.flatnonzero(T[1] <= far).tolist() == [0, npt - 1]


@pytest.mark.parametrize("detector", DETECTORS)
def test_the_pose_and_the_one_row_map(oracle, detector):
    c = RR.pose_case(detector)
    for mode in (1, 2):
        r = M.relocalize(c["map_pts"], c["map_rows"], c["xy"], c["rows"], M.K, mode)
        assert r["status"] == 0 and r["n_match"] == 200 and r["n_inl"] == 180 and not r["dist"].any() and r["dist2"].all()
        assert np.array_equal(r["mask"] > 0, ~c["wrong"])
        one = M.relocalize(c["map_pts"][:1], c["map_rows"][:1], c["xy"], c["rows"], M.K, mode)
        assert one["status"] == M.VO_ERR_TOO_FEW and one["n_match"] == 0
    assert RR.relocalize(c["map_pts"][:1], c["map_rows"][:1], c["xy"], c["rows"], M.K)["n_match"] == 1      # (mode 0 does match a map of one row)


@pytest.mark.parametrize("detector", DETECTORS)
def test_the_align_cases_have_rows_the_rule_rejects(oracle, detector):
    for npt in M.ALIGN_MAPS:
        m, mp, queries, distracted, big = M.align_call(detector, npt)
        for n in M.ALIGN_QUERIES:
            rows = queries[n][0]
            lists = {mode: _both(rows, m, mode) if n <= 65 else M.match(rows, m, mode) for mode in (1, 2)}
            if n != 257 or npt == 3:
                continue
            zero = RR.match_map(rows, m)
            assert len(distracted) >= 10 and len(m) == npt + len(distracted)
            assert all(i in zero[0] and i not in lists[1][0] and i not in lists[2][0] for i in distracted)
            assert 3 <= len(lists[2][0]) < len(zero[0]) and len(lists[1][0]) >= 3
            r = M.map_align(m, mp, rows, queries[n][1], big["max_error"], 1)
            assert r["status"] == 0 and r["n_inl"] >= 10 and r["nearest"] > A.PREMISE
            err = A.model_error((r["scale"], r["R"], r["t"]), big["model"])
            assert all(e <= A.MARGIN * ce for e, ce in zip(err, A.checker_error()))

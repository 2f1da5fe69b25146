"""CPU: tests/map_fuse_reference.py — the contract of vo_map_align_guided restated with numpy and as plain Python loops — held equal
to itself on every chosen case, and every case held to what it is named for, so that a case cannot silently stop testing its
branch; frontend.merge_maps against a loop restatement.  No device: tests/test_gpu_map_fuse.py holds the device to the same cases."""
import numpy as np
import pytest

import map_align_reference as A
import map_fuse_reference as F
import relocalize_reference as R

DETS = ("sift", "orb")


def _run(c):
    return [F.fuse_match(c["map_pts"], c["map_rows"], pts, rows, S, c["radius"], c["ratio"], c["max_distance"])
            for (rows, pts), S in zip(c["queries"], c["priors"])]


@pytest.fixture(scope="module", params=DETS)
def cases(request):
    det = request.param
    cs = F.all_cases(det)
    return det, cs, {name: _run(c) for name, c in cs.items()}


def test_the_two_restatements_agree_on_every_case(cases):
    det, cs, outs = cases
    for name, c in cs.items():
        for q, ((rows, pts), S) in enumerate(zip(c["queries"], c["priors"])):
            a = outs[name][q]
            b = F.fuse_match_loops(c["map_pts"], c["map_rows"], pts, rows, S, c["radius"], c["ratio"], c["max_distance"])
            assert a["n_seen"] == b["n_seen"] and a["n_match"] == b["n_match"], (det, name, q)
            assert np.array_equal(a["bi"], b["bi"]) and np.array_equal(a["ai"], b["ai"]), (det, name, q)
            assert a["dist"].dtype == np.float32 and a["dist"].tobytes() == b["dist"].tobytes() and a["dist2"].tobytes() == b["dist2"].tobytes(), (det, name, q)
            assert (np.diff(a["bi"]) > 0).all() and len(set(a["ai"].tolist())) == a["n_match"] <= min(len(rows), len(c["map_rows"]))


def test_every_case_is_what_it_is_named_for(cases):
    det, cs, outs = cases
    for name, c in cs.items():
        for q, e in enumerate(c["expect"]):
            o = outs[name][q]
            got = set(zip(o["bi"].tolist(), o["ai"].tolist()))
            for pair in e.get("pairs", ()):
                assert pair in got, (det, name, pair)
            assert not set(e.get("absent_a", ())) & set(o["ai"].tolist()), (det, name)
            assert not set(e.get("absent_b", ())) & set(o["bi"].tolist()), (det, name)
            for key in ("n_match", "n_seen"):
                assert key not in e or o[key] == e[key], (det, name, key, o[key])
            for i, d2 in e.get("seconds", {}).items():
                assert o["dist2"][o["bi"].tolist().index(i)] == d2, (det, name, i)


def test_sizes_cover_the_tiles_and_the_seams(cases):
    det, cs, outs = cases
    assert set(F.MAP_SIZES) == {0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 513}
    assert {n for s in F.QUERY_SIZES for n in s} == {0, 1, 3, 65, 256, 257} and all(len(set(s)) == 3 for s in F.QUERY_SIZES)
    for npt in F.MAP_SIZES:
        c, o = cs[f"sizes npt={npt}"], outs[f"sizes npt={npt}"]
        assert len(c["map_rows"]) == npt and len({S.tobytes() for S in c["priors"]}) == 3
        assert [len(r) for r, _ in c["queries"]] == list(F.QUERY_SIZES[0] if npt % 2 else F.QUERY_SIZES[1])
    c, o = cs["sizes npt=513"], outs["sizes npt=513"]
    assert o[1]["n_match"] == 0 == o[1]["n_seen"]                          # the empty query map
    assert 4 <= o[0]["n_match"] < o[0]["n_seen"] < 257                     # several query points per staged point: the uniqueness step decides
    assert (o[0]["dist2"] != F.FLT_MAX).any() and (o[0]["dist2"] == F.FLT_MAX).any()     # spheres of one and of several candidates
    assert np.array_equal(c["map_rows"][5], c["map_rows"][5 + F.TILE])
    rows, pts = c["queries"][0]
    assert np.array_equal(rows[10], rows[11]) and np.array_equal(pts[10], pts[11])
    f = outs["sizes ratio and bound"]; p = F.fuse_match(*[cs["sizes ratio and bound"][k] for k in ("map_pts", "map_rows")],
                                                        cs["sizes ratio and bound"]["queries"][0][1], cs["sizes ratio and bound"]["queries"][0][0],
                                                        cs["sizes ratio and bound"]["priors"][0], 0.4)
    assert 4 <= f[0]["n_match"] < p["n_match"]                             # the filters bite and leave something


def test_exact_geometry_decides_on_the_sphere(cases):
    det, cs, outs = cases
    below = float(np.nextafter(5.0, 0.0))
    c = cs["sphere r=5.0"]
    rows, b = c["queries"][0]
    take, y = F.transform(c["priors"][0], b)
    assert take.tolist() == [True] * 6 + [False, False]
    assert np.array_equal(y[:6], b[:6])                                    # the identity moves nothing, exactly
    off = b[:4] - c["map_pts"][:4]
    assert off.tolist() == [[3, 4, 0], [0, 0, 5], [2, 3, 6], [0, 0, 0]]
    assert (off[:2] ** 2).sum(axis=1).tolist() == [25.0, 25.0] and (off[2] ** 2).sum() == 49.0 and below * below < 25.0
    assert not np.isfinite(c["map_pts"][4:6]).all(axis=1).any()            # staged points that can never be candidates
    n = {name: outs[name][0]["n_match"] for name in cs if name.startswith("sphere")}
    assert n == {"sphere r=5.0": 3, f"sphere r={below!r}": 1, "sphere r=7.0": 4, "sphere r=0.0": 1}
    o = cs["overflow"]
    take, y = F.transform(o["priors"][0], o["queries"][0][1])
    assert np.isfinite(o["priors"][0]).all() and not take.any() and F.transform(o["priors"][1], o["queries"][1][1])[0].all()


def _cell(x, x0, extent):
    return int(min(max(np.floor((x - x0) * (F.GRID / extent)), 0), F.GRID - 1))


def test_grid_cases_meet_the_grid_where_they_say(cases):
    det, cs, outs = cases
    c = cs["grid r=10.0"]
    a = c["map_pts"]; rows, b = c["queries"][0]
    assert a.min(axis=0).tolist() == [0, 0, 0] and a.max(axis=0).tolist() == [F.GRID_BOX] * 3
    edge = F.GRID_BOX / F.GRID
    assert edge == 10.0 and {0.5, edge, 3.5 * edge} <= {cs[n]["radius"] for n in cs if n.startswith("grid")}
    assert cs["grid r=9000.0"]["radius"] > np.linalg.norm(b[10] - a[0]) > np.sqrt(3) * F.GRID_BOX      # larger than the box, and reaches it from the far point
    assert all((v / edge).is_integer() for v in b[3]) and np.array_equal(b[3], a[3])                     # a y exactly on a cell corner
    assert b[10].tolist() == [5000.0] * 3
    cell = lambda p: tuple(_cell(float(v), 0.0, F.GRID_BOX) for v in p)
    assert cell(a[5]) == cell(a[6]) and np.array_equal(c["map_rows"][5], c["map_rows"][6])               # one row twice in one cell
    assert cell(a[7])[0] == cell(a[8])[0] + 1 and cell(a[7])[1:] == cell(a[8])[1:] and np.array_equal(c["map_rows"][7], c["map_rows"][8])
    o = outs["grid r=10.0"][0]
    at = {k: i for i, k in enumerate(o["bi"].tolist())}
    assert o["dist"][at[5]] == o["dist2"][at[5]] and o["dist"][at[6]] == o["dist2"][at[6]]             # the ties really tie
    assert 7 // F.TILE == 8 // F.TILE and 9 // F.TILE != (9 + F.TILE) // F.TILE                          # equal claims in one tile, and a tile apart
    assert np.array_equal(rows[7], rows[8]) and np.array_equal(rows[9], rows[9 + F.TILE])
    for i, k, j in ((7, 8, 9), (9, 9 + F.TILE, 10)):
        assert F.int_distances(c["map_rows"][j:j + 1], rows[i]) == F.int_distances(c["map_rows"][j:j + 1], rows[k])
        assert ((b[i] - a[j]) ** 2).sum() == ((b[k] - a[j]) ** 2).sum() == 0.25
    far = outs["grid r=9000.0"][0]
    assert far["n_seen"] == len(rows) and outs["grid r=0.5"][0]["n_seen"] < outs["grid r=35.0"][0]["n_seen"] < far["n_seen"]
    assert (cs["far outside"]["queries"][0][1] > 4000).all()
    for kind, flat_axes in (("point", 3), ("line", 2), ("plane", 1)):
        p = cs[f"flat {kind}"]["map_pts"]
        assert int((p.max(axis=0) == p.min(axis=0)).sum()) == flat_axes


def test_the_filters_sit_on_their_bounds(cases):
    det, cs, outs = cases
    sift = det == "sift"
    c = cs["filter max_distance"]
    free = F.fuse_match(c["map_pts"], c["map_rows"], c["queries"][0][1], c["queries"][0][0], F.IDENTITY, c["radius"])
    assert free["dist"].tolist() == [c["max_distance"], float(np.sqrt(np.float32(3))) if sift else 3.0]   # EQUAL to the bound, and below it
    c = cs["filter ratio_eq"]
    free = F.fuse_match(c["map_pts"], c["map_rows"], c["queries"][0][1], c["queries"][0][0], F.IDENTITY, c["radius"])
    assert float(free["dist"][0]) == c["ratio"] * float(free["dist2"][0]) and float(free["dist"][1]) < c["ratio"] * float(free["dist2"][1])
    c = cs["filter ratio"]
    free = F.fuse_match(c["map_pts"], c["map_rows"], c["queries"][0][1], c["queries"][0][0], F.IDENTITY, c["radius"])
    # without the rule the nearer row 2 takes staged 4 and the farther row 3 loses it; with it row 2 fails and blocks nobody
    assert (2, 4) in set(zip(free["bi"].tolist(), free["ai"].tolist())) and 3 not in free["bi"].tolist()
    assert (3, 4) in set(zip(outs["filter ratio"][0]["bi"].tolist(), outs["filter ratio"][0]["ai"].tolist()))


def test_the_known_similarity_case(cases):
    det, cs, outs = cases
    c, o = cs["known similarity"], outs["known similarity"][0]
    rows, b = c["queries"][0]
    _, y = F.transform(c["priors"][0], b)
    shift = np.linalg.norm(y[c["dup"]] - c["map_pts"][150 + c["dup"]], axis=1)
    print(det, "prior's shift over the true duplicates: max", shift.max(), "against a radius of", c["radius"])
    assert 0.01 < shift.max() < c["radius"] / 2                            # every true duplicate lies in its sphere ...
    got = dict(zip(o["bi"].tolist(), o["ai"].tolist()))
    assert all(got.get(int(i)) == int(150 + i) for i in c["dup"])          # ... and wins it
    assert o["n_match"] == len(c["dup"]) or set(got) >= set(c["dup"].tolist())
    # the look-alikes really defeat the descriptor-only cross-check: it pairs them with the staged point that carries their row
    bi, ai, d = R.match_map(rows, c["map_rows"])
    cross = dict(zip(bi.tolist(), ai.tolist()))
    assert all(cross.get(i) == i for i in range(F.KNOWN_ALIKE))
    assert all(np.linalg.norm(y[i] - c["map_pts"][i]) > 2 * c["radius"] for i in range(F.KNOWN_ALIKE))
    right_cross = sum(cross.get(int(i)) == int(150 + i) for i in c["dup"])
    assert right_cross <= len(c["dup"]) - F.KNOWN_ALIKE < len(c["dup"]) == sum(got.get(int(i)) == int(150 + i) for i in c["dup"])
    # the refit from the guided lists recovers the generating similarity within the checker's own bound, from more inliers
    g = F.map_align_guided(c["map_rows"], c["map_pts"], rows, b, c["priors"][0], c["radius"], c["max_error"])
    first = A.map_align(c["map_rows"], c["map_pts"], rows, b, c["max_error"])
    print(det, "inliers: descriptor-only", first["n_inl"], "guided", g["n_inl"])
    assert g["status"] == 0 and first["status"] == 0 and g["n_inl"] > first["n_inl"] and g["n_inl"] >= len(c["dup"]) - 5
    err = A.model_error((g["scale"], g["R"], g["t"]), c["truth"])
    print(det, "guided refit against the generating similarity", err)
    assert err[0] < 2e-3 and err[1] < 2e-3 and err[2] < 2e-2             # noise of 0.004 per axis over 150 points in a 16-unit patch


def test_merge_maps_against_the_loop_restatement(cases):
    from visual_odometry_amd.frontend import merge_maps
    det, cs, outs = cases
    c, o = cs["known similarity"], outs["known similarity"][0]
    rows, b = c["queries"][0]
    rng = np.random.default_rng(3)
    mask = (rng.uniform(size=o["n_match"]) < 0.8).astype(np.uint8)
    s, Rm, t = c["truth"]
    got = merge_maps(c["map_rows"], c["map_pts"], rows, b, s, Rm, t, o["ai"], o["bi"], mask)
    want = F.merge_maps_loops(c["map_rows"], c["map_pts"], rows, b, s, Rm, t, o["ai"], o["bi"], mask)
    assert got["n_fused"] == want["n_fused"] == int(mask.sum()) > 0
    for k in ("rows", "points", "index_b"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    na, nb, n = len(c["map_rows"]), len(rows), len(got["rows"])
    assert n == na + nb - got["n_fused"] == len(got["points"])
    assert np.array_equal(got["rows"][:na], c["map_rows"]) and got["points"][:na].tobytes() == np.ascontiguousarray(c["map_pts"]).tobytes()
    fused = np.zeros(nb, bool); fused[o["bi"][mask != 0]] = True
    ib = got["index_b"]
    assert (ib[fused] < na).all() and np.array_equal(ib[o["bi"][mask != 0]], o["ai"][mask != 0])         # fused rows point into A
    assert np.array_equal(ib[~fused], na + np.arange(nb - got["n_fused"]))                                 # a bijection onto the rest, in B's order
    assert np.array_equal(got["rows"][ib[~fused]], rows[~fused])
    assert np.abs(got["points"][ib[~fused]] - A.transform(c["truth"], b[~fused])).max() < 1e-12
    # nothing matched: the maps are concatenated; an empty B: A comes back
    none = merge_maps(c["map_rows"], c["map_pts"], rows, b, s, Rm, t, [], [], [])
    assert none["n_fused"] == 0 and len(none["rows"]) == na + nb and np.array_equal(none["index_b"], na + np.arange(nb))
    empty = merge_maps(c["map_rows"], c["map_pts"], rows[:0], b[:0], s, Rm, t, [], [], [])
    assert len(empty["rows"]) == na and len(empty["index_b"]) == 0
    with pytest.raises(ValueError):
        merge_maps(c["map_rows"], c["map_pts"], rows, b, s, Rm, t, [0, 0], [1, 2], [1, 1])                # one staged row in two inlier matches
    with pytest.raises(ValueError):
        merge_maps(c["map_rows"], c["map_pts"], rows, b, s, Rm, t, [na], [0], [1])

"""CPU: tests/guided_reference.py — the contract of vo_map_localize_guided restated with numpy and as plain Python loops — held equal
to itself on every chosen case, and every case held to what it is named for, so that a case cannot silently stop testing its
branch.  No device and no oracle call: tests/test_gpu_relocalize_guided.py holds the device to the same cases."""
import numpy as np
import pytest

import guided_reference as G

DETS = ("sift", "orb")


@pytest.fixture(scope="module", params=DETS)
def cases(request):
    det = request.param
    cs = G.all_cases(det)
    outs = {name: [G.guided_match(c["map_pts"], c["map_rows"], xy, rows, c["K"], P, c["radius"], c["ratio"], c["max_distance"])
                   for (rows, xy), P in zip(c["frames"], c["priors"])] for name, c in cs.items()}
    return det, cs, outs


def test_the_two_restatements_agree_on_every_case(cases):
    det, cs, outs = cases
    for name, c in cs.items():
        for q, ((rows, xy), P) in enumerate(zip(c["frames"], c["priors"])):
            a = outs[name][q]
            b = G.guided_match_loops(c["map_pts"], c["map_rows"], xy, rows, c["K"], P, c["radius"], c["ratio"], c["max_distance"])
            assert a["n_seen"] == b["n_seen"] and a["n_match"] == b["n_match"], (det, name, q)
            assert np.array_equal(a["qi"], b["qi"]) and np.array_equal(a["ti"], b["ti"]), (det, name, q)
            assert a["dist"].dtype == np.float32 and a["dist"].tobytes() == b["dist"].tobytes() and a["dist2"].tobytes() == b["dist2"].tobytes(), (det, name, q)
            assert (np.diff(a["qi"]) > 0).all() and a["n_match"] <= len(rows)


def test_every_case_is_what_it_is_named_for(cases):
    det, cs, outs = cases
    for name, c in cs.items():
        for q, e in enumerate(c["expect"]):
            o = outs[name][q]
            got = set(zip(o["qi"].tolist(), o["ti"].tolist()))
            for pair in e.get("pairs", ()):
                assert pair in got, (det, name, pair)
            assert not set(e.get("absent_pts", ())) & set(o["ti"].tolist()), (det, name)
            assert not set(e.get("absent_kps", ())) & set(o["qi"].tolist()), (det, name)
            for key in ("n_match", "n_seen"):
                assert key not in e or o[key] == e[key], (det, name, key, o[key])
            for kp, d2 in e.get("seconds", {}).items():
                assert o["dist2"][o["qi"].tolist().index(kp)] == d2, (det, name, kp)


def test_sizes_cover_the_tile_and_the_frames(cases):
    det, cs, outs = cases
    assert {G.TILE - 1, G.TILE, G.TILE + 1, 2 * G.TILE + 1, 0, 1, 3, 4, 5, 63, 64, 65} <= set(G.MAP_SIZES)
    assert [len(f[0]) for f in cs["sizes frames 1 and kp_cap"]["frames"]] == [1, 512, 300]
    for npt in G.MAP_SIZES:
        c, o = cs[f"sizes npt={npt}"], outs[f"sizes npt={npt}"]
        assert [len(f[0]) for f in c["frames"]] == [300, 17, 0] and len(c["map_rows"]) == npt
        assert len({P.tobytes() for P in c["priors"]}) == 3 and o[2]["n_match"] == 0 and o[2]["n_seen"] == 0
        take, _, _ = G.project(c["priors"][0], c["map_pts"], c["K"])
        if npt >= 63:
            assert 0 < take.sum() < npt                                    # points before and behind the camera
            assert 4 <= o[0]["n_match"] <= o[0]["n_seen"]
            assert npt < G.TILE - 1 or o[0]["n_match"] < o[0]["n_seen"]    # several points per keypoint: the uniqueness step decides
            assert (o[0]["dist2"] != G.FLT_MAX).any() and (o[0]["dist2"] == G.FLT_MAX).any()      # windows of one and of several candidates
            assert (o[0]["dist2"] == o[0]["dist"]).any()                   # the duplicated keypoints 10, 11: a tie counts as a second
        if npt > 5 + G.TILE:
            assert np.array_equal(c["map_rows"][5], c["map_rows"][5 + G.TILE])
    f = outs["sizes ratio and bound"]; p = outs["sizes npt=257"]
    assert 4 <= f[0]["n_match"] < p[0]["n_match"]                          # the filters bite and leave something


def test_exact_geometry_decides_on_the_circle(cases):
    det, cs, outs = cases
    below = float(np.nextafter(5.0, 0.0))
    c = cs["exact r=5.0"]
    take, u, v = G.project(c["priors"][0], c["map_pts"], c["K"])
    assert take.tolist() == [True, True, True, False, False, False, True]
    assert all(float(x).is_integer() for x in np.concatenate([u[:3], v[:3]])) and not np.isfinite(u[6]) and not np.isfinite(v[6])
    xy = c["frames"][0][1].astype(np.float64)
    assert ((xy[0] - (u[0], v[0])) ** 2).sum() == 25.0 == ((xy[2] - (u[2], v[2])) ** 2).sum() and below * below < 25.0
    assert (xy[4] == (192, 192)).all()                                     # where point 4 would land with the sign of Z ignored
    assert outs["exact r=5.0"][0]["n_match"] == 3 and outs[f"exact r={below!r}"][0]["n_match"] == 1 == outs["exact r=0.0"][0]["n_match"]


def test_grid_cases_meet_the_grid_where_they_say(cases):
    det, cs, outs = cases
    c = cs["grid r=10.0"]
    rows, xy = c["frames"][0]
    x0, y0, edge = G.grid_of(xy)
    assert (x0, y0, edge) == (-160.0, -120.0, 10.0)
    assert {0.5, edge, 3.5 * edge} <= {cs[n]["radius"] for n in cs if n.startswith("grid")}
    assert cs["grid r=7100.0"]["radius"] > np.hypot(640, 640)              # larger than the whole keypoint box
    _, u, v = G.project(c["priors"][0], c["map_pts"], c["K"])
    assert ((u[1] - x0) / edge).is_integer() and ((v[1] - y0) / edge).is_integer()       # a projection exactly on a cell boundary
    assert (u[2], v[2]) == (5000.0, 5000.0)                                # far outside the box
    assert (xy[4] < 0).all() and (xy[5] > 64).all() and (xy[0] < 0).all()  # negative, and beyond any configured width and height
    cell = lambda i: (G.cell_of(float(xy[i][0]), x0, edge), G.cell_of(float(xy[i][1]), y0, edge))
    assert cell(6) == cell(7) and np.array_equal(rows[6], rows[7])         # one row twice in one cell
    assert cell(8)[0] == cell(9)[0] + 1 and np.array_equal(rows[8], rows[9])   # ... and in two cells: the lower keypoint in the later one
    o = outs["grid r=10.0"][0]
    at = {k: i for i, k in enumerate(o["qi"].tolist())}
    assert o["dist"][at[6]] == o["dist2"][at[6]] and o["dist"][at[8]] == o["dist2"][at[8]]
    assert 7 // G.TILE == 8 // G.TILE and 9 // G.TILE != (9 + G.TILE) // G.TILE          # equal claims in one tile, and a tile apart
    assert np.array_equal(c["map_rows"][7], c["map_rows"][8]) and np.array_equal(c["map_rows"][9], c["map_rows"][9 + G.TILE])
    far = outs["grid r=7100.0"][0]
    assert far["n_seen"] == len(c["map_rows"]) and outs["grid r=0.5"][0]["n_seen"] < outs["grid r=35.0"][0]["n_seen"] < far["n_seen"]


def test_the_known_pose_case_keeps_every_true_keypoint_in_its_window(cases):
    det, cs, outs = cases
    c, o = cs["known pose"], outs["known pose"][0]
    t = c["truth"]
    _, u, v = G.project(c["priors"][0], c["map_pts"], c["K"])
    xy = c["frames"][0][1].astype(np.float64)
    shift = np.hypot(xy[:, 0] - u[t["perm"]], xy[:, 1] - v[t["perm"]])[~t["wrong"]]
    print(det, "prior's reprojection shift over the true keypoints: max", shift.max(), "px against a radius of", c["radius"])
    assert 0.5 < shift.max() < c["radius"] / 2
    got = dict(zip(o["qi"].tolist(), zip(o["ti"].tolist(), o["dist"].tolist())))
    for i in np.flatnonzero(~t["wrong"]):
        assert got[int(i)] == (int(t["perm"][i]), 0.0)                     # the true keypoint lies in the window and wins it
    assert o["n_match"] >= 180

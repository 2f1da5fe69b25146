"""GPU: guided relocalisation — k_guided_grid, k_guided_match, k_guided_select and, unchanged, k_pnp_ransac behind
vo_map_localize_guided — on rows and positions the test CHOSE (FrontEnd.set_sift_rows / set_orb_rows with xy for the frames,
FrontEnd.stage_map for the map: no image anywhere), against tests/guided_reference.py, which tests/test_guided_reference.py holds
equal on the CPU to a plain-loop restatement and to what every case is named for.  Both detectors.

Held here:
  lists     keypoint, point, float32 distance, float32 SECOND distance, order and n_seen EQUAL the reference: maps of 0, 1, 3, 4, 5,
            63, 64, 65, 255, 256, 257, 513 points (around one tile of k_guided_match and one past two), frames of 0, 1, 17, 300 and
            kp_cap keypoints, three queries with different slots and priors per call; exact geometry on the circle; points that
            must not take part (Z = 0, Z < 0, NaN, c_2 = 5e-324); windows of half a pixel, one cell, 3.5 cells and more than the
            whole box, a projection on a cell corner and one far outside, keypoints at negative coordinates and beyond the
            configured size; ties between keypoints (one cell, two cells) and between points (one tile, a tile apart); both filters;
  pose      poses, n_inl, status and inlier masks BYTE-EQUAL to vo_solve_pnp_ransac_batch on the reference's arrays, in every call;
            the known pose recovered within tests/test_gpu_relocalize.py's bound from a perturbed prior;
  refinement  prior=None returns the bytes of the call given the preceding relocalize's poses; a failed query keeps its status;
            the refusals; relocalize(refine_radius=) is that pass;
  others    relocalize returns the same bytes after a guided call; map_matches / map_match_seconds serve the latest call;
  arguments every refusal, with the outputs untouched.
The whole file takes 1.3 s on an MI355X (measured, one run, the reference's side included); the slowest test 0.03 s."""
import ctypes as C

import numpy as np
import pytest

import guided_reference as G
import relocalize_reference as R

pytestmark = pytest.mark.gpu

GEN_TOL_R, GEN_TOL_T = 0.02, 0.1   # tests/test_gpu_relocalize.py: recovering a generating pose


@pytest.fixture(scope="module", params=("sift", "orb"))
def rig(request):
    from visual_odometry_amd.frontend import FrontEnd
    det = request.param
    if det == "sift":
        fe = FrontEnd(32, 32, max_frames=5, max_pairs=3, detector="sift", kp_cap=512)
    else:
        fe = FrontEnd(64, 64, max_frames=5, max_pairs=3, nfeatures=304, nlevels=1)
    assert fe.kp_cap >= 300
    yield det, fe
    fe.ctx.close()


def _put(fe, det, slot, rows, xy):
    (fe.set_sift_rows if det == "sift" else fe.set_orb_rows)(slot, rows, xy)


def _check(fe, c, out, slots, what, frames=None, priors=None, **pnp):
    """A guided call's output against the reference (lists, seconds, n_seen exactly) and the pose part byte for byte against
    vo_solve_pnp_ransac_batch on the reference's arrays.  Returns the references."""
    from visual_odometry_amd import geometry
    frames = c["frames"] if frames is None else frames
    priors = c["priors"] if priors is None else priors
    refs = [G.guided_match(c["map_pts"], c["map_rows"], xy, rows, c["K"], P, c["radius"], c["ratio"], c["max_distance"])
            for (rows, xy), P in zip(frames, priors)]
    got = [fe.map_matches(q) for q in range(len(slots))]
    for q, (r, (pi, ki, d, mask)) in enumerate(zip(refs, got)):
        d2 = fe.map_match_seconds(q)
        print(what, "q", q, "n_match", int(out["n_match"][q]), "ref", r["n_match"], "n_seen", int(out["n_seen"][q]), "ref", r["n_seen"],
              "status", int(out["status"][q]), "n_inl", int(out["n_inl"][q]))
        assert out["n_match"][q] == r["n_match"] == len(pi) and out["n_seen"][q] == r["n_seen"], (what, q)
        assert np.array_equal(ki, r["qi"]) and np.array_equal(pi, r["ti"]), (what, q)
        assert d.dtype == np.float32 and d.tobytes() == r["dist"].tobytes() and d2.tobytes() == r["dist2"].tobytes(), (what, q)
    off = np.concatenate([[0], np.cumsum([r["n_match"] for r in refs])]).astype(np.int32)
    obj = np.concatenate([r["obj"] for r in refs]); img = np.concatenate([r["img"] for r in refs])
    st, rvec, tvec, bmask, ninl = geometry.solve_pnp_ransac_batch(obj, img, off, c["K"], ctx=fe.ctx, **{
        {"iterations": "iterationsCount", "reproj_err": "reprojectionError"}.get(k, k): v for k, v in pnp.items() if k != "min_inliers"})
    for q in range(len(slots)):
        want_st = R.VO_ERR_NO_MODEL if st[q] == 0 and ninl[q] < pnp.get("min_inliers", 0) else st[q]
        pose = np.zeros((3, 4))
        if want_st == 0:
            pose = np.hstack([geometry.Rodrigues(rvec[q], ctx=fe.ctx)[0], tvec[q].reshape(3, 1)])
        assert out["status"][q] == want_st and out["n_inl"][q] == ninl[q], (what, q)
        assert out["poses"][q].tobytes() == pose.tobytes(), (what, q)
        assert got[q][3].tobytes() == bmask[off[q]:off[q + 1]].tobytes(), (what, q)
    return refs


def _run(fe, det, c, slots, what, **pnp):
    """Stage the case (frames into `slots`, the map) and run it with its own priors."""
    for s, (rows, xy) in zip(slots, c["frames"]):
        _put(fe, det, s, rows, xy)
    fe.stage_map(c["map_rows"], c["map_pts"])
    out = fe.relocalize_guided(slots, c["K"], np.stack(c["priors"]), c["radius"], c["ratio"], c["max_distance"], **pnp)
    return out, _check(fe, c, out, slots, f"{what} {det}", **pnp)


# ------------------------------------------------------------------ lists
@pytest.mark.parametrize("npt", G.MAP_SIZES)
def test_lists_equal_the_reference(rig, npt):
    det, fe = rig
    c = G.size_case(det, npt)
    a, _ = _run(fe, det, c, [0, 1, 3], f"npt {npt}")
    # the same queries in another order and other slots' positions; two calls on the same input return the same bytes
    order = [2, 0, 1]
    sl = [[0, 1, 3][k] for k in order]
    b = fe.relocalize_guided(sl, c["K"], np.stack([c["priors"][k] for k in order]), c["radius"])
    _check(fe, c, b, sl, f"npt {npt} reordered {det}", frames=[c["frames"][k] for k in order], priors=[c["priors"][k] for k in order])
    assert all(b[k][order.index(0)].tobytes() == a[k][0].tobytes() for k in a)
    again = fe.relocalize_guided(sl, c["K"], np.stack([c["priors"][k] for k in order]), c["radius"])
    assert all(again[k].tobytes() == b[k].tobytes() for k in b)


def test_frames_of_one_keypoint_and_of_kp_cap(rig):
    det, fe = rig
    c = G.size_case(det, 257, sizes=(1, fe.kp_cap, 300))
    out, refs = _run(fe, det, c, [4, 2, 0], "kp_cap")
    assert refs[1]["n_match"] > refs[2]["n_match"] > 4


def test_both_filters_on_a_full_call(rig):
    det, fe = rig
    c = G.size_case(det, 257, sizes=(300, 17, 300), ratio=0.9, max_distance=3.5 if det == "sift" else 12.0)
    _run(fe, det, c, [0, 1, 2], "filters", min_inliers=5)


@pytest.mark.parametrize("name", sorted(G.named_cases("orb")))
def test_named_cases(rig, name):
    det, fe = rig
    c = G.named_cases(det)[name]
    out, refs = _run(fe, det, c, [2], name)
    e = c["expect"][0]
    got = set(zip(refs[0]["qi"].tolist(), refs[0]["ti"].tolist()))
    assert all(p in got for p in e.get("pairs", ()))                       # (the CPU file holds the reference to the rest)
    if name == "known pose":
        t = c["truth"]
        assert out["status"][0] == 0 and out["n_inl"][0] >= 180
        err_R, err_t = np.abs(out["poses"][0][:, :3] - t["R"]).max(), np.abs(out["poses"][0][:, 3] - t["t"]).max()
        print(det, "error against the generating pose: R", err_R, "t", err_t)
        assert err_R < GEN_TOL_R and err_t < GEN_TOL_T


def test_the_host_array_convenience_is_the_same_operator():
    from visual_odometry_amd import _lib, geometry
    ctx = _lib.Context(0)
    try:
        for det in ("sift", "orb"):
            c = G.pose_case(det)
            rows, xy = c["frames"][0]
            got = geometry.relocalize_guided(c["map_pts"], c["map_rows"], xy, rows.astype(np.float32) if det == "sift" else rows, c["K"],
                                             c["priors"][0], c["radius"], ctx=ctx)
            r = G.guided_match(c["map_pts"], c["map_rows"], xy, rows, c["K"], c["priors"][0], c["radius"])
            pi, ki, d, mask = got["matches"]
            assert got["status"] == 0 and got["n_match"] == r["n_match"] and got["n_seen"] == r["n_seen"]
            assert np.array_equal(pi, r["ti"]) and np.array_equal(ki, r["qi"]) and np.array_equal(d, r["dist"]) and np.array_equal(got["seconds"], r["dist2"])
            assert np.abs(got["pose"][:, :3] - c["truth"]["R"]).max() < GEN_TOL_R and np.abs(got["pose"][:, 3] - c["truth"]["t"]).max() < GEN_TOL_T
    finally:
        ctx.close()


# ------------------------------------------------------------------ the refinement pass
def _same(a, b, keys=("poses", "n_match", "n_inl", "status", "n_seen")):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def test_the_refinement_pass_starts_from_the_poses_on_the_device(rig):
    from visual_odometry_amd import _lib
    det, fe = rig
    s = R.status_case(det)
    for slot, (rows, xy) in enumerate(s["frames"]):
        _put(fe, det, slot, rows, xy)
    fe.stage_map(s["map_rows"], s["map_pts"])
    with pytest.raises(_lib.VoError):
        fe.relocalize_guided([0, 1, 2], R.K, None, 8.0)                    # no earlier call on this map
    first = fe.relocalize([0, 1, 2], R.K)
    assert first["status"].tolist() == [R.VO_ERR_TOO_FEW, R.VO_ERR_NO_MODEL, R.VO_OK]
    with pytest.raises(_lib.VoError):
        fe.relocalize_guided([0, 2, 1], R.K, None, 8.0)                    # other slots
    with pytest.raises(_lib.VoError):
        fe.relocalize_guided([0, 1], R.K, None, 8.0)                       # another Q
    a = fe.relocalize_guided([0, 1, 2], R.K, None, 8.0)
    lists_a = [fe.map_matches(q) for q in range(3)]
    # a query that failed the first pass keeps its status, with zero counts and a zero pose
    assert a["status"].tolist() == [R.VO_ERR_TOO_FEW, R.VO_ERR_NO_MODEL, R.VO_OK]
    assert not a["poses"][:2].any() and not a["n_match"][:2].any() and not a["n_inl"][:2].any() and not a["n_seen"][:2].any()
    assert len(lists_a[0][0]) == 0 and len(lists_a[1][0]) == 0
    with pytest.raises(_lib.VoError):
        fe.relocalize_guided([0, 1, 2], R.K, None, 8.0)                    # the guided call has overwritten those poses
    # ... and the solved one is the call given the first pass's pose
    again = fe.relocalize([0, 1, 2], R.K)
    assert all(again[k].tobytes() == first[k].tobytes() for k in first)
    b = fe.relocalize_guided([2], R.K, first["poses"][2:3], 8.0)
    assert all(a[k][2:3].tobytes() == b[k].tobytes() for k in b)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(lists_a[2], fe.map_matches(0)))
    c = dict(map_rows=s["map_rows"], map_pts=s["map_pts"], K=R.K, radius=8.0, ratio=0.0, max_distance=0.0)
    _check(fe, c, b, [2], f"refined {det}", frames=[s["frames"][2]], priors=[first["poses"][2]])
    assert b["status"][0] == 0 and b["n_inl"][0] >= 180
    # relocalize(refine_radius=) is relocalize + that pass
    both = fe.relocalize([0, 1, 2], R.K, refine_radius=8.0)
    assert _same(both, a) and both["first_n_match"].tobytes() == first["n_match"].tobytes() and both["first_n_inl"].tobytes() == first["n_inl"].tobytes()
    # a newly staged map forgets the first pass
    fe.relocalize([0, 1, 2], R.K)
    fe.stage_map(s["map_rows"], s["map_pts"])
    with pytest.raises(_lib.VoError):
        fe.relocalize_guided([0, 1, 2], R.K, None, 8.0)


def test_the_other_calls_are_what_they_were(rig):
    from visual_odometry_amd import _lib
    det, fe = rig
    c = G.pose_case(det)
    rows, xy = c["frames"][0]
    _put(fe, det, 1, rows, xy)
    fe.stage_map(c["map_rows"], c["map_pts"])
    before = fe.relocalize([1], R.K)
    lists = fe.map_matches(0)
    with pytest.raises(_lib.VoError):
        fe.map_match_seconds(0)                                            # the cross-check keeps no second distance
    g = fe.relocalize_guided([1], R.K, c["priors"][0][None], c["radius"])
    _check(fe, c, g, [1], f"between {det}")                                # map_matches and map_match_seconds serve the guided call
    after = fe.relocalize([1], R.K)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(lists, fe.map_matches(0)))
    with pytest.raises(_lib.VoError):
        fe.map_match_seconds(0)
    rows_back, pts_back = fe.map_rows()
    assert rows_back.tobytes() == c["map_rows"].tobytes() and pts_back.tobytes() == np.ascontiguousarray(c["map_pts"]).tobytes()


# ------------------------------------------------------------------ arguments
def test_argument_checks():
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    ctx = _lib.Context(0)
    try:
        lib, h = ctx.lib, ctx.handle
        K = np.ascontiguousarray(R.K); opts = _lib.RelocOpts(0.0, 100, 8.0, 0.99, 0xFFFFFFFFFFFFFFFF, 0)
        sl = np.zeros(3, np.int32); prior = np.tile(G.P_IDENTITY.reshape(-1), (3, 1)).copy()
        outs = [np.full((3, 12), 7.0)] + [np.full(3, 7, np.int32) for _ in range(4)]
        g = _lib.GuidedOpts(5.0, 0.0)

        def call(q, pr=prior, gp=g, op=opts, kp=K):
            rc = lib.vo_map_localize_guided(h, sl.ctypes.data, q, None if kp is None else kp.ctypes.data, None if pr is None else pr.ctypes.data,
                                            None if gp is None else C.addressof(gp), None if op is None else C.addressof(op),
                                            *[v.ctypes.data for v in outs])
            if rc != 0:
                assert all((v == 7).all() for v in outs)                   # a refused call writes nothing
            return rc
        assert lib.vo_map_localize_guided(None, sl.ctypes.data, 1, K.ctypes.data, prior.ctypes.data, C.addressof(g), C.addressof(opts),
                                          *[v.ctypes.data for v in outs]) == R.VO_ERR_INVALID
        assert call(1) == R.VO_ERR_NOT_CONFIGURED
        fe = FrontEnd(32, 32, max_frames=2, max_pairs=2, detector="sift", kp_cap=256, ctx=ctx)
        assert call(1) == R.VO_ERR_INVALID                                 # no staged map
        m, mp = R.match_map_rows("sift", 65)
        fe.stage_map(m, mp)
        f, xy = R.match_frame("sift", m, 17)
        fe.set_sift_rows(0, f, xy)
        assert call(3) == R.VO_ERR_INVALID and call(-1) == R.VO_ERR_INVALID            # Q > max_pairs
        assert call(1, gp=None) == R.VO_ERR_INVALID and call(1, op=None) == R.VO_ERR_INVALID and call(1, kp=None) == R.VO_ERR_INVALID
        nan, inf = float("nan"), float("inf")
        for radius in (-1.0, -0.0 - 1e-300, nan, inf, -inf):
            assert call(1, gp=_lib.GuidedOpts(radius, 0.0)) == R.VO_ERR_INVALID, radius
        for ratio in (-0.5, nan, inf, -inf):
            assert call(1, gp=_lib.GuidedOpts(5.0, ratio)) == R.VO_ERR_INVALID, ratio
        for bad in (nan, inf, -inf):
            p = prior.copy(); p[1, 7] = bad
            assert call(2, pr=p) == R.VO_ERR_INVALID, bad
            assert call(1, pr=p) == R.VO_OK                                # (the entry lies beyond the first query)
            for v in outs:
                v[...] = 7
        sl[0] = 2
        assert call(1) == R.VO_ERR_INVALID                                 # slot out of range
        sl[0] = 0
        assert call(1, pr=None) == R.VO_ERR_INVALID                        # no vo_map_localize before it
        assert call(1, gp=_lib.GuidedOpts(0.0, 0.0)) == R.VO_OK and call(0) == R.VO_OK
        n = C.c_int32(0)
        assert lib.vo_map_matches(h, 0, None, None, None, None, 0, C.addressof(n)) == R.VO_ERR_INVALID     # (Q = 0 forgot the queries)
        assert call(1) == R.VO_OK and outs[4][0] >= 0
        assert lib.vo_map_match_seconds(h, 0, 0, None, 0, C.addressof(n)) == R.VO_OK
        # n_seen may be NULL
        assert lib.vo_map_localize_guided(h, sl.ctypes.data, 1, K.ctypes.data, prior.ctypes.data, C.addressof(g), C.addressof(opts),
                                          *[v.ctypes.data for v in outs[:4]], None) == R.VO_OK
        loud = np.full((2, 128), 255, np.uint8)
        fe.set_sift_rows(1, loud, None)                                    # a slot flagged for its norm: refused after the run
        sl[0] = 1
        assert lib.vo_map_localize_guided(h, sl.ctypes.data, 1, K.ctypes.data, prior.ctypes.data, C.addressof(g), C.addressof(opts),
                                          *[v.ctypes.data for v in outs]) == R.VO_ERR_INVALID
    finally:
        ctx.close()

"""GPU: relocalisation of resident frames against a staged map by its descriptors — k_map_gather, k_nn_map / k_nn_map_orb,
k_map_select and, unchanged, k_pnp_ransac behind vo_map_stage / vo_map_from_slam / vo_map_localize — on descriptor rows the test
CHOSE (FrontEnd.set_sift_rows / set_orb_rows for the frames, FrontEnd.stage_map for the map: no detection anywhere), against
tests/relocalize_reference.py, which tests/test_relocalize_reference.py holds equal on the CPU to a plain two-loop matcher and to
what every case is named for.  Both detectors: SIFT rows go through the matrix-core kernel, ORB rows through the popcount one.

Held here:
  matches   indices, float32 distances and order EQUAL the reference: maps of 0, 1, 3, 4, 5, 63, 64, 65, 129, 257 rows (129 and
            257: one row past a chunk of the walked side — 128 SIFT rows, 256 ORB rows), frames of 0, 1, 17, 300 rows, three frames
            of unequal size per call; duplicated rows a lane, a 16-column group and a chunk apart, in the map and in the frames;
            a slot that held a fuller frame, a map staged after a larger one; the distance filter with a match exactly on the bound;
  pose      poses, n_inl, status and the inlier masks BYTE-EQUAL to vo_solve_pnp_ransac_batch on the reference's correspondence
            arrays (the same kernel on the same input; the pose through vo_rodrigues), in every call of this file; against the
            oracle as tests/test_gpu_pnp.py compares the batch call: equal inlier sets, rvec / tvec within its POSE_TOL;
  known pose  exact points, float32 projections, 10 % wrong pixels: the generating pose within tests/test_gpu_pnp.py's bound for
            recovering one (|dR| < 0.02, |dt| < 0.1; the oracle's own error on this data is 5e-9 / 3e-8, printed by the CPU file);
  statuses  3 matches -> VO_ERR_TOO_FEW, contradictory pixels -> VO_ERR_NO_MODEL, min_inliers; failed rows zero, the third query of
            the same call solved;
  map_from_slam  on chosen feature tracks (tests/track_cases.py, four frames): map_rows() equals slam_map()'s points byte for byte
            and the rows features(slot)['desc'][keypoint] picked by pt_feature on the host, for which = 0, which = 1 and seq = 1 of a
            slam_chains call; a held-out fifth frame relocalised; slam_map() and a later slam_stream(resume) unchanged by it; the end map
            once more under a SIFT configuration (the gather by key on 128-byte rows);
  arguments every VO_ERR_* the header names for these entries.
The whole file takes 1.1 s on an MI355X (measured, one run, the oracle's side included); the slowest test 0.1 s."""
import numpy as np
import pytest

import relocalize_reference as R
import track_cases as TC

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-7                    # tests/test_gpu_pnp.py
GEN_TOL_R, GEN_TOL_T = 0.02, 0.1   # tests/test_gpu_pnp.py: recovering a generating pose


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


def _call(fe, det, map_rows, map_pts, frames, slots, what, **opts):
    """One relocalize over `slots` (frames[q] is what slot slots[q] holds) against the reference: matches exactly, and the pose
    part byte for byte against vo_solve_pnp_ransac_batch on the reference's arrays.  Returns (device output, references)."""
    from visual_odometry_amd import geometry
    out = fe.relocalize(slots, R.K, **opts)
    pnp = {k: opts[k] for k in ("iterations", "reproj_err", "confidence", "seed") if k in opts}
    refs = [R.relocalize(map_pts, map_rows, xy, rows, R.K, max_distance=opts.get("max_distance", 0.0)) for rows, xy in frames]
    got = [fe.map_matches(q) for q in range(len(slots))]
    for q, (r, (pi, ki, d, mask)) in enumerate(zip(refs, got)):
        print(what, det, "q", q, "n_match", int(out["n_match"][q]), "ref", r["n_match"], "status", int(out["status"][q]), "n_inl", int(out["n_inl"][q]))
        assert out["n_match"][q] == r["n_match"] == len(pi), (what, q)
        assert np.array_equal(ki, r["qi"]) and np.array_equal(pi, r["ti"]), (what, q)
        assert d.dtype == np.float32 and np.array_equal(d, r["dist"]), (what, q)
    off = np.concatenate([[0], np.cumsum([r["n_match"] for r in refs])]).astype(np.int32)
    obj = np.concatenate([r["obj"] for r in refs]); img = np.concatenate([r["img"] for r in refs])
    st, rvec, tvec, bmask, ninl = geometry.solve_pnp_ransac_batch(obj, img, off, R.K, ctx=fe.ctx, **{
        {"iterations": "iterationsCount", "reproj_err": "reprojectionError"}.get(k, k): v for k, v in pnp.items()})
    min_inl = opts.get("min_inliers", 0)
    for q in range(len(slots)):
        want_st = R.VO_ERR_NO_MODEL if st[q] == 0 and ninl[q] < min_inl else st[q]
        pose = np.zeros((3, 4))
        if want_st == 0:
            pose = np.hstack([geometry.Rodrigues(rvec[q], ctx=fe.ctx)[0], tvec[q].reshape(3, 1)])
        assert out["status"][q] == want_st and out["n_inl"][q] == ninl[q], (what, q)
        assert out["poses"][q].tobytes() == pose.tobytes(), (what, q)
        assert got[q][3].tobytes() == bmask[off[q]:off[q + 1]].tobytes(), (what, q)
    return out, refs, (st, rvec, tvec, bmask, ninl, off)


# ------------------------------------------------------------------ matches
@pytest.mark.parametrize("npt", R.MAP_SIZES)
def test_matches_equal_the_reference(rig, oracle, npt):
    det, fe = rig
    m, pts = R.match_map_rows(det, npt)
    frames = {n: R.match_frame(det, m, n) for n in R.FRAME_SIZES}
    for slot, n in enumerate((300, 17, 1, 0)):
        _put(fe, det, slot, *frames[n])
    fe.stage_map(m, pts)
    rows, points = fe.map_rows()
    assert rows.tobytes() == m.tobytes() and points.tobytes() == np.ascontiguousarray(pts).tobytes()
    a, _, _ = _call(fe, det, m, pts, [frames[300], frames[17], frames[0]], [0, 1, 3], f"npt {npt} a")
    b, _, _ = _call(fe, det, m, pts, [frames[1], frames[300], frames[17]], [2, 0, 1], f"npt {npt} b")
    assert a["n_match"][0] == b["n_match"][1] and a["n_match"][2] == 0
    # two calls on the same input return the same bytes
    again = fe.relocalize([2, 0, 1], R.K)
    assert all(again[k].tobytes() == b[k].tobytes() for k in again)


def test_stale_rows_past_either_end_never_win(rig, oracle):
    """A map staged after a larger one whose rows 5 .. carry the frame's rows exactly; a slot that held a fuller frame whose rows
    17 .. carry the map's rows exactly: either would win at distance 0 if a kernel read past the counts."""
    det, fe = rig
    big, big_pts = R.match_map_rows(det, 257)
    rng = np.random.default_rng(5)
    small = R.rand_rows(rng, 5, det); small_pts = rng.uniform(-2, 2, (5, 3)) + [0, 0, 6]
    frame = big[100:117].copy(); xy = rng.uniform(0, 600, (17, 2)).astype(np.float32)
    full = np.concatenate([R.rand_rows(rng, 17, det), np.tile(small, (57, 1))])[:300]
    _put(fe, det, 0, full, rng.uniform(0, 600, (300, 2)).astype(np.float32))
    _put(fe, det, 0, frame, xy)                                            # rows 17 .. 299 of the slot still hold copies of the small map's rows
    fe.stage_map(big, big_pts)
    out, refs, _ = _call(fe, det, big, big_pts, [(frame, xy)], [0], "big map")
    assert refs[0]["n_match"] == 17 and not refs[0]["dist"].any()
    fe.stage_map(small, small_pts)                                         # rows 5 .. 256 of the image still hold the big map
    out, refs, _ = _call(fe, det, small, small_pts, [(frame, xy)], [0], "small map after the big one")
    assert 1 <= refs[0]["n_match"] <= 5 and refs[0]["dist"].all()
    rows, points = fe.map_rows()
    assert rows.tobytes() == small.tobytes() and len(points) == 5


def test_the_distance_filter_is_strict(rig, oracle):
    det, fe = rig
    c = R.match_case(det, 65, 300)
    _, _, d = R.match_map(c["rows"], c["map_rows"])
    bound = float(np.sort(d)[len(d) // 2])                                 # a distance the reference reports: that match must go
    assert (d == np.float32(bound)).any() and (d < bound).any()
    _put(fe, det, 0, c["rows"], c["xy"])
    fe.stage_map(c["map_rows"], c["map_pts"])
    out, refs, _ = _call(fe, det, c["map_rows"], c["map_pts"], [(c["rows"], c["xy"])], [0], "filter", max_distance=bound)
    assert 0 < refs[0]["n_match"] == int((d < bound).sum()) < len(d)
    out, refs, _ = _call(fe, det, c["map_rows"], c["map_pts"], [(c["rows"], c["xy"])], [0], "no filter", max_distance=-1.0)
    assert refs[0]["n_match"] == len(d)


# ------------------------------------------------------------------ pose
def test_known_pose_against_the_batch_call_the_oracle_and_the_truth(rig, oracle):
    det, fe = rig
    c = R.pose_case(det)
    _put(fe, det, 1, c["rows"], c["xy"])
    fe.stage_map(c["map_rows"], c["map_pts"])
    out, refs, (st, rvec, tvec, bmask, ninl, off) = _call(fe, det, c["map_rows"], c["map_pts"], [(c["rows"], c["xy"])], [1], "pose")
    r = refs[0]
    # ... against the oracle, as tests/test_gpu_pnp.py compares the batch call (the pose above is byte for byte that call's)
    assert st[0] == r["status"] == 0 and ninl[0] == r["n_inl"] and np.array_equal(bmask, r["mask"])
    assert np.abs(rvec[0] - r["rvec"]).max() < POSE_TOL and np.abs(tvec[0] - r["tvec"]).max() < POSE_TOL
    # ... and the generating pose; the wrong pixels are the outliers
    _, _, _, mask = fe.map_matches(0)
    assert np.array_equal(mask > 0, ~c["wrong"]) and out["n_inl"][0] == 180
    err_R, err_t = np.abs(out["poses"][0][:, :3] - c["R"]).max(), np.abs(out["poses"][0][:, 3] - c["t"]).max()
    print(det, "error against the generating pose: R", err_R, "t", err_t)
    assert err_R < GEN_TOL_R and err_t < GEN_TOL_T


def test_the_host_array_convenience_is_the_same_operator(oracle):
    from visual_odometry_amd import _lib, geometry
    ctx = _lib.Context(0)
    try:
        for det in ("sift", "orb"):
            c = R.pose_case(det)
            got = geometry.relocalize(c["map_pts"], c["map_rows"], c["xy"], c["rows"].astype(np.float32) if det == "sift" else c["rows"], R.K, ctx=ctx)
            r = R.relocalize(c["map_pts"], c["map_rows"], c["xy"], c["rows"], R.K)
            pi, ki, d, mask = got["matches"]
            assert got["status"] == 0 and got["n_match"] == 200 and got["n_inl"] == r["n_inl"]
            assert np.array_equal(pi, r["ti"]) and np.array_equal(ki, r["qi"]) and np.array_equal(d, r["dist"]) and np.array_equal(mask, r["mask"])
            assert np.abs(got["pose"][:, :3] - c["R"]).max() < GEN_TOL_R and np.abs(got["pose"][:, 3] - c["t"]).max() < GEN_TOL_T
    finally:
        ctx.close()


# ------------------------------------------------------------------ statuses
def test_statuses_and_min_inliers(rig, oracle):
    det, fe = rig
    c = R.status_case(det)
    for slot, (rows, xy) in enumerate(c["frames"]):
        _put(fe, det, slot, rows, xy)
    fe.stage_map(c["map_rows"], c["map_pts"])
    out, refs, _ = _call(fe, det, c["map_rows"], c["map_pts"], c["frames"], [0, 1, 2], "statuses")
    assert out["n_match"].tolist() == [3, 200, 200]
    assert out["status"].tolist() == [R.VO_ERR_TOO_FEW, R.VO_ERR_NO_MODEL, R.VO_OK] == [r["status"] for r in refs]
    assert not out["poses"][:2].any() and out["n_inl"][:2].tolist() == [0, refs[1]["n_inl"]]
    assert np.abs(out["poses"][2][:, :3] - c["R"]).max() < GEN_TOL_R and np.abs(out["poses"][2][:, 3] - c["t"]).max() < GEN_TOL_T
    n = int(out["n_inl"][2])
    keep, _, _ = _call(fe, det, c["map_rows"], c["map_pts"], c["frames"], [0, 1, 2], "min_inliers reached", min_inliers=n)
    assert keep["status"][2] == R.VO_OK and keep["poses"].tobytes() == out["poses"].tobytes()
    cut, _, _ = _call(fe, det, c["map_rows"], c["map_pts"], c["frames"], [0, 1, 2], "min_inliers missed", min_inliers=n + 1)
    assert cut["status"].tolist() == [R.VO_ERR_TOO_FEW, R.VO_ERR_NO_MODEL, R.VO_ERR_NO_MODEL]
    assert cut["n_inl"][2] == n and not cut["poses"].any()


# ------------------------------------------------------------------ map_from_slam
H = W = 64
OPTS = dict(ba_iterations=0, filter_threshold=1.0, max_cameras=4)


def _picked_rows(fe, m, slot_of_frame):
    """The rows features(slot)['desc'][keypoint] of every point's owning feature, picked on the host by pt_feature."""
    desc = {f: fe.features(s)["desc"] for f, s in slot_of_frame.items()}
    return np.stack([desc[int(f)][int(k)] for f, k in m["pt_feature"]]) if len(m["pt_feature"]) else np.zeros((0, 32), np.uint8)


def _same_map(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_map_from_slam_gathers_the_owning_features_rows(oracle):
    from visual_odometry_amd.frontend import FrontEnd
    ca, cb = TC.cases()["tracks_births"], TC.cases()["tracks_every_frame"]
    fa, fb = TC.frames(oracle, ca), TC.frames(oracle, cb)
    fe = FrontEnd(H, W, max_frames=10, max_pairs=6, nfeatures=ca.nfeatures, nlevels=1)
    try:
        fe.ctx.set_poly_solver("opencv300")
        for k in range(5):                                                 # slots 0 .. 3: the chain; slot 4: the held-out fifth frame
            fe.set_orb_rows(k, fa[k]["desc"], fa[k]["xy"])
            fe.set_orb_rows(5 + k, fb[k]["desc"], fb[k]["xy"])
        pairs = [[0, 1], [1, 2], [2, 3]]
        res, _ = fe.run_pairs(pairs, TC.K, fe.make_opts(want_points=True), want_points=True)
        assert res["status"].tolist() == [0, 0, 0]
        out = fe.slam_chain(3, TC.K, snapshot=(1, 1), **OPTS)
        assert out["status"].tolist() == [0, 0, 0]
        slot_of_frame = {0: 0, 1: 1, 2: 2, 3: 3}
        for which in (0, 1):
            m = fe.slam_map(which)
            fe.map_from_slam(which)
            rows, points = fe.map_rows()
            assert len(points) == len(m["points"]) > 0 and points.tobytes() == m["points"].tobytes(), which
            assert rows.tobytes() == _picked_rows(fe, m, slot_of_frame).tobytes(), which
        assert len(fe.slam_map(1)["points"]) < len(fe.slam_map(0)["points"])      # (the births of frame 2 came after the snapshot)

        # the held-out fifth frame, placed by its descriptors alone: the reference's answer, and the scene's camera 4 up to the
        # chain's own drift (the map is the chain's, in the chain's gauge: camera 1 = identity)
        before = fe.slam_map(0)
        fe.map_from_slam(0)
        rows, points = fe.map_rows()
        out5, refs, _ = _call(fe, "orb", rows, points, [(fa[4]["desc"], fa[4]["xy"])], [4], "held-out frame")
        assert out5["status"][0] == 0 and out5["n_inl"][0] >= 30
        assert _same_map(before, fe.slam_map(0))                           # the chain's map is untouched by the relocalisation

        # seq = 1 of a slam_chains call
        pairs2 = pairs + [[5, 6], [6, 7], [7, 8]]
        res, _ = fe.run_pairs(pairs2, TC.K, fe.make_opts(want_points=True), want_points=True)
        outs = fe.slam_chains([3, 3], TC.K, **OPTS)
        assert outs[1]["status"].tolist() == [0, 0, 0]
        m1 = fe.slam_map(0, seq=1)
        fe.map_from_slam(0, seq=1)
        rows, points = fe.map_rows()
        assert points.tobytes() == m1["points"].tobytes() and rows.tobytes() == _picked_rows(fe, m1, {0: 5, 1: 6, 2: 7, 3: 8}).tobytes()
        fe.map_from_slam(0, seq=0)
        assert fe.map_rows()[1].tobytes() == fe.slam_map(0)["points"].tobytes() == before["points"].tobytes()

        # a stream: a relocalisation between two of its calls changes neither the map nor the continuation
        fe.run_pairs(pairs[:2], TC.K, fe.make_opts(want_points=True), want_points=True)
        fe.slam_stream(2, TC.K, total_pairs=3, **OPTS)
        with pytest.raises(NotImplementedError):
            fe.map_from_slam(0)                                            # a stream's map: its older frames lose their slots
        held = fe.slam_map(0)
        fe.run_pairs([[2, 3]], TC.K, fe.make_opts(want_points=True), want_points=True)
        want = fe.slam_stream(1, TC.K, resume=True, **OPTS)
        want_map = fe.slam_map(0)
        fe.run_pairs(pairs[:2], TC.K, fe.make_opts(want_points=True), want_points=True)
        fe.slam_stream(2, TC.K, total_pairs=3, **OPTS)
        assert _same_map(held, fe.slam_map(0))
        again = fe.relocalize([4], TC.K)                                   # the map staged from the chains call is still there
        assert again["status"][0] == 0 and _same_map(held, fe.slam_map(0))
        fe.run_pairs([[2, 3]], TC.K, fe.make_opts(want_points=True), want_points=True)
        fe.relocalize([4, 3], TC.K)
        got = fe.slam_stream(1, TC.K, resume=True, **OPTS)
        assert all(got[k].tobytes() == want[k].tobytes() for k in want) and _same_map(want_map, fe.slam_map(0))
    finally:
        fe.ctx.close()


def test_map_from_slam_under_a_sift_configuration(oracle):
    """The gather by key on 128-byte rows: the same chosen tracks with one distinct SIFT-like row per scene point instead of its ORB
    row (exact copies match at distance 0 under the L2 cross-check, so the pairs' match lists are the case's)."""
    from visual_odometry_amd.frontend import FrontEnd
    c = TC.cases()["tracks_births"]
    fr = TC.frames(oracle, c)
    table = R.rand_rows(np.random.default_rng(31), len(c.X), "sift")
    assert len(np.unique(table, axis=0)) == len(table) and all((f["ids"] >= 0).all() for f in fr[:5])
    fe = FrontEnd(32, 32, max_frames=5, max_pairs=3, detector="sift", kp_cap=256)
    try:
        fe.ctx.set_poly_solver("opencv300")
        for k in range(5):
            fe.set_sift_rows(k, table[fr[k]["ids"]], fr[k]["xy"])
        res, _ = fe.run_pairs([[0, 1], [1, 2], [2, 3]], TC.K, fe.make_opts(want_points=True), want_points=True)
        assert res["status"].tolist() == [0, 0, 0]
        for p in range(3):
            qi, ti = TC.matches(c, p)
            q, t, _, _ = fe.pair_matches(p)
            assert np.array_equal(q, qi) and np.array_equal(t, ti)
        out = fe.slam_chain(3, TC.K, **OPTS)
        assert out["status"].tolist() == [0, 0, 0]
        m = fe.slam_map(0)
        fe.map_from_slam(0)
        rows, points = fe.map_rows()
        desc = {k: fe.features(k)["desc"].astype(np.uint8) for k in range(4)}
        picked = np.stack([desc[int(f)][int(k)] for f, k in m["pt_feature"]])
        assert len(points) == 40 and points.tobytes() == m["points"].tobytes() and rows.tobytes() == picked.tobytes()
        out5, refs, _ = _call(fe, "sift", rows, points, [(table[fr[4]["ids"]], fr[4]["xy"])], [4], "held-out frame, sift")
        assert out5["status"][0] == 0 and out5["n_match"][0] == 40 and out5["n_inl"][0] >= 30
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ arguments
def test_argument_checks(oracle):
    import ctypes as C
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    ctx = _lib.Context(0)
    try:
        lib, h = ctx.lib, ctx.handle
        rows = np.zeros((4, 128), np.uint8); pts = np.zeros((4, 3))
        n = C.c_int32(0)
        assert lib.vo_map_stage(h, rows.ctypes.data, pts.ctypes.data, 4) == R.VO_ERR_NOT_CONFIGURED
        assert lib.vo_map_from_slam(h, 0, 0) == R.VO_ERR_INVALID
        assert lib.vo_map_rows(h, None, None, 0, C.addressof(n)) == R.VO_ERR_INVALID
        fe = FrontEnd(32, 32, max_frames=2, max_pairs=2, detector="sift", kp_cap=256, ctx=ctx)
        K = np.ascontiguousarray(R.K); opts = _lib.RelocOpts(0.0, 100, 8.0, 0.99, 0xFFFFFFFFFFFFFFFF, 0)
        sl = np.zeros(3, np.int32); poses = np.zeros((3, 12)); i32 = [np.zeros(3, np.int32) for _ in range(3)]

        def localize(q):
            return lib.vo_map_localize(h, sl.ctypes.data, q, K.ctypes.data, C.addressof(opts), poses.ctypes.data, *[v.ctypes.data for v in i32])
        assert localize(1) == R.VO_ERR_INVALID                             # no staged map
        assert lib.vo_map_matches(h, 0, None, None, None, None, 0, C.addressof(n)) == R.VO_ERR_INVALID
        big = np.zeros((65537, 128), np.uint8)
        assert lib.vo_map_stage(h, big.ctypes.data, np.zeros((65537, 3)).ctypes.data, 65537) == R.VO_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            fe.stage_map(big, np.zeros((65537, 3)))
        assert lib.vo_map_stage(h, None, None, 3) == R.VO_ERR_INVALID and lib.vo_map_stage(h, None, None, -1) == R.VO_ERR_INVALID
        loud = np.full((2, 128), 255, np.uint8)                            # |row|^2 = 128 * 255^2 > 2^20
        assert lib.vo_map_stage(h, loud.ctypes.data, pts.ctypes.data, 2) == R.VO_ERR_INVALID
        assert localize(1) == R.VO_ERR_INVALID                             # ... and nothing is staged then
        m, mp = R.match_map_rows("sift", 65)
        fe.stage_map(m, mp)
        f, xy = R.match_frame("sift", m, 17)
        fe.set_sift_rows(0, f, xy)
        assert localize(1) == R.VO_OK and localize(0) == R.VO_OK
        assert localize(3) == R.VO_ERR_INVALID and localize(-1) == R.VO_ERR_INVALID   # Q > max_pairs
        assert lib.vo_map_matches(h, 0, None, None, None, None, 0, C.addressof(n)) == R.VO_ERR_INVALID   # (localize(0) forgot the queries)
        sl[0] = 2
        assert localize(1) == R.VO_ERR_INVALID                             # slot out of range
        sl[0] = 0
        assert localize(1) == R.VO_OK and lib.vo_map_matches(h, 1, None, None, None, None, 0, C.addressof(n)) == R.VO_ERR_INVALID
        assert lib.vo_map_from_slam(h, 0, 0) == R.VO_ERR_INVALID           # no chain has run
        fe.set_sift_rows(1, loud, None)                                    # a slot flagged for its norm: refused after the run
        sl[0] = 1
        assert localize(1) == R.VO_ERR_INVALID
        sl[0] = 0
        assert localize(1) == R.VO_OK                                      # ... the other slots are fine
        # ORB rows are 32 bytes wide under an ORB configuration; a configure call releases the map
        fe2 = FrontEnd(64, 64, max_frames=2, max_pairs=2, nfeatures=8, nlevels=1, ctx=ctx)
        assert localize(1) == R.VO_ERR_INVALID
        with pytest.raises(ValueError):
            fe2.stage_map(m, mp)
        mo, mpo = R.match_map_rows("orb", 5)
        fe2.stage_map(mo, mpo)
        assert fe2.map_rows()[0].tobytes() == mo.tobytes()
    finally:
        ctx.close()

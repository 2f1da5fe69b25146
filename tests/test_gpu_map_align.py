"""GPU: vo_map_align (FrontEnd.align_maps / map_align_matches) — k_align_gather, k_nn_align / k_nn_align_orb, k_align_select and
k_sim3_ransac — against tests/map_align_reference.py, on descriptor rows and points the test CHOSE, through FrontEnd.stage_map; both
detectors (SIFT rows: the matrix-core body, ORB rows: the popcount body).

Held here:
  matches   indices, float32 distances and order EQUAL the checker's: staged maps of 513, 257 and 3 rows (in that order: the smaller
            maps lie in an allocation that still holds the larger one), query maps of 257, 0, 65 rows in one call and of 64, 1, 2, 3
            rows in the next; duplicated rows a lane, a 16-column group and a chunk apart on both sides; stale rows past either
            end that would win at distance 0; the strict distance filter with a match on the bound;
  model     sim, n_inl, status and the inlier masks BYTE-EQUAL to vo_sim3_ransac_batch on the checker's correspondence lists, in
            every call of this file: the same kernel on the same input;
  refusals  every one the header names, and after each the context returns the same bytes as before;
  neighbours  relocalize() on the same staged map returns identical bytes before and after an align_maps call;
  a flight  two overlapping sub-sequences of a rendered flight through slam_chains, map 1 aligned into map 0: the device's join
            against the checker's on the same saved arrays, and the distance between the two tracks' camera centres on the shared
            frames after the join, relative to the track length (printed; recorded in docs/kernels/k_sim3_ransac.md)."""
import ctypes as C

import numpy as np
import pytest

import map_align_reference as A
import relocalize_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=("sift", "orb"))
def rig(request):
    from visual_odometry_amd.frontend import FrontEnd
    det = request.param
    if det == "sift":
        fe = FrontEnd(32, 32, max_frames=2, max_pairs=1, detector="sift", kp_cap=512)
    else:
        fe = FrontEnd(64, 64, max_frames=2, max_pairs=1, nfeatures=304, nlevels=1)
    yield det, fe
    fe.ctx.close()


def _call(fe, map_rows, map_pts, queries, max_error, what, **opts):
    """One align_maps over `queries` [(rows, points)] against the checker: the match lists exactly, and the model part byte for byte
    against vo_sim3_ransac_batch on the checker's lists.  Returns (device output, the checker's match lists)."""
    from visual_odometry_amd import geometry
    off = np.concatenate([[0], np.cumsum([len(r) for r, _ in queries])]).astype(np.int32)
    rows = np.concatenate([r for r, _ in queries]); pts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for _, p in queries])
    out = fe.align_maps(rows, pts, max_error, offsets=off, **opts)
    refs = []
    for q, (qr, qp) in enumerate(queries):
        bi, ai, d = R.match_map(qr, map_rows, opts.get("max_distance", 0.0))
        refs.append(dict(bi=bi, ai=ai, dist=d, src=np.asarray(qp, np.float64).reshape(-1, 3)[bi], dst=np.asarray(map_pts, np.float64)[ai]))
        ga, gb, gd, _ = fe.map_align_matches(q)
        print(what, "q", q, "rows", len(qr), "n_match", int(out["n_match"][q]), "checker", len(bi), "status", int(out["status"][q]), "n_inl", int(out["n_inl"][q]))
        assert out["n_match"][q] == len(bi) == len(ga), (what, q)
        assert np.array_equal(gb, bi) and np.array_equal(ga, ai), (what, q)
        assert gd.dtype == np.float32 and np.array_equal(gd, d), (what, q)
    moff = np.concatenate([[0], np.cumsum([len(r["bi"]) for r in refs])]).astype(np.int32)
    ransac = {k: opts[k] for k in ("iterations", "confidence", "seed", "min_inliers") if k in opts}
    want = geometry.estimate_similarity_batch(np.concatenate([r["src"] for r in refs]).reshape(-1, 3), np.concatenate([r["dst"] for r in refs]).reshape(-1, 3),
                                              moff, max_error, ctx=fe.ctx, **ransac)
    for key in ("scale", "R", "t", "n_inl", "status"):
        assert out[key].tobytes() == want[key].tobytes(), (what, key)
    out["masks"] = [fe.map_align_matches(q)[3] for q in range(len(queries))]
    for q in range(len(queries)):
        assert out["masks"][q].tobytes() == want["mask"][moff[q]:moff[q + 1]].tobytes(), (what, q)
    return out, refs


def test_matches_and_models_on_every_size(rig, oracle):
    det, fe = rig
    for npt in (513, 257, 3):
        c = {n: A.align_case(det, npt, n) for n in (257, 0, 65, 64, 1, 2, 3)}
        m, mp = c[257]["map_rows"], c[257]["map_pts"]
        assert all(np.array_equal(v["map_rows"], m) for v in c.values())
        fe.stage_map(m, mp)
        a, ra = _call(fe, m, mp, [(c[n]["rows"], c[n]["pts"]) for n in (257, 0, 65)], 0.05, f"{det} npt {npt} a")
        b, _ = _call(fe, m, mp, [(c[n]["rows"], c[n]["pts"]) for n in (64, 1, 2, 3)], 0.05, f"{det} npt {npt} b")
        assert a["status"][1] == A.VO_ERR_TOO_FEW and a["n_match"][1] == 0                     # the empty map, for that query alone
        assert all(b["status"][q] == A.VO_ERR_TOO_FEW for q in (1, 2)) and b["n_match"][1] <= 1 and b["n_match"][2] <= 2
        if npt >= 257:
            for q, n in ((0, 257), (2, 65)):
                ref = A.sim3_ransac(ra[q]["src"], ra[q]["dst"], 0.05)
                assert ref["nearest"] > A.PREMISE and a["status"][q] == ref["status"] == 0 and a["n_inl"][q] == ref["n_inl"]
                assert np.array_equal(a["masks"][q], ref["mask"])
                err = A.model_error((a["scale"][q], a["R"][q], a["t"][q]), c[n]["model"])
                print(det, npt, n, "device error against the generating similarity", err)
                assert all(e <= A.MARGIN * ce for e, ce in zip(err, A.checker_error()))
        again = fe.align_maps(np.concatenate([c[n]["rows"] for n in (64, 1, 2, 3)]), np.concatenate([c[n]["pts"] for n in (64, 1, 2, 3)]), 0.05,
                              offsets=[0, 64, 65, 67, 70])
        assert all(again[k].tobytes() == b[k].tobytes() for k in again)                        # the same input, the same bytes
        assert all(fe.map_align_matches(q)[3].tobytes() == b["masks"][q].tobytes() for q in range(4))


def test_stale_rows_past_either_end_never_win(rig, oracle):
    """A staged map of 5 rows after one of 257 whose rows 5 .. carry the query's rows exactly; a query map of 17 rows after one of
    257 whose rows 17 .. carry the staged map's rows exactly: either would win at distance 0 if a kernel read past the counts."""
    det, fe = rig
    big, big_pts = R.match_map_rows(det, 257)
    rng = np.random.default_rng(15)
    small = R.rand_rows(rng, 5, det); small_pts = rng.uniform(-2, 2, (5, 3)) + [0, 0, 6]
    query = big[100:117].copy(); qp = rng.uniform(-3, 3, (17, 3))
    full = np.concatenate([R.rand_rows(rng, 17, det), np.tile(small, (48, 1))]); fp = rng.uniform(-3, 3, (len(full), 3))
    assert len(full) == 257
    fe.stage_map(big, big_pts)
    _call(fe, big, big_pts, [(full, fp)], 0.05, "the fuller query first")
    out, refs = _call(fe, big, big_pts, [(query, qp)], 0.05, "big map")
    assert len(refs[0]["bi"]) == 17 and not refs[0]["dist"].any()
    fe.stage_map(small, small_pts)                                         # rows 5 .. 256 of the image still hold the big map
    _call(fe, small, small_pts, [(full, fp)], 0.05, "the fuller query against the small map")
    out, refs = _call(fe, small, small_pts, [(query, qp)], 0.05, "small map after the big one")   # query rows 17 .. still hold copies of the small map
    assert 1 <= len(refs[0]["bi"]) <= 5 and refs[0]["dist"].all()


def test_the_distance_filter_is_strict(rig, oracle):
    det, fe = rig
    c = A.align_case(det, 65, 300)
    _, _, d = R.match_map(c["rows"], c["map_rows"])
    bound = float(np.sort(d)[len(d) // 2])                                 # a distance the checker reports: that match must go
    assert (d == np.float32(bound)).any() and (d < bound).any()
    fe.stage_map(c["map_rows"], c["map_pts"])
    out, refs = _call(fe, c["map_rows"], c["map_pts"], [(c["rows"], c["pts"])], 0.05, "filter", max_distance=bound)
    assert 0 < len(refs[0]["bi"]) == int((d < bound).sum()) < len(d)
    out, refs = _call(fe, c["map_rows"], c["map_pts"], [(c["rows"], c["pts"])], 0.05, "no filter", max_distance=-1.0)
    assert len(refs[0]["bi"]) == len(d)
    out, _ = _call(fe, c["map_rows"], c["map_pts"], [(c["rows"], c["pts"])], 0.05, "options", seed=77, iterations=65, min_inliers=10 ** 6)
    assert out["status"][0] == A.VO_ERR_NO_MODEL and out["n_inl"][0] > 0 and not out["R"][0].any()


def test_every_refusal_leaves_the_context_as_it_was(rig, oracle):
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    det, fe = rig
    D = 128 if det == "sift" else 32
    c = A.align_case(det, 257, 65)
    fe.stage_map(c["map_rows"], c["map_pts"])
    first = fe.align_maps(c["rows"], c["pts"], 0.05)
    first_m = fe.map_align_matches(0)

    def same():
        again = fe.align_maps(c["rows"], c["pts"], 0.05)
        assert all(again[k].tobytes() == first[k].tobytes() for k in first)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(fe.map_align_matches(0), first_m))

    lib, h = fe.ctx.lib, fe.ctx.handle
    rows = np.ascontiguousarray(c["rows"]); pts = np.ascontiguousarray(c["pts"])
    sim = np.zeros(13 * 70); i32 = [np.zeros(70, np.int32) for _ in range(3)]
    n = C.c_int32(0)

    def raw(off, Q, opts=None, r=rows, p=pts):
        o = opts or _lib.AlignOpts(0.0, 0.05, 1000, 0.99, 0xFFFFFFFFFFFFFFFF, 0)
        off = np.ascontiguousarray(off, np.int32)
        return lib.vo_map_align(h, r.ctypes.data, p.ctypes.data, off.ctypes.data, Q, C.addressof(o), sim.ctypes.data, *[v.ctypes.data for v in i32])

    for bad in (_lib.AlignOpts(0.0, 0.0, 1000, 0.99, 1, 0), _lib.AlignOpts(0.0, -2.0, 1000, 0.99, 1, 0), _lib.AlignOpts(0.0, 0.05, 1000, 1.0, 1, 0)):
        assert raw([0, 65], 1, bad) == A.VO_ERR_INVALID
        assert lib.vo_map_align_matches(h, 0, None, None, None, None, 0, C.addressof(n)) == A.VO_ERR_INVALID    # a refused call forgets the queries
        same()
    assert raw([1, 65], 1) == A.VO_ERR_INVALID and raw([0, 40, 30], 2) == A.VO_ERR_INVALID and raw([0, 65], -1) == A.VO_ERR_INVALID
    assert lib.vo_map_align(h, None, None, np.array([0, 65], np.int32).ctypes.data, 1, None, sim.ctypes.data, *[v.ctypes.data for v in i32]) == A.VO_ERR_INVALID
    same()
    assert raw(np.arange(66), 65) == A.VO_ERR_UNSUPPORTED                                      # Q > 64
    with pytest.raises(NotImplementedError):
        fe.align_maps(np.zeros((65537, D), np.uint8), np.zeros((65537, 3)), 0.05)              # more than 65536 query rows
    same()
    assert raw(np.arange(65), 64) == 0                                                         # 64 maps of one row each: the bound itself
    assert (i32[2][:64] == A.VO_ERR_TOO_FEW).all()
    assert lib.vo_map_align_matches(h, 64, None, None, None, None, 0, C.addressof(n)) == A.VO_ERR_INVALID
    assert lib.vo_map_align_matches(h, -1, None, None, None, None, 0, C.addressof(n)) == A.VO_ERR_INVALID
    same()
    with pytest.raises(ValueError):
        fe.align_maps(c["rows"][:, :D - 1], c["pts"], 0.05)
    with pytest.raises(ValueError):
        fe.align_maps(c["rows"], c["pts"][:-1], 0.05)
    if det == "sift":                                                                          # the norm bound of the integer matcher, as vo_map_stage has it
        loud = c["rows"].copy(); loud[7] = 255
        with pytest.raises(_lib.VoError) as e:
            fe.align_maps(loud, c["pts"], 0.05)
        assert e.value.code == A.VO_ERR_INVALID
        same()
    # no staged map: a configured context that never staged one, and this one after a configure call
    other = FrontEnd(32, 32, max_frames=1, max_pairs=1, detector="sift", kp_cap=64) if det == "sift" else FrontEnd(64, 64, max_frames=1, max_pairs=1, nfeatures=64, nlevels=1)
    with pytest.raises(_lib.VoError) as e:
        other.align_maps(c["rows"], c["pts"], 0.05)
    assert e.value.code == A.VO_ERR_INVALID
    other.ctx.close()


def test_relocalize_is_left_alone(rig, oracle):
    det, fe = rig
    c = R.pose_case(det)
    (fe.set_sift_rows if det == "sift" else fe.set_orb_rows)(0, c["rows"], c["xy"])
    fe.stage_map(c["map_rows"], c["map_pts"])
    before = fe.relocalize([0], R.K); before_m = fe.map_matches(0)
    assert before["status"][0] == 0
    q = A.align_case(det, 200, 65)
    fe.align_maps(q["rows"], q["pts"], 0.05)
    kept = fe.map_matches(0)                                                                   # the latest relocalize's lists are still there
    assert all(x.tobytes() == y.tobytes() for x, y in zip(kept, before_m))
    after = fe.relocalize([0], R.K)
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fe.map_matches(0), before_m))


# ------------------------------------------------------------------ a rendered flight, two overlapping sub-sequences
FLIGHT_MAX_ERROR = 0.1             # in map 0's units (its first pair's baseline): a tenth of the step between two frames


def _centres(poses):
    return np.stack([-T[:, :3].T @ T[:, 3] for T in poses])


def test_two_overlapping_flights_join(oracle):
    """Frames 0..3 and frames 1..4 of the restart tests' flight, each a sequence of slam_chains with a map of its own (816 and 848
    points in a run on an MI355X; 634 matches, 577 inliers at max_error 0.1).  (The sub-sequence that starts at frame 2 is not used:
    the map step leaves its points behind its cameras, and no similarity mends a track that is wrong in its own gauge.)"""
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd, apply_similarity
    seq = synth.sequence(7, 640, 480, step=4.0, cache_dir="/tmp")
    K = seq["K"]
    fe = FrontEnd(480, 640, max_frames=8, max_pairs=6, nfeatures=1000)
    fe.upload(np.stack([seq["frames"][f] for f in (0, 1, 2, 3, 1, 2, 3, 4)])); fe.detect(0, 8)     # frames 0..3 and frames 1..4
    fe.run_pairs([[0, 1], [1, 2], [2, 3], [4, 5], [5, 6], [6, 7]], K, want_points=True)
    outs = fe.slam_chains([3, 3], K)
    assert all((o["status"] == 0).all() for o in outs)
    fe.map_from_slam(seq=1); rows1, pts1 = fe.map_rows()
    fe.map_from_slam(seq=0); rows0, pts0 = fe.map_rows()                   # map 0 stays staged
    out = fe.align_maps(rows1, pts1, FLIGHT_MAX_ERROR)
    ga, gb, gd, gm = fe.map_align_matches(0)
    ref = A.map_align(rows0, pts0, rows1, pts1, FLIGHT_MAX_ERROR)
    print("maps", len(rows0), len(rows1), "matches", ref["n_match"], "inliers", ref["n_inl"], "checker iterations", ref["iters"], "nearest", ref["nearest"])
    assert ref["nearest"] > A.PREMISE                                      # the premise, on this data
    assert np.array_equal(ga, ref["ai"]) and np.array_equal(gb, ref["bi"]) and np.array_equal(gd, ref["dist"])
    assert out["status"][0] == ref["status"] == 0 and out["n_inl"][0] == ref["n_inl"] and np.array_equal(gm, ref["mask"])
    dev, chk = (out["scale"][0], out["R"][0], out["t"][0]), (ref["scale"], ref["R"], ref["t"])
    err = A.model_error(dev, chk)
    bound = tuple(A.MARGIN * v for v in A.checker_error())
    print("device against the checker  s %.2e  R %.2e  t %.2e   bound  s %.2e  R %.2e  t %.2e" % (err + bound), " scale", chk[0])
    assert all(e <= b for e, b in zip(err, bound))
    # the shared frames 1, 2, 3: rows 1..3 of track 0, rows 0..2 of track 1
    c0 = _centres(outs[0]["poses"][1:4])
    before = np.linalg.norm(c0 - _centres(outs[1]["poses"][0:3]), axis=1).mean()
    after_dev = np.linalg.norm(c0 - _centres(apply_similarity(outs[1]["poses"][0:3], *dev)), axis=1).mean()
    after_chk = np.linalg.norm(c0 - _centres(apply_similarity(outs[1]["poses"][0:3], *chk)), axis=1).mean()
    track = np.linalg.norm(np.diff(_centres(outs[0]["poses"]), axis=0), axis=1).sum()
    print("camera centres on the shared frames: before %.4f  after (device) %.6f  after (checker) %.6f  track length %.4f  relative %.2e  factor %.1f"
          % (before, after_dev, after_chk, track, after_dev / track, before / after_dev))
    # an absent or identity join leaves `before`: the device must reach the checker's improvement, within the margin
    assert after_chk < before
    assert before / after_dev >= (before / after_chk) / A.MARGIN
    assert abs(after_dev - after_chk) <= bound[2] + bound[0] * track + bound[1] * track
    fe.ctx.close()

"""GPU: ratio-test matching against the staged map — vo_set_map_match modes 1 (knnMatch(k=2) + `m.distance < ratio * n.distance`) and
2 (the cross-check and that rule) of vo_map_localize and vo_map_align: the top-2 instantiations of k_nn_map / k_nn_map_orb /
k_nn_align / k_nn_align_orb, and k_map_select / k_align_select — on descriptor rows the test CHOSE (set_sift_rows / set_orb_rows,
stage_map), against tests/map_ratio_reference.py, which tests/test_map_ratio_reference.py holds equal on the CPU to a plain two-loop
matcher and to what every case is there for.  Both detectors.

Held here, in both modes:
  lists     map index, query index, float32 distance, float32 SECOND distance (vo_map_match_seconds) and order EQUAL the reference:
            maps of 0, 1, 2, 3, 17, 63, 64, 65, 129, 257 rows, frames of 0, 1, 17, 300 rows, three frames of unequal size per call;
            nearest and second nearest placed in one lane, two lanes of a group, two groups of a chunk, two chunks (128+ and 256+
            apart), the second before and after the first; an exact tie for nearest (rejected for ratio <= 1, kept above it with the
            lower index and n.distance == m.distance) and for second place; distances 3 and 4 at ratio 0.75 rejected, 3 and 5 kept;
            max_distance on top, with a match on each bound; two query rows keeping one map row; stale rows past either end; a map of
            65536 rows with the two neighbours at its ends;
  pose      poses, n_inl, status and inlier masks BYTE-EQUAL to vo_solve_pnp_ransac_batch on the reference's lists; a map of one row
            VO_ERR_TOO_FEW;
  align     vo_map_align's lists and seconds equal the reference on two maps with distractor rows; sim, n_inl, status and masks
            BYTE-EQUAL to vo_sim3_ransac_batch on those lists;
  setting   mode 0 after a mode-1 call returns the bytes it returned before it; vo_map_match_seconds after a mode-0 call is
            VO_ERR_INVALID; two calls on the same input return the same bytes.
The whole file takes 1.9 s on an MI355X (measured, one run, the oracle's side included); the slowest test 0.3 s (the long map)."""
import ctypes as C

import numpy as np
import pytest

import map_ratio_reference as M
import relocalize_reference as R

pytestmark = pytest.mark.gpu

MODES = {1: "ratio", 2: "cross+ratio"}
POSE_TOL = 1e-7                    # tests/test_gpu_pnp.py


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


def _call(fe, map_rows, map_pts, frames, slots, what, mode, ratio=M.RATIO, **opts):
    """One relocalize over `slots` (frames[q] is what slot slots[q] holds) in `mode` against the reference: the lists and the second
    distances exactly, the pose part byte for byte against vo_solve_pnp_ransac_batch on the reference's arrays."""
    from visual_odometry_amd import geometry
    out = fe.relocalize(slots, M.K, match=MODES[mode], ratio=ratio, **opts)
    refs = []
    for q, (rows, xy) in enumerate(frames):
        qi, ti, d, d2 = M.match(rows, map_rows, mode, ratio, opts.get("max_distance", 0.0))
        obj, img = R.correspondences(map_pts, xy, qi, ti)
        refs.append(dict(qi=qi, ti=ti, dist=d, dist2=d2, obj=obj, img=img, n_match=len(qi)))
        pi, ki, gd, _ = fe.map_matches(q)
        g2 = fe.map_match_seconds(q)
        print(what, "mode", mode, "q", q, "rows", len(rows), "n_match", int(out["n_match"][q]), "ref", len(qi), "status", int(out["status"][q]))
        assert out["n_match"][q] == len(qi) == len(pi) == len(g2), (what, mode, q)
        assert np.array_equal(ki, qi) and np.array_equal(pi, ti), (what, mode, q)
        assert gd.dtype == g2.dtype == np.float32 and np.array_equal(gd, d) and np.array_equal(g2, d2), (what, mode, q)
    off = np.concatenate([[0], np.cumsum([r["n_match"] for r in refs])]).astype(np.int32)
    pnp = {{"iterations": "iterationsCount", "reproj_err": "reprojectionError"}.get(k, k): opts[k] for k in ("iterations", "reproj_err", "confidence", "seed") if k in opts}
    st, rvec, tvec, bmask, ninl = geometry.solve_pnp_ransac_batch(np.concatenate([r["obj"] for r in refs]), np.concatenate([r["img"] for r in refs]), off,
                                                                  M.K, ctx=fe.ctx, **pnp)
    for q in range(len(slots)):
        pose = np.zeros((3, 4))
        if st[q] == 0:
            pose = np.hstack([geometry.Rodrigues(rvec[q], ctx=fe.ctx)[0], tvec[q].reshape(3, 1)])
        assert out["status"][q] == st[q] and out["n_inl"][q] == ninl[q], (what, mode, q)
        assert out["poses"][q].tobytes() == pose.tobytes(), (what, mode, q)
        assert fe.map_matches(q)[3].tobytes() == bmask[off[q]:off[q + 1]].tobytes(), (what, mode, q)
    return out, refs, (st, rvec, tvec, bmask, ninl)


# ------------------------------------------------------------------ lists
@pytest.mark.parametrize("npt", M.MAP_SIZES)
def test_lists_and_seconds_equal_the_reference(rig, oracle, npt):
    det, fe = rig
    m, pts, frames = M.call_frames(det, npt)
    for slot, n in enumerate((300, 17, 1, 0)):
        _put(fe, det, slot, *frames[n])
    fe.stage_map(m, pts)
    for mode in (1, 2):
        a, ra, _ = _call(fe, m, pts, [frames[300], frames[17], frames[0]], [0, 1, 3], f"{det} npt {npt} a", mode)
        b, rb, _ = _call(fe, m, pts, [frames[1], frames[300], frames[17]], [2, 0, 1], f"{det} npt {npt} b", mode)
        assert a["n_match"][0] == b["n_match"][1] and a["n_match"][2] == 0
        assert (a["n_match"][0] > 0) == (npt >= 2)                        # a map of 0 or 1 rows gives no match; every other map some
        if npt < 2:
            assert (a["status"] == M.VO_ERR_TOO_FEW).all() and (b["status"] == M.VO_ERR_TOO_FEW).all()
        again = fe.relocalize([2, 0, 1], M.K, match=MODES[mode], ratio=M.RATIO)                # the same input, the same bytes
        assert all(again[k].tobytes() == b[k].tobytes() for k in again)
        assert all(fe.map_match_seconds(q).tobytes() == rb[q]["dist2"].tobytes() for q in range(3))


def test_chosen_first_and_second_neighbours(rig, oracle):
    det, fe = rig
    c = M.placement_case(det)
    m, pts, fr = c["map_rows"], c["map_pts"], (c["rows"], c["xy"])
    _put(fe, det, 0, *fr)
    fe.stage_map(m, pts)
    names = c["names"]
    for mode in (1, 2):
        out, refs, _ = _call(fe, m, pts, [fr], [0], f"{det} placements", mode)
        pi, ki, d, _ = fe.map_matches(0); d2 = fe.map_match_seconds(0)
        kept = dict(zip(ki.tolist(), zip(pi.tolist(), d.tolist(), d2.tolist())))
        for i, name in enumerate(names):
            first, seconds, a, b = M.PLACEMENTS[name]
            if "tie for nearest" in name or name == "bound: 3 against 4":
                assert i not in kept, (mode, name)                         # n.distance == m.distance; 3 < 0.75 * 4 is false
            else:
                assert kept[i] == (first, float(a), float(b)), (mode, name)
        i, j, row = M.SHARED
        assert kept[j][0] == row and ((kept[i][0] == row) if mode == 1 else (i not in kept))   # mode 1: two keypoints keep map row 32
        # the distance bound on top: 3.0 turns the (3, 5) row away, the (3, 4) row is the ratio's
        out, refs, _ = _call(fe, m, pts, [fr], [0], f"{det} placements, max_distance 3", mode, max_distance=3.0)
        assert names.index("bound: 3 against 5") in kept and names.index("bound: 3 against 5") not in refs[0]["qi"]
        assert len(refs[0]["qi"]) == len(kept) - 1
    # a tie for nearest is kept by a ratio above 1 only: the lower index, n.distance == m.distance
    _call(fe, m, pts, [fr], [0], f"{det} placements, ratio 1", 1, ratio=1.0)
    assert not any(names.index(n) in fe.map_matches(0)[1] for n in names if "tie for nearest" in n)
    _call(fe, m, pts, [fr], [0], f"{det} placements, ratio 1.5", 1, ratio=1.5)
    pi, ki, d, _ = fe.map_matches(0); d2 = fe.map_match_seconds(0)
    for n in names:
        if "tie for nearest" in n:
            first, seconds, _, _ = M.PLACEMENTS[n]
            at = ki == names.index(n)
            assert pi[at].tolist() == [min(first, *seconds)] and d[at].tolist() == d2[at].tolist() == [1.0]


def test_stale_rows_past_either_end_are_neither_first_nor_second(rig, oracle):
    """A map staged after a larger one whose rows 5 .. carry the frame's rows exactly; a slot that held a fuller frame whose rows
    17 .. carry the map's rows exactly: either would come first (or second) at distance 0 if a kernel read past the counts."""
    det, fe = rig
    big, big_pts = R.match_map_rows(det, 257)
    rng = np.random.default_rng(5)
    small = R.rand_rows(rng, 5, det); small_pts = rng.uniform(-2, 2, (5, 3)) + [0, 0, 6]
    frame = big[100:117].copy(); xy = rng.uniform(0, 600, (17, 2)).astype(np.float32)
    for k in range(0, 17, 2):                                              # ... half of them a move away from a row of the small map: kept there
        frame[k] = M.move(small[k % 5], (k,), det)
    full = np.concatenate([R.rand_rows(rng, 17, det), np.tile(small, (57, 1))])[:300]
    _put(fe, det, 0, full, rng.uniform(0, 600, (300, 2)).astype(np.float32))
    _put(fe, det, 0, frame, xy)                                            # rows 17 .. 299 of the slot still hold copies of the small map's rows
    for mode in (1, 2):
        fe.stage_map(big, big_pts)
        out, refs, _ = _call(fe, big, big_pts, [(frame, xy)], [0], "big map", mode)
        assert refs[0]["n_match"] >= 6 and not refs[0]["dist"].any()      # the untouched rows find their own row at distance 0
        fe.stage_map(small, small_pts)                                     # rows 5 .. 256 of the image still hold the big map
        out, refs, _ = _call(fe, small, small_pts, [(frame, xy)], [0], "small map after the big one", mode)
        assert refs[0]["n_match"] >= (5 if mode == 1 else 3) and refs[0]["dist"].all() and (refs[0]["dist2"] > 2).all()


def test_a_long_map_with_the_neighbours_at_its_ends(rig, oracle):
    det, fe = rig
    c = M.long_map_case(det)
    _put(fe, det, 0, c["rows"], c["xy"])
    fe.stage_map(c["map_rows"], c["map_pts"])
    for mode in (1, 2):
        out, refs, _ = _call(fe, c["map_rows"], c["map_pts"], [(c["rows"], c["xy"])], [0], "long map", mode)
        pi, ki, d, _ = fe.map_matches(0)
        assert ki.tolist() == [0, 1] and pi.tolist() == [65535, 0] and d.tolist() == [1, 1]
        assert fe.map_match_seconds(0).tolist() == ([2, 2] if det == "sift" else [4, 4])


# ------------------------------------------------------------------ pose
def test_known_pose_and_the_one_row_map(rig, oracle):
    det, fe = rig
    c = R.pose_case(det)
    _put(fe, det, 1, c["rows"], c["xy"])
    for mode in (1, 2):
        fe.stage_map(c["map_rows"], c["map_pts"])
        out, refs, (st, rvec, tvec, bmask, ninl) = _call(fe, c["map_rows"], c["map_pts"], [(c["rows"], c["xy"])], [1], "pose", mode)
        r = M.relocalize(c["map_pts"], c["map_rows"], c["xy"], c["rows"], M.K, mode)
        assert st[0] == r["status"] == 0 and out["n_match"][0] == 200 and ninl[0] == r["n_inl"] == 180 and np.array_equal(bmask, r["mask"])
        assert np.abs(rvec[0] - r["rvec"]).max() < POSE_TOL and np.abs(tvec[0] - r["tvec"]).max() < POSE_TOL
        assert np.array_equal(fe.map_matches(0)[3] > 0, ~c["wrong"])
        fe.stage_map(c["map_rows"][:1], c["map_pts"][:1])
        out, refs, _ = _call(fe, c["map_rows"][:1], c["map_pts"][:1], [(c["rows"], c["xy"])], [1], "one row", mode)
        assert out["status"][0] == M.VO_ERR_TOO_FEW and out["n_match"][0] == 0 and not out["poses"].any()
    assert fe.relocalize([1], M.K)["n_match"][0] == 1                      # (the cross-check does match a map of one row)


def test_the_host_array_convenience_takes_the_mode(oracle):
    from visual_odometry_amd import _lib, geometry
    ctx = _lib.Context(0)
    try:
        for det in ("sift", "orb"):
            c = M.placement_case(det)
            got = geometry.relocalize(c["map_pts"], c["map_rows"], c["xy"], c["rows"], M.K, ctx=ctx, match="ratio", ratio=M.RATIO)
            qi, ti, d, d2 = M.match(c["rows"], c["map_rows"], 1)
            pi, ki, gd, _ = got["matches"]
            assert got["n_match"] == len(qi) > 10 and np.array_equal(pi, ti) and np.array_equal(ki, qi) and np.array_equal(gd, d)
            assert np.array_equal(got["seconds"], d2)
    finally:
        ctx.close()


# ------------------------------------------------------------------ two maps
def _acall(fe, map_rows, map_pts, queries, max_error, what, mode, ratio=M.RATIO, **opts):
    from visual_odometry_amd import geometry
    off = np.concatenate([[0], np.cumsum([len(r) for r, _ in queries])]).astype(np.int32)
    rows = np.concatenate([r for r, _ in queries]); pts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for _, p in queries])
    out = fe.align_maps(rows, pts, max_error, offsets=off, match=MODES[mode], ratio=ratio, **opts)
    refs = []
    for q, (qr, qp) in enumerate(queries):
        bi, ai, d, d2 = M.match(qr, map_rows, mode, ratio, opts.get("max_distance", 0.0))
        refs.append(dict(bi=bi, ai=ai, dist=d, dist2=d2, src=np.asarray(qp, np.float64).reshape(-1, 3)[bi], dst=np.asarray(map_pts, np.float64)[ai]))
        ga, gb, gd, _ = fe.map_align_matches(q)
        g2 = fe.map_align_match_seconds(q)
        print(what, "mode", mode, "q", q, "rows", len(qr), "n_match", int(out["n_match"][q]), "reference", len(bi), "status", int(out["status"][q]))
        assert out["n_match"][q] == len(bi) == len(ga) == len(g2), (what, mode, q)
        assert np.array_equal(gb, bi) and np.array_equal(ga, ai), (what, mode, q)
        assert gd.dtype == g2.dtype == np.float32 and np.array_equal(gd, d) and np.array_equal(g2, d2), (what, mode, q)
    moff = np.concatenate([[0], np.cumsum([len(r["bi"]) for r in refs])]).astype(np.int32)
    want = geometry.estimate_similarity_batch(np.concatenate([r["src"] for r in refs]).reshape(-1, 3), np.concatenate([r["dst"] for r in refs]).reshape(-1, 3),
                                              moff, max_error, ctx=fe.ctx)
    for key in ("scale", "R", "t", "n_inl", "status"):
        assert out[key].tobytes() == want[key].tobytes(), (what, mode, key)
    for q in range(len(queries)):
        assert fe.map_align_matches(q)[3].tobytes() == want["mask"][moff[q]:moff[q + 1]].tobytes(), (what, mode, q)
    return out, refs


def test_align_maps_lists_seconds_and_models(rig, oracle):
    det, fe = rig
    for npt in M.ALIGN_MAPS:
        m, mp, qs, distracted, big = M.align_call(det, npt)
        fe.stage_map(m, mp)
        zero = fe.align_maps(qs[257][0], qs[257][1], big["max_error"])
        zero_m = fe.map_align_matches(0)
        for mode in (1, 2):
            a, ra = _acall(fe, m, mp, [qs[n] for n in (257, 0, 65)], big["max_error"], f"{det} npt {npt} a", mode)
            b, _ = _acall(fe, m, mp, [qs[n] for n in (64, 1, 2, 3)], big["max_error"], f"{det} npt {npt} b", mode)
            assert a["status"][1] == M.VO_ERR_TOO_FEW and a["n_match"][1] == 0
            if npt >= 257:
                assert a["status"][0] == 0 and a["n_inl"][0] >= 10
                assert all(i in zero_m[1] and i not in ra[0]["bi"] for i in distracted)        # the cross-check keeps them, the rule does not
                assert a["n_match"][0] < zero["n_match"][0] or mode == 1
            again = fe.align_maps(np.concatenate([qs[n][0] for n in (64, 1, 2, 3)]), np.concatenate([qs[n][1] for n in (64, 1, 2, 3)]), big["max_error"],
                                  offsets=[0, 64, 65, 67, 70], match=MODES[mode], ratio=M.RATIO)
            assert all(again[k].tobytes() == b[k].tobytes() for k in again)
        after = fe.align_maps(qs[257][0], qs[257][1], big["max_error"])                       # mode 0 again: the bytes it returned before
        assert all(after[k].tobytes() == zero[k].tobytes() for k in zero)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(fe.map_align_matches(0), zero_m))
        n = C.c_int32(0)
        assert fe.ctx.lib.vo_map_match_seconds(fe.ctx.handle, 1, 0, None, 0, C.addressof(n)) == M.VO_ERR_INVALID


# ------------------------------------------------------------------ the setting
def test_the_setting_leaks_nothing(rig, oracle):
    from visual_odometry_amd import _lib
    det, fe = rig
    m, pts, frames = M.call_frames(det, 257)
    for slot, n in enumerate((300, 17, 1)):
        _put(fe, det, slot, *frames[n])
    fe.stage_map(m, pts)
    lib, h = fe.ctx.lib, fe.ctx.handle
    n = C.c_int32(0)
    before = fe.relocalize([0, 1, 2], M.K); before_m = [fe.map_matches(q) for q in range(3)]
    assert lib.vo_map_match_seconds(h, 0, 0, None, 0, C.addressof(n)) == M.VO_ERR_INVALID     # that call ran in mode 0
    for q, n_rows in enumerate((300, 17, 1)):                              # ... and is what tests/test_gpu_relocalize.py holds it to
        qi, ti, d = R.match_map(frames[n_rows][0], m)
        assert np.array_equal(before_m[q][1], qi) and np.array_equal(before_m[q][0], ti) and np.array_equal(before_m[q][2], d)
    for mode in (1, 2):
        one = fe.relocalize([0, 1, 2], M.K, match=MODES[mode], ratio=M.RATIO)
        assert one["n_match"][0] == len(M.match(frames[300][0], m, mode)[0]) > 0
        assert lib.vo_map_match_seconds(h, 0, 0, None, 0, C.addressof(n)) == 0 and n.value == 0   # cap 0: nothing copied
        assert lib.vo_map_match_seconds(h, 0, 3, None, 0, C.addressof(n)) == M.VO_ERR_INVALID
        assert lib.vo_map_match_seconds(h, 2, 0, None, 0, C.addressof(n)) == M.VO_ERR_INVALID
        after = fe.relocalize([0, 1, 2], M.K)
        assert all(after[k].tobytes() == before[k].tobytes() for k in before)
        assert all(x.tobytes() == y.tobytes() for q in range(3) for x, y in zip(fe.map_matches(q), before_m[q]))
        assert lib.vo_map_match_seconds(h, 0, 0, None, 0, C.addressof(n)) == M.VO_ERR_INVALID
    # the raw setting: a refused call leaves it as it was; it survives a newly staged map; FrontEnd's default argument puts the cross-check back
    fe.ctx.set_map_match("ratio", M.RATIO)
    assert [lib.vo_set_map_match(h, *a) for a in ((3, 0.75), (-1, 0.75), (1, 0.0), (2, float("nan")), (1, float("inf")))] == [M.VO_ERR_INVALID] * 5
    fe.stage_map(m, pts)
    opts = _lib.RelocOpts(0.0, 100, 8.0, 0.99, 0xFFFFFFFFFFFFFFFF, 0)
    sl = np.array([0, 1, 2], np.int32); K = np.ascontiguousarray(M.K); poses = np.zeros((3, 12)); i32 = [np.zeros(3, np.int32) for _ in range(3)]
    assert lib.vo_map_localize(h, sl.ctypes.data, 3, K.ctypes.data, C.addressof(opts), poses.ctypes.data, *[v.ctypes.data for v in i32]) == 0
    assert i32[0][0] == len(M.match(frames[300][0], m, 1)[0]) and np.array_equal(fe.map_match_seconds(0), M.match(frames[300][0], m, 1)[3])
    assert all(fe.relocalize([0, 1, 2], M.K)[k].tobytes() == before[k].tobytes() for k in before)

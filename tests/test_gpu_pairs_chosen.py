"""GPU: the batched geometry tail of vo_pairs_run — k_match_select's gather of px / xn by the match indices, k_ransac, k_pose_prepare ->
k_pose -> k_pose_finish, k_triangulate_pairs — on correspondences the test CHOSE: descriptor rows and keypoint positions go into the
slots through FrontEnd.set_orb_rows / set_sift_rows, built by tests/two_view_cases.py so that the match list is known (slot B is a
permutation of slot A) and every pair is a two-view problem with a known answer.  tests/test_two_view_cases_reference.py holds on the
CPU that each case reaches what it is named for.  The oracle's stages are composed as twoview.oracle_pair_stages composes them.

Compared per pair, for equality: status, n_kp1, n_kp2, n_match, n_inl, n_good, ransac_iters; the match list (qi, ti, dist) and the
inlier mask; for VO_OK pairs E, R, t bit for bit (300-sweep mode against the oracle's 300 sweeps, and the default mode against the
oracle under the kernel's exit rule) and the first n_inl columns of X bit for bit against oracle.triangulate on projection matrices
formed in the kernel's operation order; for failed pairs the whole record as include/vo_hip.h states it.

Cases (tests/two_view_cases.py): 0 .. 4 matches (VO_ERR_TOO_FEW); five matches without a model (VO_ERR_NO_MODEL), with 2 / 4 / 10
stacked models (VO_ERR_AMBIGUOUS) and with exactly one (a normal VO_OK pair of five inliers); ten equal points (no model in any sample:
the iteration counter reaches the budget); scenes whose recoverPose winner is candidate 0, 1, 2, 3 alone, ties 20 : 20 inside each
pair of candidates and 21 : 19 / 19 : 21 splits across it; one scene under the distance thresholds 50, 9, 8, 7, 1; inlier counts
255, 256, 257, 511, 512, 513, kp_cap = 768 and front / behind halves 256 + 256, 257 + 256 (k_pose's blocks of 256); 63, 64, 65 matches
with 30 % outliers; fy = 1.07 fx.  Launches hold failed pairs between good ones, B == max_pairs, the list reversed; a second launch
on the same front end swaps failed and good pairs and rewrites the slots with fewer rows; one launch runs on SIFT rows (the L2 select).
The single-call twins geometry.recoverPose (k_pose_finish's mask branch, all four winners) and geometry.triangulatePoints (1, 63, 64,
65 points, zero parallax among them) are held to the oracle in the same way.

Defect found by this file: k_ransac's five-match branch set all five mask bytes of a pair WITHOUT a model (VO_ERR_NO_MODEL), where the
oracle and the kernel's own M > 5 branch leave none set; the bytes are now written with the model count.

The frame is 64 x 64 with one pyramid level (SIFT: 32 x 32), kp_cap 264 (768 for the block edges, 256 for SIFT).
The whole file takes 1.0 - 1.1 s on an MI355X (measured, two runs, the oracle's side included): the seven launches of 20 pairs 0.37 s,
every other test under 0.1 s."""
import numpy as np
import pytest

import two_view_cases as T
from test_gpu_chain import _KP, _inv_pose

pytestmark = pytest.mark.gpu

H = W = 64
INT_FIELDS = ("status", "n_kp1", "n_kp2", "n_match", "n_inl", "n_good", "ransac_iters")


def _c(*names):
    return [T.cases()[n] for n in names]


def _k60_launch():
    """Every K60 case of the winner / tie / threshold groups, the pairs without enough matches between them: 20 pairs."""
    good = [c for c in T.group("winner", "tie", "threshold") if c.K is T.K60]
    few = _c("few_0", "few_1", "few_2", "few_3", "few_4")
    assert len(good) == 15
    out = []
    for i, c in enumerate(good):
        out.append(c)
        if i % 3 == 0:
            out.append(few[i // 3])
    return out


def _k8_launch():
    """Every structured case beside good pairs under the same camera; shifted by one place, failed and good pairs change places."""
    return _c("k8_winner2", "five_degree_9_and_skipped_root", "k8_winner3", "five_rank_deficient_null_space", "five_degree_9_one_real_root",
              "ten_equal_points", "k8_winner2", "few_3", "k8_winner3", "five_degree_8", "five_degree_9_one_real_root", "five_zero_pivot",
              "k8_winner2", "five_ten_nan_models", "k8_winner3", "five_zero_pivot_all_zero")


def _front_end(nfeatures, n_pairs, detector="orb"):
    from visual_odometry_amd.frontend import FrontEnd
    if detector == "sift":
        fe = FrontEnd(32, 32, max_frames=2 * n_pairs, max_pairs=n_pairs, detector="sift", kp_cap=256)
        assert fe.kp_cap == 256
    else:
        fe = FrontEnd(H, W, max_frames=2 * n_pairs, max_pairs=n_pairs, nfeatures=nfeatures, nlevels=1)
        assert fe.kp_cap == T.HR.kp_cap_for(nfeatures)
    return fe


def _launch(fe, O, cases, K, dist=50.0, max_iters=1000):
    """Pair p takes slots 2 p and 2 p + 1, rewritten for its case; ONE run_pairs call holds all of `cases`, with want_points.
    Returns copies: (records, X, [pair_matches(p)])."""
    put = fe.set_orb_rows if fe.detector == "orb" else fe.set_sift_rows
    for p, c in enumerate(cases):
        assert c.M < 5 or np.array_equal(c.K, K), c.name          # fewer than five matches: K does not enter
        rows1, xy1, rows2, xy2, _, _ = T.slots(O, c, fe.detector)
        put(2 * p, rows1, xy1)
        put(2 * p + 1, rows2, xy2)
    opts = fe.make_opts(max_iters=max_iters, dist_thresh=dist, want_points=True)
    res, X = fe.run_pairs([[2 * p, 2 * p + 1] for p in range(len(cases))], K, opts, want_points=True)
    assert X is not None and X.shape == (len(cases), 4, fe.kp_cap)
    return res.copy(), X.copy(), [fe.pair_matches(p) for p in range(len(cases))]


def _same(O, fe, out, cases, dist=50.0, max_iters=1000, what=""):
    from visual_odometry_amd import _lib
    assert (T.VO_OK, T.VO_ERR_TOO_FEW, T.VO_ERR_NO_MODEL, T.VO_ERR_AMBIGUOUS) == (_lib.VO_OK, _lib.VO_ERR_TOO_FEW, _lib.VO_ERR_NO_MODEL, _lib.VO_ERR_AMBIGUOUS)
    res, X, matches = out
    for p, c in enumerate(cases):
        tag = (what, p, c.name, dist)
        e = T.expected(O, c, dist, max_iters)
        _, _, _, _, qi, ti = T.slots(O, c, fe.detector)
        r = res[p]
        got = {k: int(r[k]) for k in INT_FIELDS}
        want = dict(status=e["status"], n_kp1=c.M, n_kp2=c.M, n_match=c.M, n_inl=e["n_inl"], n_good=e["n_good"], ransac_iters=e["ransac_iters"])
        print(tag, got)
        assert got == want, tag
        q, t, d, m = matches[p]
        assert np.array_equal(q, qi) and np.array_equal(t, ti), tag
        assert d.dtype == np.float32 and len(d) == c.M and not d.any(), tag
        assert np.array_equal(m, e["mask"]), tag
        E, R, tt = r["E"].reshape(3, 3), r["R"].reshape(3, 3), r["t"].reshape(3, 1)
        if e["status"] == T.VO_OK:
            assert np.array_equal(E, e["E"]), tag
            assert np.array_equal(R, e["R"]) and np.array_equal(tt, e["t"]), tag
            n = e["n_inl"]
            inl = e["mask"] > 0
            p1, p2 = c.p1.astype(np.float64)[inl], c.p2.astype(np.float64)[inl]
            ref = O.triangulate(_KP(c.K, _inv_pose(R, tt)), _KP(c.K, np.eye(3, 4)), p1.T, p2.T)
            with np.errstate(all="ignore"):
                ref = ref / ref[3]
            assert np.array_equal(ref, e["X"], equal_nan=True)
            assert np.array_equal(X[p][:, :n], ref, equal_nan=True), (tag, np.abs(X[p][:, :n] - ref).max())
        elif e["status"] == T.VO_ERR_AMBIGUOUS:
            assert np.array_equal(E, e["models"][0], equal_nan=True) and not R.any() and not tt.any(), tag
        else:
            assert not E.any() and not R.any() and not tt.any(), tag


def _identical(a, b, cases):
    """Two launches of one list left the same bytes: records, match lists, masks, and X where it is valid."""
    assert a[0].tobytes() == b[0].tobytes()
    for p in range(len(cases)):
        for u, v in zip(a[2][p], b[2][p]):
            assert u.tobytes() == v.tobytes()
        n = int(a[0][p]["n_inl"]) if int(a[0][p]["status"]) == T.VO_OK else 0
        assert a[1][p][:, :n].tobytes() == b[1][p][:, :n].tobytes()


@pytest.fixture
def faithful(oracle):
    assert not oracle.get_dk_early_exit()
    return oracle


# ------------------------------------------------------------------ the batched tail
def test_winners_ties_and_too_few_side_by_side(faithful):
    """20 pairs == max_pairs; the list forwards and reversed; the distance thresholds (one per launch) on every scene."""
    cases = _k60_launch()
    fe = _front_end(8, len(cases))
    try:
        fe.ctx.set_poly_solver("opencv300")
        assert fe.kp_cap == 264 and fe.max_pairs == len(cases) == 20
        _same(faithful, fe, _launch(fe, faithful, cases, T.K60), cases, what="forward")
        back = cases[::-1]
        _same(faithful, fe, _launch(fe, faithful, back, T.K60), back, what="reversed")
        for dist in T.DIST_THRESHOLDS[1:]:
            _same(faithful, fe, _launch(fe, faithful, cases, T.K60, dist=dist), cases, dist=dist, what="threshold")
    finally:
        fe.ctx.close()


def test_winners_and_ties_in_the_default_mode(kernel_dk_rule):
    """The product's default root finder against the oracle under the same exit rule, bit for bit (tests/test_gpu_geometry.py)."""
    cases = _k60_launch()
    fe = _front_end(8, len(cases))
    try:
        fe.ctx.set_poly_solver("fast")
        _same(kernel_dk_rule, fe, _launch(fe, kernel_dk_rule, cases, T.K60), cases, what="fast")
    finally:
        fe.ctx.close()


def test_five_matches_and_no_state_between_launches(faithful):
    """The structured five-match cases and the ten equal points beside good pairs; then the list shifted by one place on the SAME
    front end — TOO_FEW, AMBIGUOUS and NO_MODEL pairs at the indices that held good pairs and good pairs where failed ones were,
    slots rewritten with fewer rows than before — then the first list again, which leaves the bytes of its first run."""
    cases = _k8_launch()
    shifted = cases[-1:] + cases[:-1]
    ok = [T.expected(faithful, c, max_iters=100)["status"] == T.VO_OK for c in cases]
    swapped = [(a, b) for a, b in zip(ok, ok[-1:] + ok[:-1]) if a != b]
    assert (True, False) in swapped and (False, True) in swapped
    for status in (T.VO_ERR_TOO_FEW, T.VO_ERR_AMBIGUOUS, T.VO_ERR_NO_MODEL):     # each at an index that held a good pair
        assert any(ok[p] and T.expected(faithful, shifted[p], max_iters=100)["status"] == status for p in range(len(cases))), status
    assert any(shifted[p].M < cases[p].M for p in range(len(cases)))
    fe = _front_end(8, len(cases))
    try:
        fe.ctx.set_poly_solver("opencv300")
        first = _launch(fe, faithful, cases, T.K8, max_iters=100)
        _same(faithful, fe, first, cases, max_iters=100, what="first")
        second = _launch(fe, faithful, shifted, T.K8, max_iters=100)
        _same(faithful, fe, second, shifted, max_iters=100, what="shifted")
        again = _launch(fe, faithful, cases, T.K8, max_iters=100)
        _same(faithful, fe, again, cases, max_iters=100, what="again")
        _identical(first, again, cases)
        back = cases[::-1]
        _same(faithful, fe, _launch(fe, faithful, back, T.K8, max_iters=100), back, max_iters=100, what="reversed")
    finally:
        fe.ctx.close()


def test_block_and_capacity_edges_of_the_pose_kernels(faithful):
    """n_inl on both sides of k_pose's blocks of 256 and at kp_cap; the candidates' counts coming from different blocks."""
    b = {c.name: c for c in T.group("block")}
    cases = [b["block_255"], T.cases()["few_1"], b["block_256"], b["block_257"], T.cases()["few_0"], b["block_511"], b["block_512"],
             b["block_513"], T.cases()["few_4"], b[f"block_{T.BLOCK_KP_CAP}"], b["block_256_256"], b["block_257_256"]]
    assert len(cases) == len(b) + 3
    fe = _front_end(512, len(cases))
    try:
        fe.ctx.set_poly_solver("opencv300")
        assert fe.kp_cap == T.BLOCK_KP_CAP >= 768
        _same(faithful, fe, _launch(fe, faithful, cases, T.K60), cases, what="forward")
        back = cases[::-1]
        _same(faithful, fe, _launch(fe, faithful, back, T.K60), back, what="reversed")
    finally:
        fe.ctx.close()


def test_wave_edges_of_the_scoring_and_non_square_pixels(faithful):
    waves = [T.cases()["wave_63"], T.cases()["few_2"], T.cases()["wave_64"], T.cases()["wave_65"]]
    other = [T.cases()["non_square"], T.cases()["few_4"], T.cases()["non_square"]]
    fe = _front_end(8, len(waves))
    try:
        fe.ctx.set_poly_solver("opencv300")
        _same(faithful, fe, _launch(fe, faithful, waves, T.K_SCENE), waves, what="waves")
        _same(faithful, fe, _launch(fe, faithful, other, T.K_NONSQUARE), other, what="non-square")
        _same(faithful, fe, _launch(fe, faithful, waves[::-1], T.K_SCENE), waves[::-1], what="waves reversed")
    finally:
        fe.ctx.close()


def test_sift_rows_feed_the_same_tail(faithful):
    """The L2 select (k_nn_l2i8 -> k_match_select with square-rooted distances) gathers for the same geometry kernels."""
    cases = _c("k64_winner3", "five_degree_8_k64", "k64_tie_second_pair")
    fe = _front_end(0, len(cases), detector="sift")
    try:
        fe.ctx.set_poly_solver("opencv300")
        assert any(np.abs(c.p1 - np.rint(c.p1)).max() > 0.01 for c in cases)      # sub-pixel positions
        _same(faithful, fe, _launch(fe, faithful, cases, T.K64), cases, what="sift")
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ the single-call twins
def test_recover_pose_single_call_every_winner(faithful, ctx):
    """geometry.recoverPose on the oracle's E and inliers: the pose_mask branch of k_pose_finish for all four winners, the ties and the
    distance thresholds; the front / behind halves across k_pose's blocks as well."""
    from visual_odometry_amd import geometry
    cases = T.group("winner", "tie", "threshold") + _c("block_256_256", "block_257_256")
    assert {c.want["best"] for c in cases} == {0, 1, 2, 3}
    for c in cases:
        for dist in (T.DIST_THRESHOLDS if c.group == "threshold" else (50.0,)):
            e = T.expected(faithful, c, dist)
            ng, R, t, pm = faithful.recover_pose(e["E"], e["q1"], e["q2"], c.K, dist)
            n, R2, t2, m2 = geometry.recoverPose(e["E"], e["q1"], e["q2"], c.K, dist, ctx=ctx)
            print(c.name, dist, n, ng, e["best"])
            assert n == ng == e["n_good"], (c.name, dist)
            assert np.array_equal(R2, R) and np.array_equal(t2, t), (c.name, dist)
            assert m2.dtype == np.uint8 and np.array_equal(m2.ravel(), pm), (c.name, dist)
            assert int((m2 > 0).sum()) == n


@pytest.mark.parametrize("M", [1, 63, 64, 65])
def test_triangulate_points_single_call(faithful, ctx, M):
    """The un-normalised 4 x M output bit for bit, a NaN equal to a NaN.  Columns with the same projection in both views, under
    cameras that differ (no parallax along that ray) and under twice the same camera (no parallax at all), are among them."""
    from visual_odometry_amd import geometry
    c = T.cases()["block_257"]
    e = T.expected(faithful, c)
    assert len(e["q1"]) >= M
    P1, P2 = _KP(c.K, _inv_pose(e["R"], e["t"])), _KP(c.K, np.eye(3, 4))
    x1, x2 = e["q1"][:M].T.copy(), e["q2"][:M].T.copy()
    if M > 1:
        x2[:, -2:] = x1[:, -2:]
    for A, B in ((P1, P2), (P2, P2)) if M > 1 else ((P1, P2),):
        ref = faithful.triangulate(A, B, x1, x2)
        got = geometry.triangulatePoints(A, B, x1, x2, ctx=ctx)
        assert got.shape == ref.shape == (4, M)
        assert np.array_equal(got, ref, equal_nan=True), (M, np.abs(got - ref).max())

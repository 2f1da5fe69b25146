"""GPU: vo_pairs_epipolar (k_pairs_epipolar) on what vo_pairs_run left on the device, against the numpy checker applied to the same
pair's downloads — fe.pair_matches (match list, inlier mask), the keypoint positions and res["E"] — byte for byte: the distances, and
the sequential mean / std / max.

Detected pairs: the small pair shape of the geometry tests, 320 x 240, 4 frames, 3 pairs.  Chosen pairs (set_orb_rows, rows and
positions of tests/two_view_cases.py): pairs that fail (too few matches, no model, stacked models) between good ones, and a pair of
exactly five inliers.  A VO_OK pair with exactly ONE inlier is not reachable: a pair needs five matches to get a model
(VO_ERR_TOO_FEW below that), and the model is kept with its own inlier count only if RANSAC found one, which for an essential
matrix fitted to five matches counts those five; the one-inlier rule (std = 0) is held on the checker in
tests/test_epilines_reference.py."""
import numpy as np
import pytest

import epilines_reference as ER
import two_view_cases as T

pytestmark = pytest.mark.gpu


def _check(fe, res, K, positions, stats):
    """positions(p) -> (xy of the pair's first slot, xy of its second slot), float32 rows indexed by keypoint."""
    assert stats["dist"] is not None
    for p in range(len(res)):
        qi, ti, _, mask = fe.pair_matches(p)
        xy1, xy2 = positions(p)
        inl = mask > 0
        x1 = xy1[qi[inl]].astype(np.float64); x2 = xy2[ti[inl]].astype(np.float64)
        status = int(res[p]["status"])
        want = ER.pairs_epipolar(x1 if status == 0 else x1[:0], x2 if status == 0 else x2[:0], res[p]["E"], K, status)
        if status == 0:
            assert want["n"] == int(res[p]["n_inl"]) == int(inl.sum())
        got = {k: stats[k][p] for k in ("n", "mean", "std", "max")}
        print(p, status, got)
        assert int(got["n"]) == want["n"], p
        for k in ("mean", "std", "max"):
            assert np.array_equal(np.float64(got[k]), np.float64(want[k])), (p, k, got[k], want[k])
        assert stats["dist"][p].shape == (want["n"],) and np.array_equal(stats["dist"][p], want["dist"]), p
    return stats


def test_detected_pairs():
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    seq = synth.sequence(4, 320, 240, cache_dir="/tmp", workers=1)
    K = seq["K"]
    fe = FrontEnd(240, 320, max_frames=4, max_pairs=3, nfeatures=500, nlevels=8)
    try:
        _detected_pairs(fe, seq, K)
    finally:
        fe.ctx.close()


def _detected_pairs(fe, seq, K):
    from visual_odometry_amd.frontend import FrontEnd
    fe.upload(seq["frames"]); fe.detect(0, 4)
    pairs = [[0, 1], [1, 2], [2, 3]]
    res, _ = fe.run_pairs(pairs, K)                                      # the run need not triangulate
    res = res.copy()
    assert (res["status"] == 0).all() and (res["n_inl"] > 20).all()
    feats = [fe.features(s)["xy"] for s in range(4)]
    stats = _check(fe, res, K, lambda p: (feats[pairs[p][0]], feats[pairs[p][1]]), fe.epipolar_stats(K, want_dist=True))
    # inliers of a 1-pixel RANSAC threshold lie within about a pixel of their epilines, on each side
    assert (stats["max"] < 4.0).all() and (stats["mean"] > 0).all() and (stats["std"] > 0).all()
    # dist is optional: the same statistics without it
    plain = fe.epipolar_stats(K)
    assert plain["dist"] is None
    for k in ("n", "mean", "std", "max"):
        assert np.array_equal(plain[k], stats[k])
    # sequential sums against numpy's pairwise ones: |difference| <= 2 n u max (one rounding per partial sum)
    for p in range(3):
        d = stats["dist"][p]
        tol = len(d) * np.finfo(np.float64).eps * d.max()
        assert abs(stats["mean"][p] - np.mean(d)) <= tol and abs(stats["std"][p] - np.std(d)) <= tol

    # refusals, as vo_tracks_pnp_batch: another B than the run's; K shapes the pair path would read differently
    from visual_odometry_amd import _lib
    for B in (2, 4, 0):
        with pytest.raises(_lib.VoError) as e:
            fe.epipolar_stats(K, n_pairs=B)
        assert e.value.code == _lib.VO_ERR_INVALID
    for r, c, v in ((0, 1, 0.5), (2, 2, 2.0), (2, 0, 1e-3), (0, 0, 0.0), (1, 1, np.nan)):
        Kb = K.copy(); Kb[r, c] = v
        assert not ER.k_supported(Kb)
        with pytest.raises(NotImplementedError):
            fe.epipolar_stats(Kb)
    assert np.array_equal(fe.epipolar_stats(K)["mean"], stats["mean"])   # a refused call changes nothing
    # a configure call in between: the run is forgotten
    fe2 = FrontEnd(240, 320, max_frames=4, max_pairs=3, nfeatures=500, nlevels=8, ctx=fe.ctx)
    with pytest.raises(_lib.VoError) as e:
        fe2.epipolar_stats(K, n_pairs=3)
    assert e.value.code == _lib.VO_ERR_INVALID


def test_chosen_pairs_with_failures(oracle):
    from test_gpu_pairs_chosen import _front_end, _launch
    names = ("k8_winner2", "few_3", "five_degree_9_one_real_root", "five_zero_pivot", "k8_winner3", "five_degree_8", "few_0", "ten_equal_points",
             "five_rank_deficient_null_space", "k8_winner2")
    cases = [T.cases()[n] for n in names]
    fe = _front_end(8, len(cases))
    try:
        fe.ctx.set_poly_solver("opencv300")          # the structured five-match cases are built for cv::solvePoly's 300 sweeps
        res, _, _ = _launch(fe, oracle, cases, T.K8, max_iters=100)
        status = [int(s) for s in res["status"]]
        print(list(zip(names, status, res["n_inl"].tolist())))
        assert status.count(0) >= 3 and T.VO_ERR_TOO_FEW in status and len(set(status) - {0, T.VO_ERR_TOO_FEW}) >= 1
        assert any(s == 0 and int(n) == 5 for s, n in zip(status, res["n_inl"]))          # a pair of exactly five inliers
        sl = [T.slots(oracle, c, "orb") for c in cases]
        stats = _check(fe, res, T.K8, lambda p: (sl[p][1], sl[p][3]), fe.epipolar_stats(T.K8, want_dist=True))
        for p, s in enumerate(status):
            if s != 0:
                assert (stats["n"][p], stats["mean"][p], stats["std"][p], stats["max"][p]) == (0, 0.0, 0.0, 0.0) and len(stats["dist"][p]) == 0
            else:
                assert stats["n"][p] == res["n_inl"][p] > 0
    finally:
        fe.ctx.close()

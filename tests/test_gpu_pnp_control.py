"""GPU: the control flow of k_pnp_ransac — which five indices each sample draws, from which of the three sources of the random
stream (the 448 numbers staged per round, the 8192-entry table, the generator re-run from the seed), how many samples the
adaptive bound lets it consume inside rounds of 64 scored four at a time, and what iterations / reproj_err / confidence / seed
do — against the CPU oracle, on the cases that tests/test_pnp_control_reference.py picks and pins on the CPU.

The kernel reports no iteration count; it is inferred from budgets, as in tests/test_gpu_ransac_quad.py: with budget b the
first b samples are all that can be seen, so a result that equals the oracle's for b = first accepted sample - 1 (no model),
that sample and the next pins the sample sequence, and one that equals the oracle's for stop - 1, stop, stop + 1 and for budgets
on both sides of every round boundary pins the stop rule.

Tolerances are those of tests/test_gpu_pnp.py: status, mask and n_inl exact, the pose within POSE_TOL = 1e-7 in cv2 mode and
within 1e-9 in fast mode."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_control as P  # noqa: E402
import test_pnp_control_reference as C  # noqa: E402
from test_gpu_pnp import K, POSE_TOL, problem  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"cv2": POSE_TOL, "fast": 1e-9}
CONFIDENCES = (0.5, 0.9, 0.99, 0.999, 0.999999)
CHAIN_PNP = C.CHAIN_PNP


@pytest.fixture()
def refine_modes(oracle, ctx):
    def set_mode(m):
        oracle.set_pnp_refine(m); ctx.set_pnp_refine(m)
    yield set_mode
    set_mode("cv2")


def _device(X, uv, iterations=100, reproj_err=8.0, confidence=0.99, seed=P.DEFAULT_SEED, ctx=None):
    """One problem through the batched entry, which reports the kernel's status as it is -> (status, rvec, tvec, mask, n_inl)."""
    from visual_odometry_amd import geometry
    st, rv, tv, mask, ninl = geometry.solve_pnp_ransac_batch(X, uv, np.array([0, len(X)], np.int32), K, iterations, reproj_err,
                                                             confidence, seed, ctx=ctx)
    return int(st[0]), rv[0], tv[0], mask, int(ninl[0])


def _check(oracle, X, uv, tol, what, ctx=None, **opts):
    """The device's verdict, mask, inlier count and pose against the oracle's under the same options; returns the oracle's."""
    ref = oracle.solve_pnp_ransac(X, uv, K, **opts)
    got = _device(X, uv, ctx=ctx, **opts)
    assert got[0] == ref[0], (what, got[0], ref[0])
    assert got[4] == ref[4] and np.array_equal(got[3], ref[3]), (what, got[4], ref[4])
    if ref[0] == 0:
        err = max(np.abs(got[1] - ref[1]).max(), np.abs(got[2] - ref[2]).max())
        assert err < tol, (what, err)
    else:
        assert not got[3].any(), what
    return ref


# ---------------------------------------------------------------------------------------------- sample sequence
@pytest.mark.parametrize("name", list(C.LATE_CASES))
def test_sample_sequence_by_first_acceptance(oracle, ctx, name):
    from visual_odometry_amd import geometry
    c, f = C.late_case(name), C.late_facts(oracle, name)
    X, uv, o = c["X"], c["uv"], c["opts"]
    first = f["first"]
    if c["kind"] == "no_model":
        assert first is None
        for b in (1, 64, 65, c["budget"]):
            ok, _, _, inl = geometry.solvePnPRansac(X, uv, K, None, iterationsCount=b, reprojectionError=o["reproj_err"], confidence=o["confidence"], seed=o["seed"])
            assert not ok and inl is None, b
            assert _check(oracle, X, uv, POSE_TOL, (name, b), iterations=b, **o)[0] == -4
        return
    ok, _, _, inl = geometry.solvePnPRansac(X, uv, K, None, iterationsCount=first - 1, reprojectionError=o["reproj_err"], confidence=o["confidence"], seed=o["seed"])
    assert not ok and inl is None                                         # one sample less: no model
    assert _check(oracle, X, uv, POSE_TOL, (name, first - 1), iterations=first - 1, **o)[0] == -4
    for b in (first, first + 1, c["budget"]):
        ref = oracle.solve_pnp_ransac(X, uv, K, iterations=b, **o)
        ok, rvec, tvec, inl = geometry.solvePnPRansac(X, uv, K, None, iterationsCount=b, reprojectionError=o["reproj_err"], confidence=o["confidence"], seed=o["seed"])
        assert ok and ref[0] == 0 and inl.ravel().tolist() == np.nonzero(ref[3])[0].tolist() == sorted(c["good"]), (name, b)
        assert np.abs(rvec.ravel() - ref[1]).max() < POSE_TOL and np.abs(tvec.ravel() - ref[2]).max() < POSE_TOL, (name, b)


# ---------------------------------------------------------------------------------------------- stop rule
@pytest.mark.parametrize("mode", ["cv2", "fast"])
@pytest.mark.parametrize("name", list(C.STOP_CASES))
def test_stop_rule_by_budgets(oracle, ctx, refine_modes, name, mode):
    c, f = C.stop_case(name), C.stop_facts(oracle, name)
    stop = f["stop"]
    assert c["kinds"] <= f["kinds"]
    refine_modes(mode)
    seen = set()
    for b in (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, stop - 1, stop, stop + 1, c["budget"]):
        ref = _check(oracle, c["X"], c["uv"], TOL[mode], (name, mode, b), iterations=b, confidence=c["confidence"], **c["opts"])
        seen.add((ref[0], ref[4]))
    assert len(seen) >= 3                                                 # the budgets do show different states of the run
    if "unused_hypothesis" in c["kinds"]:                                 # run on, the round of the stop ends with another model
        more = _check(oracle, c["X"], c["uv"], TOL[mode], (name, mode, "no stop"), iterations=f["round_end"], confidence=P.NO_STOP, **c["opts"])
        last = oracle.solve_pnp_ransac(c["X"], c["uv"], K, iterations=c["budget"], confidence=c["confidence"], **c["opts"])
        assert more[4] > last[4]


# ---------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("scene", [(301, 120, 0.4, 1.0), (302, 300, 0.5, 2.0)])
def test_reproj_err_and_confidence(oracle, ctx, scene):
    X, uv, *_ = problem(scene[0], scene[1], scene[2], noise=scene[3])
    counts = {}
    for err in (0.5, 1.0, 3.0, 8.0, 20.0):
        for conf in CONFIDENCES:
            ref = _check(oracle, X, uv, POSE_TOL, (scene, err, conf), iterations=300, reproj_err=err, confidence=conf)
            counts[(err, conf)] = (ref[0], ref[4])
    assert len({v for (e, _), v in counts.items() if e == 3.0}) >= 2      # the confidence decides where the run stops
    assert len({counts[(e, 0.999999)] for e in (0.5, 1.0, 3.0, 8.0, 20.0)}) >= 4            # and the threshold what is counted


def test_iterations_below_two_run_one_sample(oracle, ctx):
    X, uv, *_ = problem(313, 80, 0.2)
    one = _check(oracle, X, uv, POSE_TOL, 1, iterations=1, reproj_err=8.0)
    assert one[0] == 0                                                    # the first sample has a model here: a result to compare
    for it in (0, -5):
        ref = _check(oracle, X, uv, POSE_TOL, it, iterations=it, reproj_err=8.0)
        assert ref[0] == 0 and np.array_equal(ref[3], one[3]) and np.array_equal(ref[1], one[1])
    two = oracle.solve_pnp_ransac(X, uv, K, iterations=20)
    assert two[4] > one[4]                                                # and one sample is not the whole run
    Xn, uvn = C.late_case("n6_no_model")["X"], C.late_case("n6_no_model")["uv"]
    for it in (1, 0, -5):
        assert _check(oracle, Xn, uvn, POSE_TOL, it, iterations=it, reproj_err=0.5)[0] == -4


def test_confidence_outside_the_open_interval(oracle, ctx):
    from visual_odometry_amd import _lib, geometry
    X, uv, *_ = problem(303, 80, 0.2)
    for conf in (0.0, 1.0, float("nan")):
        ref = _check(oracle, X, uv, POSE_TOL, conf, confidence=conf)
        assert ref[0] == _lib.VO_ERR_INVALID == -1 and ref[4] == 0 and not ref[3].any()
        with pytest.raises(_lib.VoError) as e:
            geometry.solvePnPRansac(X, uv, K, None, confidence=conf)
        assert e.value.code == _lib.VO_ERR_INVALID


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("mode", ["cv2", "fast"])
def test_sizes_around_the_strides(oracle, ctx, refine_modes, mode):
    refine_modes(mode)
    verdicts = []
    for n in C.SIZES:
        X, uv = C.size_case(n)
        ref = _check(oracle, X, uv, TOL[mode], (n, mode), **C.SIZE_OPTS)
        verdicts.append(ref[0])
        if n >= 63:
            assert ref[0] == 0 and 0.5 * n < ref[4] < 0.85 * n, (n, ref[4])
    assert verdicts.count(0) >= 8


@pytest.mark.parametrize("mode", ["cv2", "fast"])
@pytest.mark.parametrize("k,planar", C.CONSENSUS_CASES)
def test_consensus_of_five_six_and_seven(oracle, ctx, refine_modes, k, planar, mode):
    refine_modes(mode)
    X, uv = C.consensus_case(k, planar)
    ref = _check(oracle, X, uv, TOL[mode], (k, planar, mode), **C.CONSENSUS_OPTS)
    assert ref[0] == 0 and ref[4] == k


# ---------------------------------------------------------------------------------------------- one launch
def test_one_launch_every_path(oracle, ctx):
    """Problems that take every exit of the kernel in one launch, with options none of which is a default: each equals its
    single call and the oracle, in both orders; no mask byte outside a problem's rows is written — rows before the first and
    after the last problem belong to no problem, and a neighbour's bytes are its single call's.  Under these options the
    beyond-table problem accepts its first model past the table, and the stop-rule problem stops inside round 1 with a better
    hypothesis of that round left unused: both are asserted from the oracle, so neither can drift off its path unnoticed."""
    from visual_odometry_amd import geometry
    opts = C.BATCH_OPTS
    beyond, stopc = C.late_case("n13_seed_0_beyond"), C.stop_case("low_noise_for_the_batch")
    nomodel = C.late_case("n6_no_model")
    probs = [problem(310 + m, m, 0.0)[:2] for m in (3, 4, 5)] + [(nomodel["X"], nomodel["uv"]), (beyond["X"], beyond["uv"]),
                                                                 (stopc["X"], stopc["uv"]), C.size_case(513)]
    assert beyond["opts"] == {k: opts[k] for k in ("reproj_err", "confidence", "seed")}
    assert C.late_facts(oracle, "n13_seed_0_beyond")["first"] < opts["iterations"]
    assert dict(confidence=stopc["confidence"], **stopc["opts"]) == {k: opts[k] for k in ("reproj_err", "confidence", "seed")}
    f = C.stop_facts(oracle, "low_noise_for_the_batch")
    stop = P.stop_of(f["hist"], stopc["n"], opts["confidence"], opts["iterations"])[0]
    assert stop == f["stop"] < opts["iterations"] and stop % P.ROUND and stop % P.GROUP and "unused_hypothesis" in f["kinds"]
    single = [_device(X, uv, **opts) for X, uv in probs]
    assert [s[0] for s in single] == [-3, 0, 0, -4, 0, 0, 0]
    for s, (X, uv) in zip(single, probs):
        ref = oracle.solve_pnp_ransac(X, uv, K, **opts)
        assert s[0] == ref[0] and s[4] == ref[4] and np.array_equal(s[3], ref[3])
    assert single[5][4] == f["used"][-1][1]                               # the model of the last improvement before the stop
    run_on = oracle.solve_pnp_ransac(stopc["X"], stopc["uv"], K, iterations=f["round_end"], confidence=P.NO_STOP, **stopc["opts"])
    assert run_on[4] > single[5][4]                                       # which the rest of its round would have replaced
    pad = 3
    for order in (list(range(len(probs))), list(reversed(range(len(probs))))):
        sel = [probs[i] for i in order]
        obj = np.concatenate([np.full((pad, 3), 7.0)] + [p[0] for p in sel] + [np.full((pad, 3), 7.0)])
        img = np.concatenate([np.full((pad, 2), 7.0)] + [p[1] for p in sel] + [np.full((pad, 2), 7.0)])
        off = (pad + np.concatenate([[0], np.cumsum([len(p[0]) for p in sel])])).astype(np.int32)
        status, rvec, tvec, mask, ninl = geometry.solve_pnp_ransac_batch(obj, img, off, K, opts["iterations"], opts["reproj_err"],
                                                                         opts["confidence"], opts["seed"])
        assert len(mask) == off[-1] + pad and not mask[:pad].any() and not mask[off[-1]:].any()
        for b, i in enumerate(order):
            st, rv, tv, m, n_in = single[i]
            assert (status[b], ninl[b]) == (st, n_in), (order, b)
            assert np.array_equal(mask[off[b]:off[b + 1]], m), (order, b)
            if st == 0:
                assert np.array_equal(rvec[b], rv) and np.array_equal(tvec[b], tv), (order, b)


# ---------------------------------------------------------------------------------------------- the shared table
def test_table_is_rewritten_when_the_seed_changes(oracle, kernel_dk_rule):
    """ensure_rng keeps one table for E-RANSAC and PnP: every call that changes the seed has to rewrite it, whichever operator
    wrote it last.  A context of its own, so that the order of the calls is the whole history of its table."""
    from twoview import scene
    from visual_odometry_amd import _lib, geometry
    c = _lib.Context(0)
    try:
        X, uv, *_ = problem(304, 150, 0.5, noise=1.0)
        Kt, _, _, p1, p2 = scene(64, 400, outliers=0.6)
        popts = dict(iterations=300, reproj_err=3.0, confidence=0.999)

        def pnp(seed):
            ref = _check(oracle, X, uv, POSE_TOL, ("pnp", seed), ctx=c, seed=seed, **popts)
            assert ref[0] == 0
            return _device(X, uv, ctx=c, seed=seed, **popts)

        def essential(seed):
            rc, Er, mr, _ = kernel_dk_rule.find_essential_ransac(p1, p2, Kt, prob=0.999, max_iters=1000, seed=seed)
            E, mask = geometry.findEssentialMat(p1, p2, Kt, geometry.FM_RANSAC, 0.999, 1.0, 1000, seed=seed, ctx=c)
            assert rc == 0 and np.array_equal(mask.ravel(), mr) and np.array_equal(E, Er[0]), ("E", seed)
            return mr

        a = pnp(7)
        e_default = essential(P.DEFAULT_SEED)
        d = pnp(P.DEFAULT_SEED)
        e7 = essential(7)
        b = pnp(7)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert not np.array_equal(a[3], d[3]) and not np.array_equal(e7, e_default)     # the seed does change both results
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------- chain entries
def test_localize_chain_passes_the_options_on(oracle, kernel_dk_rule):
    """FrontEnd.localize_chain with iterations / reproj_err / confidence / seed none of which is a default, against
    reference_chain with the same options, each step on the device's previous camera (tests/test_gpu_chain.py's rule).
    FrontEnd.slam_chain with the same options is tests/test_gpu_slam_chain.py::test_pnp_options_reach_the_kernel, beside the
    resident run it shares."""
    from test_gpu_chain import reference_chain
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    n, w, h, nfeat = 7, 640, 480, 1000
    seq = synth.sequence(n, w, h, step=4.0, cache_dir="/tmp")
    Ks = seq["K"]
    pairs = [[k, k + 1] for k in range(n - 1)]
    fe = FrontEnd(h, w, max_frames=n, max_pairs=n - 1, nfeatures=nfeat)
    try:
        fe.upload(seq["frames"]); fe.detect(0, n)
        fe.run_pairs(pairs, Ks, want_points=True)
        default = fe.localize_chain(n - 1, Ks)
        got = fe.localize_chain(n - 1, Ks, **CHAIN_PNP)
        p = oracle.orb_params(nfeatures=nfeat)
        feats = [oracle.orb_detect_and_compute(seq["frames"][f], p) for f in range(n)]
        want = reference_chain(oracle, feats, pairs, Ks, follow=got["poses"], pnp=CHAIN_PNP)
        assert got["status"].tolist() == want["status"]
        assert got["n_corr"].tolist() == want["n_corr"] and got["n_inl"].tolist() == want["n_inl"]
        assert got["n_map"].tolist() == want["n_map"]
        for k in range(n):
            assert np.abs(got["poses"][k] - want["poses"][k]).max() < 1e-6, k
        assert want["status"][1] == 0 and want["n_inl"][1] > 4
        assert got["n_inl"].tolist() != default["n_inl"].tolist()             # the options reached the kernel
    finally:
        fe.ctx.close()

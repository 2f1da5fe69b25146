"""GPU parity of k_ransac after its register and LDS footprint was cut (elimination in registers, null-space basis and B(z)
parked in LDS over the root finding, two waves per SIMD), against the CPU oracle's `find_essential_ransac` and `five_point`,
through the entry points of tests/test_gpu_ransac_quad.py and tests/test_gpu_geometry_split.py: findEssentialMat (one pair
from chosen points), the stage call five_point, and the batched front end, which alone reports `ransac_iters`.

What each group is for:

 * match counts 4, 5, 6, 8 (too few to sample, the minimum sample, the first counts with a choice), 63 / 64 / 65 and
   255 / 256 / 257 (one more or less than the 64 lanes a wave scores at once, and than the workgroup's 256 threads);
 * batches of 1, 2 and 3 pairs (an odd pair alone on a compute unit), where a pair that ends in round 0 sits beside one that
   needs several rounds (a third of its matches are inliers), also with `max_iters` one below and one above one and two
   rounds of 64 samples (and of the 16 and 32 the kernel can be built with);
 * samples with repeated and with collinear points (rank-deficient null space, zero pivot, a polynomial of lower degree,
   coincident roots): which of these paths a sample takes is not asserted, only that the kernel returns what the oracle does.
   The match count 4 is answered by findEssentialMat in Python, as cv2 does; 1 .. 4 matches do not reach the kernel through
   any entry point (tests/test_gpu_ransac_quad.py covers M = 0 through the batched path).

Tolerances are those of tests/test_gpu_ransac_quad.py: with the 300-sweep solver E, mask, inlier count and iteration count
equal the oracle's bit for bit; with the default solver masks and counts are equal and E and [R|t] are within 1e-4 of the
oracle's 300-sweep result.  The oracle's results are computed once per problem and shared."""
import functools

import numpy as np
import pytest
from test_gpu_geometry_split import TIGHT, Problem
from test_gpu_ransac_quad import oracle_iterations
from twoview import scene

pytestmark = pytest.mark.gpu

MODES = ["opencv300", "fast"]
COUNTS = [5, 6, 8, 63, 64, 65, 255, 256, 257]
ROUNDS = (16, 32, 64)
BUDGETS = sorted({r * k + d for r in ROUNDS for k in (1, 2) for d in (-1, 1)})       # 15 .. 129


@pytest.fixture
def solver(ctx, oracle, request):
    assert not oracle.get_dk_early_exit()
    ctx.set_poly_solver(request.param)
    yield request.param
    ctx.set_poly_solver("fast")


@functools.lru_cache(maxsize=None)
def points(m, outliers=0.3):
    K, _, _, p1, p2 = scene(200 + m, max(m, 40), outliers=outliers)
    return K, p1[:m].copy(), p2[:m].copy()


_REF = {}


def reference(oracle, key, K, p1, p2, **kw):
    """The oracle's result for a problem, computed once."""
    if key not in _REF:
        _REF[key] = oracle.find_essential_ransac(p1, p2, K, **kw)
    return _REF[key]


def compare(oracle, mode, K, p1, p2, ref, tag, **kw):
    """findEssentialMat against the oracle's (rc, E, mask, n_inl) under the module's tolerances."""
    from visual_odometry_amd import geometry
    rc, Er, mr, nr = ref
    E, mask = geometry.findEssentialMat(p1, p2, K, geometry.FM_RANSAC, kw.get("prob", 0.99), kw.get("thresh", 1.0), kw.get("max_iters", 1000))
    if rc != 0:
        assert E is None, tag
        return
    assert E is not None, tag
    assert np.array_equal(mask.ravel(), mr) and int(mask.sum()) == nr, tag
    got = E.reshape(-1, 3, 3)
    assert got.shape == Er.shape, tag
    if mode == "opencv300":
        assert np.array_equal(got, Er), tag
        return
    assert np.abs(got - Er).max() < 1e-4, tag
    if len(p1) > 5:                                   # one model: its pose against the pose of the oracle's model
        inl = mr > 0
        ng, R, t, _ = geometry.recoverPose(got[0], p1[inl], p2[inl], K)
        ngr, Rr, tr, _ = oracle.recover_pose(Er[0], p1[inl], p2[inl], K)
        assert ng == ngr, tag
        assert np.abs(np.hstack([R, t.reshape(3, 1)]) - np.hstack([Rr, tr.reshape(3, 1)])).max() < 1e-4, tag


# ---------------------------------------------------------------------------------------------- match counts
def test_four_matches_are_too_few(ctx):
    from visual_odometry_amd import geometry
    K, p1, p2 = points(8)
    assert geometry.findEssentialMat(p1[:4], p2[:4], K) == (None, None)


@pytest.mark.parametrize("solver", MODES, indirect=True)
@pytest.mark.parametrize("m", COUNTS)
def test_match_counts(oracle, solver, m):
    K, p1, p2 = points(m)
    ref = reference(oracle, ("count", m), K, p1, p2, prob=0.99)
    compare(oracle, solver, K, p1, p2, ref, (solver, m))


# ---------------------------------------------------------------------------------------------- budgets around the round sizes
@pytest.mark.parametrize("solver", MODES, indirect=True)
def test_budgets_around_the_rounds(oracle, solver):
    """400 matches of which about 30 % are inliers: the adaptive bound stays in the hundreds, so every budget below ends
    the loop at the budget, inside, at the end of or just after a round."""
    K, p1, p2 = points(400, outliers=0.7)
    full = reference(oracle, ("budget", 1000), K, p1, p2, prob=0.999, max_iters=1000)
    assert full[0] == 0 and oracle_iterations(oracle, p1, p2, K, 0.999, 1.0, 1000) > 2 * max(ROUNDS)
    compare(oracle, solver, K, p1, p2, full, (solver, 1000), prob=0.999, max_iters=1000)
    for budget in BUDGETS:
        ref = reference(oracle, ("budget", budget), K, p1, p2, prob=0.999, max_iters=budget)
        compare(oracle, solver, K, p1, p2, ref, (solver, budget), prob=0.999, max_iters=budget)


# ---------------------------------------------------------------------------------------------- degenerate samples
LINE = [[-2, 0], [-1, 0], [0, 0], [1, 0], [2, 0]]
SQUARE = [[0, 0], [1, 0], [0, 1], [1, 1]]
DEGENERATE = {
    "one_point_twice": (SQUARE + [[1, 1]], [[0, 0], [2, 0], [0, 2], [2, 2], [2, 2]]),
    "two_points_twice": ([[0, 0], [0, 0], [1, 0], [1, 0], [0, 1]], [[0, 1], [0, 1], [1, 1], [1, 1], [0, 2]]),
    "one_point_five_times": ([[1, 2]] * 5, [[2, 1]] * 5),
    "collinear_both": (LINE, [[-2, 1], [-1, 1], [0, 1], [1, 1], [2, 1]]),
    "collinear_first_only": (LINE, [[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1]]),
    "four_collinear": ([[-1, 0], [0, 0], [1, 0], [2, 0], [0, 1]], [[-1, 0.5], [0, 0.5], [1, 0.5], [2, 0.5], [0.25, 2]]),
    "three_collinear_one_twice": ([[-1, -1], [0, 0], [1, 1], [1, 1], [0, 2]], [[-1, -1], [0, 0], [1, 1], [1, 1], [0.5, 2]]),
}


@pytest.mark.parametrize("solver", ["opencv300"], indirect=True)
def test_degenerate_samples_300_sweeps_bit_identical(oracle, solver):
    from visual_odometry_amd import geometry
    for name, (a, b) in DEGENERATE.items():
        a, b = np.array(a, np.float64), np.array(b, np.float64)
        got, ref = geometry.five_point(a, b), oracle.five_point(a, b)
        assert got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True), name


def test_degenerate_samples_default_solver_same_rule(ctx, kernel_dk_rule):
    from visual_odometry_amd import geometry
    for name, (a, b) in DEGENERATE.items():
        a, b = np.array(a, np.float64), np.array(b, np.float64)
        got, ref = geometry.five_point(a, b), kernel_dk_rule.five_point(a, b)
        assert got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True), name


@pytest.mark.parametrize("solver", MODES, indirect=True)
def test_repeated_matches_in_the_set(oracle, solver):
    """A match set in which every match appears three times (a sample of five then often holds a point twice), and one
    of points on two lines."""
    K, p1, p2 = points(64)
    r1, r2 = np.repeat(p1[:20], 3, axis=0), np.repeat(p2[:20], 3, axis=0)
    compare(oracle, solver, K, r1, r2, reference(oracle, "tripled", K, r1, r2, prob=0.99), (solver, "tripled"))
    s = np.linspace(-1.0, 1.0, 12)
    l1 = np.concatenate([np.stack([320 + 200 * s, 240 + 0 * s], 1), np.stack([320 + 0 * s, 240 + 150 * s], 1)])
    l2 = (l1 - np.array([320.0, 240.0])) * 1.03 + np.array([332.0, 237.0])
    compare(oracle, solver, K, l1, l2, reference(oracle, "lines", K, l1, l2, prob=0.99), (solver, "lines"))


# ---------------------------------------------------------------------------------------------- batches, with the iteration count
PAIRS = [[0, 0], [0, 1], [1, 2]]                 # a frame with itself ends in round 0; neighbours at 0.3 px need several rounds


@pytest.fixture(scope="module")
def batch_problem(oracle, seq_small):
    assert not oracle.get_dk_early_exit()
    f = seq_small["frames"]
    return Problem(oracle, [f[0], f[1], f[2]], seq_small["K"], 500)


def batch_ref(pr, i, j, max_iters):
    """Problem.ref with a budget: (status, E, n_inl, iterations) of the oracle for pair (i, j) under TIGHT."""
    key = ("batch", i, j, max_iters)
    if key not in _REF:
        O = pr.oracle
        qi, ti, _ = O.match_hamming(pr.det[i]["desc"], pr.det[j]["desc"], 2)
        p1, p2 = pr.det[i]["xy"][qi].astype(np.float64), pr.det[j]["xy"][ti].astype(np.float64)
        rc, E, mask, ninl = O.find_essential_ransac(p1, p2, pr.K, max_iters=max_iters, **TIGHT)
        iters = oracle_iterations(O, p1, p2, pr.K, TIGHT["prob"], TIGHT["thresh"], max_iters)
        _REF[key] = dict(status=rc, E=E[0] if rc == 0 else None, n_inl=ninl if rc == 0 else 0, n_match=len(p1), ransac_iters=iters)
    return _REF[key]


def check_batch(res, k, ref, exact, tag):
    for name in ("status", "n_match", "n_inl", "ransac_iters"):
        assert int(res[k][name]) == ref[name], (tag, name, int(res[k][name]), ref[name])
    if ref["status"] == 0:
        E = res[k]["E"].reshape(3, 3)
        assert np.array_equal(E, ref["E"]) if exact else np.abs(E - ref["E"]).max() < 1e-4, tag


@pytest.mark.parametrize("mode", MODES)
def test_batches_of_one_two_three(batch_problem, mode):
    pr = batch_problem
    ends, pending = batch_ref(pr, 0, 0, 1000), batch_ref(pr, 0, 1, 1000)
    assert ends["status"] == 0 and ends["ransac_iters"] <= min(ROUNDS)
    assert pending["status"] == 0 and pending["ransac_iters"] > 2 * max(ROUNDS)
    fe = pr.front_end(len(PAIRS))
    fe.ctx.set_poly_solver(mode)
    try:
        for batch in (PAIRS[:1], PAIRS[1:2], PAIRS[:2], PAIRS[1::-1], PAIRS, PAIRS[::-1]):
            res, _ = fe.run_pairs(batch, pr.K, opts=fe.make_opts(**TIGHT))
            for k, (i, j) in enumerate(batch):
                check_batch(res, k, batch_ref(pr, i, j, 1000), mode == "opencv300", (mode, batch, k))
    finally:
        fe.ctx.set_poly_solver("fast")


@pytest.mark.parametrize("mode", MODES)
def test_batch_budgets_around_the_rounds(batch_problem, mode):
    """The pair that ends in round 0 beside the one that would go on, under budgets one below and one above one and two
    rounds: the reported count is the budget for the second and stays what it was for the first."""
    pr = batch_problem
    fe = pr.front_end(2)
    fe.ctx.set_poly_solver(mode)
    try:
        for budget in (63, 65, 127, 129):
            res, _ = fe.run_pairs(PAIRS[:2], pr.K, opts=fe.make_opts(max_iters=budget, **TIGHT))
            for k, (i, j) in enumerate(PAIRS[:2]):
                ref = batch_ref(pr, i, j, budget)
                check_batch(res, k, ref, mode == "opencv300", (mode, budget, k))
            assert batch_ref(pr, 0, 1, budget)["ransac_iters"] == budget
    finally:
        fe.ctx.set_poly_solver("fast")

"""GPU parity of the quad five-point solver (one sample per four lanes) and of the RANSAC round built on it, against the
CPU oracle: `oracle.five_point` through the raw stage call, `oracle.find_essential_ransac` through findEssentialMat, and
the batched front end for the iteration counter the kernel reports.

Every input below was picked on the CPU with the oracle alone, so that each case reaches the path it is named for:

 * five-point samples: the oracle's model count tells the number of kept real roots, and that count is what the
   fixture asserts on the CPU, together with the rank of the 5 x 9 epipolar matrix (numpy) for the samples without a
   model.  The rarer paths (zero pivot, a polynomial of degree 9 or 8, a root whose xy1[2] falls under the 1e-10 skip
   threshold) do not show in the oracle's return values: SPECIAL_SAMPLES are structured inputs (small integers and binary
   fractions, exact on every machine) that exercise them, but which path each takes is NOT asserted here, only that the
   kernel returns the oracle's models for it.  An odd model count (1) at least implies an odd degree, i.e. below 10.
 * RANSAC problems: the oracle does not return its iteration count, but the count follows from what it does return:
   the best sample's position is the smallest `max_iters` for which the oracle already returns its final model (the
   sample sequence does not depend on `max_iters`), and the adaptive bound after that model is RANSACUpdateNumIters of
   its inlier count; the loop runs to the larger of the two.  `oracle_iterations` does that; the parametrised cases
   assert the count they were picked for, so a case that drifts off its path fails instead of passing for nothing.
   A solver wave takes 16 samples; the cases sit on both sides of 16, 32 and 64 so that they hold for every round size
   the kernel can be built with, and `max_iters` of 1, 17, 33 and 1000 are multiples of none.

Tolerances are those of tests/test_gpu_faithful.py and tests/test_gpu_geometry.py: in 300-sweep mode E, mask and
iteration count equal bit for bit; in the default mode against the oracle's 300 sweeps masks and counts equal and E
within 1e-4; in the default mode against the oracle running the kernel's exit rule, bit for bit again."""
import math

import numpy as np
import pytest
from twoview import five_point_sample, oracle_pair_stages, scene

pytestmark = pytest.mark.gpu

ROUND = 16          # samples per solver wave; the round is 16, 32 or 64 samples


@pytest.fixture
def ctx300(ctx, oracle):
    assert not oracle.get_dk_early_exit()
    ctx.set_poly_solver("opencv300")
    yield ctx
    ctx.set_poly_solver("fast")


# ---------------------------------------------------------------------------------------------- oracle-side iteration count
def update_num_iters(prob, ep, max_iters):
    """RANSACUpdateNumIters for 5 model points (ptsetreg.cpp), as oracle/voo_geom.c and the kernel compute it."""
    prob = min(max(prob, 0.0), 1.0); ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - prob, np.finfo(np.float64).tiny)
    denom = 1.0 - (1.0 - ep) ** 5
    if denom < np.finfo(np.float64).tiny:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(np.rint(num / denom))


def oracle_last_change(oracle, p1, p2, K, prob, thresh, max_iters):
    """(sample at which the oracle's RANSAC loop took its final model, its inlier count), from its results alone (see the
    module docstring); (None, 0) where no model was ever accepted."""
    rc, E, mask, ninl = oracle.find_essential_ransac(p1, p2, K, prob=prob, thresh=thresh, max_iters=max_iters)
    if rc != 0:
        return None, 0
    lo, hi = 1, max(max_iters, 1)                    # smallest budget that already ends with the final model
    while lo < hi:
        mid = (lo + hi) // 2
        rc2, E2, mask2, _ = oracle.find_essential_ransac(p1, p2, K, prob=prob, thresh=thresh, max_iters=mid)
        if rc2 == 0 and np.array_equal(E2, E) and np.array_equal(mask2, mask):
            hi = mid
        else:
            lo = mid + 1
    return lo, ninl


def oracle_iterations(oracle, p1, p2, K, prob, thresh, max_iters):
    """Iterations the oracle's RANSAC loop ran, from its results alone (see the module docstring)."""
    last, ninl = oracle_last_change(oracle, p1, p2, K, prob, thresh, max_iters)
    if last is None:
        return max(max_iters, 1)                     # no model was ever accepted: the bound never moved
    return max(last, update_num_iters(prob, (len(p1) - ninl) / len(p1), max(max_iters, 1)))


# ---------------------------------------------------------------------------------------------- five-point samples
CROSS = [[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1]]
# name: (x1, x2, models the oracle returns with 300 sweeps, rank of the epipolar matrix); the names say what the samples
# were built for, the two numbers are what is asserted
SPECIAL_SAMPLES = {
    "rank_deficient_null_space": ([[2, 1], [-1, -1], [1, 0], [-1, -1], [-1, -1]], [[-1, -2], [1, 1], [2, 0], [1, -1], [1, 1]], 0, 4),
    "zero_pivot": ([[0, 0], [-1, 0], [2, 0], [-1, 0], [-2, 0]], [[-1, 0], [-1, -2], [1, 1], [1, 0], [-1, 1]], 0, 5),
    "zero_pivot_all_zero": ([[0, 0]] * 5, [[0, 0]] * 5, 0, 1),
    "degree_9_and_skipped_root": (CROSS, (np.array(CROSS) * 0.25).tolist(), 2, 5),
    "degree_9_five_real_one_skipped": (CROSS, (np.array(CROSS) * 1.5).tolist(), 4, 5),
    "degree_9_one_real_root": ([[-2, -1], [2, -1], [0, -1], [1, -1], [-1, 1]], [[1, 1], [0, 0], [-1, -1], [2, 2], [0, 2]], 1, 5),
    "degree_8": (CROSS, (np.array(CROSS) * 0.5).tolist(), 4, 5),
    "ten_nan_models": ([[0, 0], [1, 0], [0, 1], [1, 1], [2, 1]], [[0, 0], [1, 0], [0, 1], [1, 1], [2, 1]], 10, 5),
}


def same_models(got, ref):
    """Bit for bit; a NaN equals a NaN (the `ten_nan_models` sample: IEEE leaves a NaN's sign and payload to the machine)."""
    return got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)


def uniform_samples(oracle, want, limit=40000):
    """Samples of unrelated points (no two-view geometry behind them), scanned with the oracle until one of each wanted
    model count has turned up.  Such samples reach 0 and 10 real roots, which samples of a real scene rarely do."""
    rng = np.random.default_rng(3)
    found = {}
    for _ in range(limit):
        a, b = rng.uniform(-1, 1, (5, 2)), rng.uniform(-1, 1, (5, 2))
        n = len(oracle.five_point(a, b))
        if n in want and n not in found:
            found[n] = (a, b)
            if len(found) == len(want):
                break
    return found


@pytest.fixture
def five_point_cases(oracle):
    """(name, x1, x2) for the literal samples and for scanned samples with 0, 2, 4, 6, 8 and 10 models; asserts on the CPU
    that each has the model count it is named for."""
    assert not oracle.get_dk_early_exit()
    cases = []
    for name, (a, b, n, rank) in SPECIAL_SAMPLES.items():
        a, b = np.array(a, np.float64), np.array(b, np.float64)
        assert len(oracle.five_point(a, b)) == n, name
        q = np.array([[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0] for (u1, v1), (u2, v2) in zip(a, b)])
        assert np.linalg.matrix_rank(q) == rank, name     # < 5: no four-dimensional null space; 5 with no model: lost later
        cases.append((name, a, b))
    found = uniform_samples(oracle, {0, 2, 4, 6, 8, 10})
    assert sorted(found) == [0, 2, 4, 6, 8, 10]
    cases += [(f"uniform_{n}_models", *found[n]) for n in sorted(found)]
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(20000):                               # samples of a real two-view scene: 2, 4, 6 and 8 models
        a, b = five_point_sample(rng)
        n = len(oracle.five_point(a, b))
        if n not in seen:
            seen.add(n); cases.append((f"scene_{n}_models", a, b))
        if seen >= {2, 4, 6, 8}:
            break
    assert seen >= {2, 4, 6, 8}
    return cases


def test_five_point_300_sweeps_bit_identical(oracle, ctx300, five_point_cases):
    from visual_odometry_amd import geometry
    for name, a, b in five_point_cases:
        got, ref = geometry.five_point(a, b), oracle.five_point(a, b)
        assert same_models(got, ref), name


def test_five_point_default_solver_bit_identical_to_same_rule(ctx, five_point_cases, kernel_dk_rule):
    from visual_odometry_amd import geometry
    for name, a, b in five_point_cases:
        got, ref = geometry.five_point(a, b), kernel_dk_rule.five_point(a, b)
        assert same_models(got, ref), name


def test_five_point_repeats_do_not_interfere(oracle, ctx300, five_point_cases):
    """The quad's exchanges leave nothing behind: any order of the samples gives the same models."""
    from visual_odometry_amd import geometry
    ref = {name: oracle.five_point(a, b) for name, a, b in five_point_cases}
    for name, a, b in list(reversed(five_point_cases)) + five_point_cases:
        assert same_models(geometry.five_point(a, b), ref[name]), name


# ---------------------------------------------------------------------------------------------- RANSAC rounds
# (name, scene arguments, points used, prob, max_iters, iterations the oracle runs in 300-sweep mode)
# The expected counts were read off `oracle_iterations` on the CPU; they are asserted, not assumed.
def _problem(seed, n, outl, take=None):
    K, R, t, p1, p2 = scene(seed, n, outliers=outl)
    return K, p1[:take], p2[:take]


def _unrelated(seed, n):
    """n correspondences without a two-view geometry behind them, the second point up to 400 px from the first: few models
    gather a sixth and a seventh inlier by chance, so the final model comes late."""
    rng = np.random.default_rng(seed)
    p1 = rng.uniform([0, 0], [640, 480], (n, 2))
    return np.array([[800, 0, 320], [0, 800, 240], [0, 0, 1.0]]), p1, p1 + rng.uniform(-400.0, 400.0, (n, 2))


def case_problem(name):
    """(K, p1, p2) of a RANSAC case: a scene, or for the cases in UNRELATED (seed, n) of _unrelated."""
    _, seed, n, outl, take, _, _ = _ransac_case(name)
    return _unrelated(seed, n) if name in UNRELATED else _problem(seed, n, outl, take)


RANSAC_CASES = [
    # name,                 seed, n,   outl, take, prob,  max_iters
    ("one_wave",            60,   800, 0.1,  None, 0.99,  1000),
    ("over_16",             61,   400, 0.25, None, 0.99,  1000),
    ("over_32",             1,    800, 0.3,  None, 0.99,  1000),
    ("over_64_by_little",   62,   400, 0.3,  None, 0.99,  1000),
    ("over_64",             63,   400, 0.5,  None, 0.99,  1000),
    ("several_rounds",      64,   400, 0.6,  None, 0.999, 1000),
    ("budget_exhausted",    65,   300, 0.85, None, 0.999, 1000),
    ("max_iters_1",         63,   400, 0.5,  None, 0.99,  1),
    ("max_iters_17",        63,   400, 0.5,  None, 0.99,  17),
    ("max_iters_33",        63,   400, 0.5,  None, 0.99,  33),
    ("max_iters_33_hard",   65,   300, 0.85, None, 0.999, 33),
    ("M_5",                 31,   200, 0.0,  5,    0.99,  1000),
    ("M_6",                 31,   200, 0.0,  6,    0.99,  1000),
    ("M_7",                 31,   200, 0.0,  7,    0.99,  1000),
    ("M_6_outliers",        66,   200, 0.5,  6,    0.999, 1000),
    ("M_7_outliers",        66,   200, 0.5,  7,    0.999, 1000),
    ("M_8_outliers",        66,   200, 0.5,  8,    0.999, 1000),
    ("past_the_table",      76,   13,  None, None, 1 - 2.0 ** -53, 2000),       # unrelated points, not a scene
]
UNRELATED = {"past_the_table"}
# Which of these cases take their final model from a sample drawn past the table is asserted on the CPU, where the CPU suite
# runs it: tests/test_pnp_control_reference.py::test_which_essential_cases_draw_past_the_table (only `past_the_table`).

# what each case has to reach, as a range of the oracle's iteration count (inclusive)
RANSAC_REACH = {
    "one_wave": (2, ROUND), "over_16": (ROUND + 1, 2 * ROUND), "over_32": (2 * ROUND + 1, 4 * ROUND),
    "over_64_by_little": (4 * ROUND + 1, 6 * ROUND), "over_64": (4 * ROUND + 1, 1000), "several_rounds": (5 * 4 * ROUND, 1000), "budget_exhausted": (1000, 1000),
    "max_iters_1": (1, 1), "max_iters_17": (17, 17), "max_iters_33": (33, 33), "max_iters_33_hard": (33, 33),
    "past_the_table": (1509, 1509),
}


def _ransac_case(name):
    return next(c for c in RANSAC_CASES if c[0] == name)


@pytest.mark.parametrize("name", [c[0] for c in RANSAC_CASES])
def test_ransac_300_sweeps_bit_identical(oracle, ctx300, name):
    from visual_odometry_amd import geometry
    _, _, _, _, _, prob, max_iters = _ransac_case(name)
    K, p1, p2 = case_problem(name)
    rc, Er, mr, nr = oracle.find_essential_ransac(p1, p2, K, prob=prob, max_iters=max_iters)
    iters = oracle_iterations(oracle, p1, p2, K, prob, 1.0, max_iters) if len(p1) > 5 else 0
    if name in RANSAC_REACH:
        lo, hi = RANSAC_REACH[name]
        assert lo <= iters <= hi, (name, iters)
    E, mask = geometry.findEssentialMat(p1, p2, K, geometry.FM_RANSAC, prob, 1.0, max_iters)
    if rc != 0:
        assert E is None, name
        return
    assert E is not None and np.array_equal(mask.ravel(), mr), name
    assert np.array_equal(E.reshape(-1, 3, 3), Er), name            # M == 5: the stacked models, all of them
    # the same problem under every smaller budget that ends inside, at and after a round: the kernel's consumed-sample
    # rule (`r0 + h >= niters`) decides the same as the oracle's loop bound
    for budget in (iters - 1, iters, iters + 1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND, 2 * ROUND + 1, 4 * ROUND, 4 * ROUND + 1):
        if len(p1) <= 5 or budget < 1 or budget > max_iters:
            continue
        rc, Er, mr, nr = oracle.find_essential_ransac(p1, p2, K, prob=prob, max_iters=budget)
        E, mask = geometry.findEssentialMat(p1, p2, K, geometry.FM_RANSAC, prob, 1.0, budget)
        if rc != 0:
            assert E is None, (name, budget)
            continue
        assert E is not None and np.array_equal(mask.ravel(), mr) and np.array_equal(E, Er[0]), (name, budget)


@pytest.mark.parametrize("name", [c[0] for c in RANSAC_CASES])
def test_ransac_default_solver_vs_faithful_oracle(oracle, ctx, name):
    from visual_odometry_amd import geometry
    assert not oracle.get_dk_early_exit()
    _, _, _, _, _, prob, max_iters = _ransac_case(name)
    K, p1, p2 = case_problem(name)
    rc, Er, mr, nr = oracle.find_essential_ransac(p1, p2, K, prob=prob, max_iters=max_iters)
    E, mask = geometry.findEssentialMat(p1, p2, K, geometry.FM_RANSAC, prob, 1.0, max_iters)
    if rc != 0:
        assert E is None, name
        return
    assert E is not None and np.array_equal(mask.ravel(), mr), name
    got = E.reshape(-1, 3, 3)
    assert got.shape == Er.shape, name
    err = np.abs(got - Er).max()
    assert err < 1e-4, name


def test_fewer_than_five_points_python_guard(ctx):
    """findEssentialMat answers M < 5 in Python, as cv2 does; the kernel's own M < 5 branch is reached by the next test."""
    from visual_odometry_amd import geometry
    K, p1, p2 = _problem(31, 200, 0.0)
    for m in range(5):
        assert geometry.findEssentialMat(p1[:m], p2[:m], K) == (None, None)


def test_batched_pair_with_too_few_matches(oracle, seq_small):
    """The kernel's M < 5 branch, through the batched path: a frame without a keypoint gives pairs without a match
    (M = 0; pairs of 1..4 matches: tests/test_gpu_pairs_chosen.py), beside a normal pair in the same launch."""
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    frames, K = seq_small["frames"], seq_small["K"]
    blank = np.full_like(frames[0], 128)
    p = oracle.orb_params(nfeatures=500)
    assert len(oracle.orb_detect_and_compute(blank, p)["xy"]) == 0
    ref = oracle.pair(blank, frames[0], p, K)
    assert ref["rc"] == _lib.VO_ERR_TOO_FEW and ref["n_match"] == 0
    fe = FrontEnd(480, 640, max_frames=3, max_pairs=3, nfeatures=500, nlevels=8, device=0)
    fe.upload(np.stack([blank, frames[0], frames[1]]))
    fe.detect(0, 3)
    res, _ = fe.run_pairs([[0, 1], [1, 2], [1, 0]], K)
    for k in (0, 2):
        assert int(res[k]["status"]) == _lib.VO_ERR_TOO_FEW
        assert (int(res[k]["n_match"]), int(res[k]["n_inl"]), int(res[k]["ransac_iters"])) == (0, 0, 0)
    good = oracle.pair(frames[0], frames[1], p, K)
    assert int(res[1]["status"]) == 0 and (int(res[1]["n_match"]), int(res[1]["n_inl"])) == (good["n_match"], good["n_inl"])


# ---------------------------------------------------------------------------------------------- the kernel's own counter
@pytest.mark.parametrize("mode", ["opencv300", "fast"])
def test_batched_iteration_counter_matches_oracle(oracle, ctx, seq_small, mode):
    """vo_pair_result.ransac_iters (only the batched path reports it) against the oracle's count, over near and wide
    pairs of the synthetic sequence.  Both modes: the counts are integers decided by inlier counts, which the default
    solver reproduces.  The kernel closes its counter from the round's end where the last samples of a round (or the
    samples before the one the loop stops at) have no model, so its count can fall short of the serial loop's and then
    depends on the round size (docs/experiments.md); E, mask and inlier count never do.  These six pairs do not meet
    that case at the committed round size, and the equality below is asserted for them as it stands."""
    from visual_odometry_amd.frontend import FrontEnd
    assert not oracle.get_dk_early_exit()
    frames, K = seq_small["frames"], seq_small["K"]
    pairs = [[0, 1], [1, 2], [2, 3], [0, 2], [1, 3], [0, 3]]
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=len(pairs), nfeatures=500, nlevels=8, device=0)
    fe.ctx.set_poly_solver(mode)
    try:
        fe.upload(frames)
        fe.detect(0, 4)
        res, _ = fe.run_pairs(pairs, K)
    finally:
        fe.ctx.set_poly_solver("fast")
    p = oracle.orb_params(nfeatures=500)
    for k, (i, j) in enumerate(pairs):
        st = oracle_pair_stages(oracle, frames[i], frames[j], p, K)
        p1 = st["d1"]["xy"][st["qi"]].astype(np.float64); p2 = st["d2"]["xy"][st["ti"]].astype(np.float64)
        iters = oracle_iterations(oracle, p1, p2, K, 0.99, 1.0, 1000)
        assert int(res[k]["n_match"]) == len(p1) and int(res[k]["n_inl"]) == st["n_inl"]
        assert int(res[k]["ransac_iters"]) == iters
        if mode == "opencv300":
            assert np.array_equal(res[k]["E"].reshape(3, 3), st["E"])
        else:
            assert np.abs(res[k]["E"].reshape(3, 3) - st["E"]).max() < 1e-4

"""CPU: tests/pnp_control.py (the random stream, the five-index draw, RANSACUpdateNumIters and the serial stop rule, re-typed)
against the oracle's solvePnPRansac, and the cases that tests/test_gpu_pnp_control.py runs on the device, frozen here with
the property each is named for asserted on the oracle, so that a case that drifts off its path fails instead of passing for
nothing.  The oracle is seen through its results alone: the first budget with a model (first_accept) and the budgets at which
its (mask, n_inl) changes (history).

Late acceptance: n points of which exactly five project exactly (the others are displaced by 30-100 px) and reproj_err = 0.5,
so a sample is accepted only when it is that five-subset.  The consistent five are CHOSEN from the restated sampler: the
subset drawn at a sample that lies where the case is wanted and that no earlier sample has drawn; the oracle then has to
accept first at exactly that sample, which is what is asserted.  Search that was run (CPU, seconds): n = 13, budget 4000, RNG
seeds default / 0 / 1 / 12345 / 2^63, the first samples of the first round that starts at or past 8192 + 448 and of the round
that contains position 8192 (3 candidates x 2 scene seeds each, 60 in all: the oracle accepted first at the predicted sample
in every one); n = 7 and n = 8, RNG seeds default, 1, 2, ... in order, taking samples of round 2 or later whose round consumes
more than 448 numbers and whose own draw starts 448 or more numbers into the round: n = 7 seeds 52, 83, 342, 345 and n = 8
seeds 3, 21, 31, 35 were the first four each (the default seed has none), again all accepted where predicted.
Every required kind was found.  Beyond them, `n8_last_staged_number` and `n7_last_staged_number` (RNG seeds 1-399 scanned, seeds
31 and 125 the first without index 0 among the five) accept at a sample whose draw keeps the number in the last slot of the
staged window, position 447 of its round: the window cases above start past the window and never depend on that slot.

Stop rule: 150 noisy scenes (tests/test_gpu_pnp.problem, scene seeds 0-149; n 40-300, noise 0.5-2 px, 30-60 % outliers,
reproj_err 2-8, budget 1000) x the five confidences were scanned with history(); the seven below cover every required kind.
With 1 - 1e-12 as the confidence the adaptive bound still falls below the budget once enough inliers are found (138
samples for 133 inliers of 190), so a history is only used up to `valid`, the sample at which that run itself would stop,
and every case asserts that its stop, the end of its stop's round and stop + 1 lie within it.

`low_noise_for_the_batch` is the stop-rule problem of the batched launch (BATCH_OPTS), whose one set of options has to be the
late-acceptance cases' reproj_err = 0.5: at that threshold the scenes above (noise 0.5-2 px) run to the budget, so this one has
noise 0.2 px and RNG seed 0.  Scanned: scene seeds 400-439 (n and outlier share drawn from the seed) at noise 0.2; seed 437
stops after sample 43, inside a group of round 1, and a later sample of that round would have been an improvement."""
import functools

import numpy as np
import pytest

import pnp_control as P
from test_gpu_pnp import K, problem

D = P.DEFAULT_SEED

# name: (n, scene seed, RNG seed, the five consistent points, budget, kind)
LATE_CASES = {
    "n13_round_beyond_table":   (13, 1, D,       (1, 4, 6, 10, 12),  4000, "beyond"),
    "n13_round_straddles":      (13, 1, D,       (3, 4, 6, 11, 12),  4000, "straddle"),
    "n13_seed_0_beyond":        (13, 2, 0,       (1, 3, 4, 5, 7),    4000, "beyond"),
    "n13_seed_2p63_beyond":     (13, 1, 2 ** 63, (0, 9, 10, 11, 12), 4000, "beyond"),
    "n13_seed_1_straddles":     (13, 2, 1,       (0, 7, 8, 11, 12),  4000, "straddle"),
    "n13_seed_12345_straddles": (13, 1, 12345,   (1, 4, 5, 10, 12),  4000, "straddle"),
    "n7_past_the_window":       (7,  1, 52,      (1, 2, 4, 5, 6),    300,  "window"),
    "n8_past_the_window":       (8,  1, 21,      (1, 3, 5, 6, 7),    300,  "window"),
    "n8_last_staged_number":    (8,  1, 31,      (1, 2, 3, 4, 5),    300,  "edge"),
    "n7_last_staged_number":    (7,  1, 125,     (1, 3, 4, 5, 6),    300,  "edge"),
    "n6_no_model":              (6,  1, D,       (0, 2, 3, 5),       300,  "no_model"),
}
# no model before the five are drawn, so the confidence cannot move the first acceptance; after it 5 of n leave the bound below it
LATE_CONFIDENCE = 0.999
SEED_CASES = {0: "n13_seed_0_beyond", 1: "n13_seed_1_straddles", 12345: "n13_seed_12345_straddles", 2 ** 63: "n13_seed_2p63_beyond",
              D: "n13_round_beyond_table"}

# name: (scene seed, n, noise, outliers, reproj_err, confidence, kinds the case is kept for)
STOP_BUDGET = 1000
STOP_CASES = {
    "improves_at_round_end":      (141, 169, 2.0, 0.6, 8.0, 0.99,     {"improves_last_of_round", "stops_in_round_3_or_later"}),
    "improves_and_stops_at_193":  (145, 171, 2.0, 0.4, 3.0, 0.5,      {"improves_first_of_round", "stops_inside_group", "stops_in_round_3_or_later"}),
    "six_improvements":           (145, 171, 2.0, 0.4, 3.0, 0.9,      {"improves_first_of_round", "improves_first_of_group", "improves_last_of_group", "stops_inside_group"}),
    "unused_in_round_3":          (134, 254, 2.0, 0.4, 6.0, 0.999,    {"unused_hypothesis", "stops_inside_group", "stops_in_round_3_or_later", "improves_last_of_group"}),
    "unused_in_round_1":          (108, 237, 1.5, 0.4, 4.0, 0.9,      {"unused_hypothesis", "improves_first_of_group", "improves_last_of_group", "stops_inside_group"}),
    "stops_at_its_improvement":   (128, 83,  1.5, 0.5, 8.0, 0.5,      {"stops_inside_group", "stops_in_round_3_or_later", "improves_first_of_group"}),
    "long_run":                   (121, 53,  1.5, 0.5, 3.0, 0.999999, {"stops_inside_group", "stops_in_round_3_or_later"}),
    "low_noise_for_the_batch":    (437, 190, 0.2, 0.3, 0.5, 0.999,    {"unused_hypothesis", "stops_inside_group"}),
}
STOP_SEEDS = {"low_noise_for_the_batch": 0}          # RNG seed of a case that does not run with the default
# the options both chain entries are run with (tests/test_gpu_pnp_control.py, tests/test_gpu_slam_chain.py): none is a default
CHAIN_PNP = dict(iterations=37, reproj_err=3.0, confidence=0.999, seed=7)
# the one set of options of the batched launch: none is a default, late acceptance past the table and an adaptive stop both occur
BATCH_OPTS = dict(iterations=1500, reproj_err=0.5, confidence=0.999, seed=0)
REQUIRED_KINDS = {"improves_last_of_round", "improves_first_of_round", "improves_last_of_group", "improves_first_of_group",
                  "stops_inside_group", "stops_in_round_3_or_later", "unused_hypothesis"}

# consensus sets of exactly k inliers among 9 points (scene seed 12, default RNG seed, reproj_err 0.5, budget 300): 5 non-planar
# inliers leave cv2's refinement without a DLT (the RANSAC model is returned), 6 are its minimum; planar sets take the homography
CONSENSUS_CASES = [(k, planar) for planar in (False, True) for k in (5, 6, 7)]
CONSENSUS_OPTS = dict(iterations=300, reproj_err=0.5)
# sizes around the strides of the scorer (64 lanes per hypothesis, 256 for the final mask) and of the refinement's reductions
SIZES = (6, 7, 63, 64, 65, 255, 256, 257, 511, 513)
SIZE_OPTS = dict(iterations=200, reproj_err=4.0, confidence=0.999)


# ---------------------------------------------------------------------------------------------- case builders
def consistent_scene(scene_seed, n, good, planar=False):
    """n points of which exactly those in `good` project exactly; the others are displaced by 30-100 px."""
    X, uv, R, t, _ = problem(scene_seed, n, 0.0, noise=0.0)
    if planar:
        X[:, 2] = 0.3 * X[:, 0] - 0.2 * X[:, 1] + 1.0
        Xc = X @ R.T + t
        uv = ((Xc / Xc[:, 2:]) @ K.T)[:, :2]
    rng = np.random.default_rng(5000 + scene_seed)
    ang = rng.uniform(0, 2 * np.pi, n); r = rng.uniform(30, 100, n)
    bad = np.ones(n, bool); bad[list(good)] = False
    uv[bad] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)[bad]
    return X, uv


@functools.lru_cache(maxsize=None)
def late_case(name):
    n, scene_seed, seed, good, budget, kind = LATE_CASES[name]
    X, uv = consistent_scene(scene_seed, n, good)
    return dict(name=name, X=X, uv=uv, n=n, good=good, budget=budget, kind=kind, seed=seed,
                opts=dict(reproj_err=0.5, confidence=LATE_CONFIDENCE, seed=seed))


@functools.lru_cache(maxsize=None)
def stop_case(name):
    scene_seed, n, noise, outl, err, conf, kinds = STOP_CASES[name]
    X, uv, *_ = problem(scene_seed, n, outl, noise=noise)
    opts = dict(reproj_err=err, seed=STOP_SEEDS[name]) if name in STOP_SEEDS else dict(reproj_err=err)
    return dict(name=name, X=X, uv=uv, n=n, budget=STOP_BUDGET, confidence=conf, kinds=kinds, opts=opts)


def consensus_case(k, planar):
    return consistent_scene(12, 9, tuple(range(1, 1 + k)), planar)


def size_case(n):
    X, uv, *_ = problem(200 + n, n, 0.3)
    return X, uv


_late_facts, _stop_facts = {}, {}


def late_facts(oracle, name):
    """dict(first = first accepted sample or None, start = its stream position, round, round_start, round_used)."""
    if name not in _late_facts:
        c = late_case(name)
        first = P.first_accept(oracle, c["X"], c["uv"], K, c["budget"], **c["opts"])
        subs = P.subsets(c["seed"], c["n"], P.ROUND * P.round_of(first or c["budget"]))
        f = dict(first=first, subs=subs, total=subs[min(c["budget"], len(subs) - 1)][1])
        if first:
            rnd = P.round_of(first)
            r0, used = P.round_span(subs, rnd)
            f.update(start=subs[first - 1][1], end=subs[first][1], round=rnd, round_start=r0, round_used=used)
        _late_facts[name] = f
    return _late_facts[name]


def stop_facts(oracle, name):
    """dict(hist, valid, stop, used, kinds) of a stop-rule case at its budget."""
    if name not in _stop_facts:
        c = stop_case(name)
        hist = P.history(oracle, c["X"], c["uv"], K, c["budget"], **c["opts"])
        valid = P.stop_of(hist, c["n"], P.NO_STOP, c["budget"])[0]
        stop, used = P.stop_of(hist, c["n"], c["confidence"], c["budget"])
        end = P.ROUND * P.round_of(stop)
        kinds = set()
        for s, _ in used:
            if s % P.ROUND == 0: kinds.add("improves_last_of_round")
            if s % P.ROUND == 1 and s > 1: kinds.add("improves_first_of_round")
            if s % P.GROUP == 0 and s % P.ROUND != 0: kinds.add("improves_last_of_group")
            if s % P.GROUP == 1 and s % P.ROUND != 1: kinds.add("improves_first_of_group")
        if stop % P.GROUP: kinds.add("stops_inside_group")
        if stop > 2 * P.ROUND: kinds.add("stops_in_round_3_or_later")
        if any(stop < s <= end for s, _ in hist): kinds.add("unused_hypothesis")
        _stop_facts[name] = dict(hist=hist, valid=valid, stop=stop, used=used, kinds=kinds, round_end=end)
    return _stop_facts[name]


def _state(oracle, c, iterations, confidence):
    rc, _, _, mask, ninl = oracle.solve_pnp_ransac(c["X"], c["uv"], K, iterations=iterations, confidence=confidence, **c["opts"])
    return rc, mask.tobytes(), ninl


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_stream_and_draw_restated():
    """The generator against hand-checkable values, and the sampler's own invariants."""
    a = 4164903690
    s1 = (0xFFFFFFFF * a) & 0xFFFFFFFFFFFFFFFF
    assert P.rng_stream(0, 2) == [s1 & 0xFFFFFFFF, (((s1 & 0xFFFFFFFF) * a + (s1 >> 32)) & 0xFFFFFFFF)]
    assert P.rng_stream(1, 1) == [a & 0xFFFFFFFF] and P.rng_stream(2 ** 63, 1) == [2 ** 31]       # low word 0: the carry alone
    assert P.rng_stream(0, 50) == P.rng_stream(0xFFFFFFFF, 50) != P.rng_stream(D, 50)
    for seed, n in ((D, 6), (7, 13), (0, 300)):
        stream = P.rng_stream(seed, 4000)
        subs = P.subsets(seed, n, 300)
        assert subs[0][1] == 0 and len(subs) == 301
        for (idx, start), (_, nxt) in zip(subs, subs[1:]):
            draws = [v % n for v in stream[start:nxt]]
            assert len(set(idx)) == 5 and list(dict.fromkeys(draws)) == list(idx) and draws[-1] == idx[-1]
    # expected draws per sample (the figures the staged window was sized with): 8.7 at n = 6, 7.65 at n = 7, 7.07 at n = 8
    for n, want in ((6, 8.7), (7, 7.65), (8, 7.07), (13, 6.01)):
        assert abs(sum(n / (n - i) for i in range(5)) - want) < 0.01
        assert abs(P.subsets(D, n, 2000)[-1][1] / 2000 - want) < 0.25


def test_update_num_iters_restated():
    assert P.update_num_iters(0.99, 0.5, 1000) == 145 and P.update_num_iters(0.99, 0.5, 100) == 100
    assert P.update_num_iters(0.99, 0.0, 1000) == 0 and P.update_num_iters(0.99, 1.0, 1000) == 1000
    assert P.update_num_iters(0.999, 0.5, 1000) == 218 and P.update_num_iters(0.5, 0.5, 1000) == 22
    assert P.stop_of([(3, 10), (9, 50)], 100, 0.99, 1000) == (145, [(3, 10), (9, 50)])
    assert P.stop_of([(3, 10), (200, 50)], 100, 0.99, 150) == (150, [(3, 10)])
    assert P.stop_of([(3, 10), (200, 50)], 100, 0.99, 1000) == (200, [(3, 10), (200, 50)])        # the bound falls below the sample


# ---------------------------------------------------------------------------------------------- late acceptance
@pytest.mark.parametrize("name", list(LATE_CASES))
def test_late_acceptance_is_where_the_sampler_says(oracle, name):
    c, f = late_case(name), late_facts(oracle, name)
    X, uv, opts = c["X"], c["uv"], c["opts"]
    if c["kind"] == "no_model":
        assert f["first"] is None and oracle.solve_pnp_ransac(X, uv, K, iterations=c["budget"], **opts)[0] == -4
        draws = f["total"]
        print(f"{name}: no model in {c['budget']} samples, {draws} numbers drawn ({draws / c['budget']:.2f} per sample)")
        assert draws > 8.2 * c["budget"]                                  # heavy redraws: 8.7 expected at n = 6
        assert all(len(set(idx) & set(c["good"])) < 5 for idx, _ in f["subs"][:-1])
        return
    first = f["first"]
    print(f"{name}: first accepted sample {first}, stream position {f['start']}, round {f['round']} "
          f"(starts at {f['round_start']}, consumes {f['round_used']})")
    assert first is not None and set(f["subs"][first - 1][0]) == set(c["good"])
    assert oracle.solve_pnp_ransac(X, uv, K, iterations=first - 1, **opts)[0] == -4
    rc, _, _, mask, ninl = oracle.solve_pnp_ransac(X, uv, K, iterations=first, **opts)
    assert rc == 0 and ninl == 5 and np.nonzero(mask)[0].tolist() == sorted(c["good"])
    if c["kind"] == "beyond":                                             # a whole round past the table
        assert f["start"] >= P.TABLE + P.WINDOW and f["round_start"] >= P.TABLE
    elif c["kind"] == "straddle":                                         # the winning round holds position 8192
        assert f["round_start"] < P.TABLE < f["round_start"] + f["round_used"]
    elif c["kind"] == "edge":                                             # the winning draw keeps the last staged number
        edge = f["round_start"] + P.WINDOW - 1
        assert f["start"] <= edge < f["end"] < P.TABLE
        draws = [v % c["n"] for v in P.rng_stream(c["seed"], edge + 1)[f["start"]:]]
        assert draws[-1] not in draws[:-1] and draws[-1] != 0             # an index of the five, and not what an unset slot reads
    else:                                                                 # the winning draw starts past the staged window
        assert f["round"] >= 2 and f["round_used"] > P.WINDOW and f["start"] - f["round_start"] >= P.WINDOW
        assert f["start"] < P.TABLE


def test_every_seed_has_its_case(oracle):
    """The stream for seeds 0 (mapped to 0xffffffff), 1, 12345, 2^63 and the default: each has a scene whose first acceptance
    the sampler predicts (asserted by the parametrised test above), and the five scenes' sample sequences differ."""
    assert sorted(SEED_CASES) == sorted({0, 1, 12345, 2 ** 63, D})
    firsts = set()
    for seed, name in SEED_CASES.items():
        c = late_case(name)
        assert c["seed"] == seed and late_facts(oracle, name)["first"] is not None
        firsts.add(tuple(P.subsets(seed, 13, 8)[:-1]))
    assert len(firsts) == 5


# ---------------------------------------------------------------------------------------------- stop rule
def test_stop_cases_cover_every_required_kind(oracle):
    got = set()
    for name, case in STOP_CASES.items():
        f = stop_facts(oracle, name)
        assert case[6] <= f["kinds"], (name, f["kinds"])
        got |= case[6]
    assert got == REQUIRED_KINDS


@pytest.mark.parametrize("name", list(STOP_CASES))
def test_stop_rule_reproduces_the_oracle(oracle, name):
    c, f = stop_case(name), stop_facts(oracle, name)
    stop, used, hist = f["stop"], f["used"], f["hist"]
    print(f"{name}: n {c['n']}, confidence {c['confidence']}: stops after sample {stop} (round {P.round_of(stop)}, "
          f"{(stop - 1) % P.ROUND + 1} of 64), improvements {used}, history valid to {f['valid']}, kinds {sorted(f['kinds'])}")
    assert len(used) >= 3 and max(stop + 1, f["round_end"]) <= f["valid"] <= c["budget"]
    for b in (stop - 1, stop, stop + 1, c["budget"]):
        s_b, used_b = P.stop_of(hist, c["n"], c["confidence"], b)
        assert s_b == min(b, stop)
        last, good = used_b[-1]
        got = _state(oracle, c, b, c["confidence"])
        assert got == _state(oracle, c, last, P.NO_STOP) and got[0] == 0 and got[2] == good, (name, b)
    if "unused_hypothesis" in c["kinds"]:                                 # its round holds a better hypothesis past the stop
        assert _state(oracle, c, f["round_end"], P.NO_STOP)[1] != _state(oracle, c, c["budget"], c["confidence"])[1]


# ---------------------------------------------------------------------------------------------- consensus sizes
@pytest.mark.parametrize("k,planar", CONSENSUS_CASES)
def test_consensus_cases_have_their_size(oracle, k, planar):
    X, uv = consensus_case(k, planar)
    poses = []
    try:
        for mode in ("cv2", "fast"):
            oracle.set_pnp_refine(mode)
            rc, rv, tv, mask, ninl = oracle.solve_pnp_ransac(X, uv, K, **CONSENSUS_OPTS)
            assert rc == 0 and ninl == k and np.nonzero(mask)[0].tolist() == list(range(1, 1 + k))
            poses.append(np.concatenate([rv, tv]))
    finally:
        oracle.set_pnp_refine("cv2")
    assert np.abs(poses[0] - poses[1]).max() < 1e-5
    if planar:                                                            # the plane is seen: W[2] / W[1] of the centred points
        w = np.linalg.svd(X[1:1 + k] - X[1:1 + k].mean(0), compute_uv=False)
        assert w[2] / w[1] < 1e-3


# ---------------------------------------------------------------------------------------------- E-RANSAC: the same table edge
def test_which_essential_cases_draw_past_the_table(oracle):
    """The sampler of k_ransac has three sources like k_pnp_ransac's: RS_STREAM = 512 numbers staged per round, the 8192-entry
    table, and past it the generator re-run from the seed.  Which RANSAC_CASES of tests/test_gpu_ransac_quad.py take their
    final model from a sample drawn past the table follows from the restated draw rule (subsets: the same `% M, redraw a
    repeat` rule) and the oracle's last model change.  Answer, asserted below: only `past_the_table`.  The cases of 300 or
    more points draw about 5.03 numbers per sample, 5 030 for their 1000 samples; M_7 / M_7_outliers and M_8_outliers draw
    7 746 and 7 117 for theirs; M_6 and M_6_outliers would draw 8 628 but take their final model at samples 9 and 1 (83 and
    10 numbers) and stop after 9 and 13.  `past_the_table` was picked for it: 13 unrelated correspondences (6.0 numbers per
    sample), scanned over seeds 0-249 with a confidence of 1 - 2^-53, under which six inliers of 13 leave the bound at 1734:
    seeds 76 and 92 reach seven inliers only at samples 1509 and 1480, whose draws end at 9 112 and 8 942."""
    import test_gpu_ransac_quad as Q
    assert not oracle.get_dk_early_exit()
    past = {}
    for name, _, _, _, _, prob, max_iters in Q.RANSAC_CASES:
        Kq, p1, p2 = Q.case_problem(name)
        M = len(p1)
        if M <= 5:
            continue
        subs = P.subsets(D, M, max(max_iters, 1))
        if subs[-1][1] <= P.TABLE:
            continue                                 # the whole budget stays inside the table
        last, ninl = Q.oracle_last_change(oracle, p1, p2, Kq, prob, 1.0, max_iters)
        print(name, "M", M, "final model at sample", last, "inliers", ninl, "draw", subs[last - 1][1], "to", subs[last][1])
        if subs[last][1] > P.TABLE:
            past[name] = (subs[last - 1][1], subs[P.ROUND * ((last - 1) // P.ROUND)][1])
    assert list(past) == ["past_the_table"]
    start, round_start = past["past_the_table"]
    assert start >= P.TABLE + P.WINDOW_E and round_start >= P.TABLE        # a whole round of 64 samples past it
    assert Q.RANSAC_REACH["past_the_table"] == (1509, 1509)

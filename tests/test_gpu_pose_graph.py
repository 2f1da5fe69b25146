"""GPU: k_pose_graph (vo_pose_graph, vo_pose_graph_batch) against the numpy checker tests/pose_graph_reference.py, as
tests/test_gpu_bundle_adjust.py holds the bundle adjustment: status, iterations_run and trials_run equal; estimates and chi2 within
100 x the checker's own order floor for that case (its dense solve as given against a seeded permutation of the unknowns), floored
at 1e-12 relative.  The graphs are the smallest at which each path of the kernel can go wrong (pose_graph_reference.SMALL_CASES):
one edge; one run and no separator; a loop to the fixed vertex; adjacent separators with an empty run between them and a shared one;
a fixed vertex in the middle; every free vertex a separator; a duplicated chain edge; weights per component; Huber against a wrong
loop edge; runs longer than the workgroup (N = 300); the separator system at capacity (N = 70, 32 loops: 64 separators, factored in
the call's scratch where the smaller ones are factored in LDS).

Every case is compared at pose_graph_reference.decisive_iterations(), the count in SMALL_CASES (the reason is stated there: past it a
run accepts or rejects by the last bit of chi2, differently in any two summation orders, and ends up to 1e-10 away).  Order floors of
the checker there (largest difference between its two solve orders), and what the kernel showed on an MI355X:
    case                    it   s         R         t         chi2        |gpu - checker| s, R, t, chi2
    pair                     3   0         0         0         0           0 6.8e-19 1.6e-17 7.1e-36
    chain5                   8   1.1e-16   2.2e-16   5.3e-15   1.1e-30     1.1e-16 3.3e-16 3.6e-15 2.4e-29
    loop_to_fixed            4   3.3e-16   1.1e-16   7.1e-15   2.6e-19     2.2e-16 3.3e-16 5.3e-15 5.9e-19
    adjacent_separators      7   4.4e-16   3.3e-16   8.9e-15   2.6e-19     8.9e-16 3.3e-16 1.1e-14 3.6e-19
    fixed_in_the_middle      5   2.2e-16   3.5e-16   5.3e-15   1.4e-18     2.2e-16 2.2e-16 3.6e-15 1.9e-18
    complete6                3   0         4.4e-16   3.6e-15   4.8e-19     2.2e-16 5.6e-16 3.6e-15 2.8e-18
    duplicated_chain_edge    4   2.2e-16   3.1e-16   4.1e-15   9.0e-19     2.2e-16 3.3e-16 5.1e-15 3.5e-19
    weights                  6   2.2e-16   3.3e-16   2.6e-15   4.9e-17     6.7e-16 3.3e-16 7.1e-15 3.3e-17
    huber_wrong_loop         6   3.3e-16   7.8e-16   5.3e-15   8.3e-17     2.2e-16 4.4e-16 7.1e-15 2.1e-17
    n300                    10   4.1e-14   9.1e-14   9.6e-13   3.9e-19     5.0e-14 3.3e-14 6.5e-13 9.6e-19
    capacity                 9   2.6e-15   2.9e-15   4.8e-14   3.1e-18     3.2e-15 3.8e-15 4.9e-14 7.6e-18
Only where the final chi2 is a cancellation residue (a graph without loop edges fits exactly: pair, chain5; or chi2_final < 1e-24)
chi2's bound is also never below pose_graph_reference.chi2_rounding: 1e-28 left of terms of 1e-3 is known to no order to 1e-12 of
itself (pair: floor 0, chi2 3e-30).  Every other case keeps 100 x floor, floored at 1e-12 relative."""
import numpy as np
import pytest

import pose_graph_reference as P

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(name):
    """(graph, huber_delta, iterations, checker run, tolerances), computed once per module"""
    if name not in _CACHE:
        mk, delta, iters = P.SMALL_CASES[name]
        g = mk()
        ref, floor, same, other = P.order_floor(P.args(g), iters, delta)
        assert same and ref["trials"] == other["trials"], f"{name}: the checker's two orders disagree at {iters} iterations; no parity case"
        print(f"order floor {name} it={iters}: " + " ".join(f"{k}={v:.1e}" for k, v in floor.items()))
        _CACHE[name] = (g, delta, iters, ref, P.tolerances(ref, floor, g["edges"], g["info"]))
    return _CACHE[name]


def _compare(name, got, ref, tol):
    assert (got["status"], got["iterations"], got["trials"]) == (ref["status"], ref["iterations"], ref["trials"]), name
    assert abs(got["chi2_initial"] - ref["chi2_initial"]) <= 1e-12 * abs(ref["chi2_initial"]), name
    q, r = P.quantities(got["sims"], got["chi2_final"]), P.quantities(ref["sims"], ref["chi2_final"])
    for k in q:
        err = float(np.abs(q[k] - r[k]).max())
        print(f"{name} {k}: |gpu - checker| = {err:.2e}, bound {tol[k]:.2e}")
        assert err <= tol[k], (name, k, err, tol[k])


@pytest.mark.parametrize("name", list(P.SMALL_CASES))
def test_parity_with_the_checker(name):
    from visual_odometry_amd import map_filters
    g, delta, iters, ref, tol = _case(name)
    got = map_filters.optimize_pose_graph(*P.args(g), iterations=iters, huber_delta=delta)
    _compare(name, got, ref, tol)
    fixed = g["fixed"].astype(bool)
    assert np.array_equal(got["sims"][fixed], g["sims"][fixed]), "a fixed vertex keeps its input bytes"
    assert got["chi2_final"] <= got["chi2_initial"]


def test_one_batched_call_holds_them_all():
    """All graphs in one launch, an over-capacity graph (33 loop edges) and an invalid one between them: theirs come back unchanged
    with their own status, the neighbours' bytes equal their stand-alone runs; and a second call returns the same bytes."""
    from visual_odometry_amd import _lib, map_filters
    names = list(P.SMALL_CASES)
    same_opts = [n for n in names if P.SMALL_CASES[n][1] == 0.0]
    graphs = {n: P.SMALL_CASES[n][0]() for n in same_opts}
    over, bad = P.over_capacity(), P.invalid_graph()
    problems = [P.args(graphs[n]) for n in same_opts[:3]] + [P.args(over)] + [P.args(graphs[n]) for n in same_opts[3:6]] + [P.args(bad)] \
        + [P.args(graphs[n]) for n in same_opts[6:]]
    order = same_opts[:3] + ["over"] + same_opts[3:6] + ["bad"] + same_opts[6:]
    out = map_filters.optimize_pose_graph_batch(problems, iterations=10)
    again = map_filters.optimize_pose_graph_batch(problems, iterations=10)
    for name, o, a in zip(order, out, again):
        assert o["sims"].tobytes() == a["sims"].tobytes() and (o["chi2_final"], o["trials"]) == (a["chi2_final"], a["trials"]), name
        if name == "over":
            assert o["status"] == _lib.VO_ERR_UNSUPPORTED and o["sims"].tobytes() == over["sims"].tobytes() and o["trials"] == 0
        elif name == "bad":
            assert o["status"] == _lib.VO_ERR_INVALID and o["sims"].tobytes() == bad["sims"].tobytes() and o["trials"] == 0
        else:
            alone = map_filters.optimize_pose_graph(*P.args(graphs[name]), iterations=10)
            assert o["status"] == 0 and o["sims"].tobytes() == alone["sims"].tobytes(), name
            assert (o["chi2_initial"], o["chi2_final"], o["iterations"], o["trials"]) == (alone["chi2_initial"], alone["chi2_final"], alone["iterations"], alone["trials"]), name


def test_huber_in_a_batched_call():
    """huber_delta is an option of the call: the wrong-loop case between two neighbours, all three under Huber, equal their
    stand-alone runs under Huber byte for byte, and the wrong-loop case equals the checker's."""
    from visual_odometry_amd import map_filters
    mk, delta, iters = P.SMALL_CASES["huber_wrong_loop"]
    names = ["loop_to_fixed", "huber_wrong_loop", "adjacent_separators"]
    graphs = [P.SMALL_CASES[n][0]() for n in names]
    out = map_filters.optimize_pose_graph_batch([P.args(g) for g in graphs], iterations=iters, huber_delta=delta)
    for name, g, o in zip(names, graphs, out):
        alone = map_filters.optimize_pose_graph(*P.args(g), iterations=iters, huber_delta=delta)
        assert o["status"] == 0 and o["sims"].tobytes() == alone["sims"].tobytes(), name
        assert (o["chi2_initial"], o["chi2_final"], o["iterations"], o["trials"]) == (alone["chi2_initial"], alone["chi2_final"], alone["iterations"], alone["trials"]), name
    _, _, _, ref, tol = _case("huber_wrong_loop")
    _compare("huber_wrong_loop in a batch", out[1], ref, tol)
    plain = map_filters.optimize_pose_graph(*P.args(graphs[1]), iterations=iters)
    assert plain["sims"].tobytes() != out[1]["sims"].tobytes(), "Huber changes the wrong-loop case"


def test_the_single_call_refuses_what_the_batch_marks():
    from visual_odometry_amd import _lib, map_filters
    with pytest.raises(NotImplementedError):
        map_filters.optimize_pose_graph(*P.args(P.over_capacity()))
    with pytest.raises(_lib.VoError):
        map_filters.optimize_pose_graph(*P.args(P.invalid_graph()))
    g = P.SMALL_CASES["chain5"][0]()
    with pytest.raises(_lib.VoError):
        map_filters.optimize_pose_graph(*P.args(g), iterations=0)


def test_a_closed_course_ends_nearer_the_truth():
    """End to end through the frontend helpers: N = 60 on a closed course, odometry with noise and 1 % scale drift per step (the
    track is its dead reckoning, so every chain edge starts at zero error), two true loop edges.  The device's result has a smaller
    mean camera-centre error than the start."""
    from visual_odometry_amd import frontend, map_filters
    n = 60
    truth = P.course(n, wobble=0.02, seed=41)
    track = P.drifted(truth, 41, scale_drift=0.01, rot=0.003, trans=0.02)
    edges, meas = frontend.odometry_edges(track)
    for i, j in [(0, 59), (10, 50)]:
        edges = np.vstack([edges, [[i, j]]]).astype(np.int32)
        meas = np.vstack([meas, frontend.loop_edge(truth[i], truth[j])[None]])
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    r = map_filters.optimize_pose_graph(track, fixed, edges, meas, iterations=10)
    centres = lambda V: -np.einsum("nji,nj->ni", frontend.vertices_to_poses(V)[:, :, :3], frontend.vertices_to_poses(V)[:, :, 3])  # noqa: E731
    before = float(np.linalg.norm(centres(track) - centres(truth), axis=1).mean())
    after = float(np.linalg.norm(centres(r["sims"]) - centres(truth), axis=1).mean())
    print(f"mean camera-centre error: {before:.4f} before, {after:.4f} after")
    assert r["status"] == 0 and after < before

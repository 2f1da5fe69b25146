"""GPU: k_sim3_ransac behind vo_sim3_ransac_batch (geometry.estimate_similarity[_batch]) against tests/map_align_reference.py on
correspondences the test CHOSE.  tests/test_map_align_reference.py establishes on the CPU that in no hypothesis the checker consumes
a squared error comes within 1e-6 (relative) of the bound, so status, n_inl and the inlier masks are required EQUAL; (s, R, t) is
held to MARGIN = 100 times the checker's own largest error against the generating similarity on the exact family (measured on the
CPU: s 1.8e-15, R 5.6e-15, t 2.1e-14; the figures are printed by the tests and recorded in docs/kernels/k_sim3_ransac.md).

Held here:
  family    n / outliers = 3/0, 4/1, 5/2, 63/20, 64/32, 65/40, 257/128, 300/210, 1000/800, 2000/1700, 300/100 coplanar, exact data,
            scale 0.25 or 4, max_error 0.1: in ONE batched call with the noisy case (default seed), and every case alone with
            seed = n (redraws at n = 4 and 5, rejected samples, a stop in the second round of 64, the whole budget of 1000 with
            3002 random numbers);
  noisy     Gaussian noise of 0.004 per axis: the device's transform against the checker's, same bound;
  branches  n = 0, 1, 2 -> VO_ERR_TOO_FEW; a collinear triple, 40 identical points, 7 collinear points (every sample rejected) ->
            VO_ERR_NO_MODEL, each between good problems whose bytes do not change; 3100 correspondences (past the LDS staging
            path); min_inliers above and at the count; iterations 1 and 65; another seed;
  bytes     two calls on the same input return the same bytes; every refusal leaves the context able to repeat them."""
import numpy as np
import pytest

import map_align_reference as A

pytestmark = pytest.mark.gpu


def _batch(ctx, problems, **opts):
    """problems: [(src, dst)] -> the device's dict with mask split per problem"""
    from visual_odometry_amd import geometry
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.int32)
    src = np.concatenate([np.asarray(s, np.float64).reshape(-1, 3) for s, _ in problems])
    dst = np.concatenate([np.asarray(d, np.float64).reshape(-1, 3) for _, d in problems])
    out = geometry.estimate_similarity_batch(src, dst, off, opts.pop("max_error", A.MAX_ERROR), ctx=ctx, **opts)
    out["masks"] = [out["mask"][off[k]:off[k + 1]] for k in range(len(problems))]
    return out


def _bound():
    ce = A.checker_error()
    return tuple(A.MARGIN * v for v in ce)


def _equal(out, k, ref, what):
    """status, n_inl and the mask EQUAL the checker's; a failed problem's model is zeros"""
    assert out["status"][k] == ref["status"], (what, int(out["status"][k]), ref["status"])
    assert out["n_inl"][k] == ref["n_inl"], (what, int(out["n_inl"][k]), ref["n_inl"])
    assert out["masks"][k].dtype == np.uint8 and np.array_equal(out["masks"][k], ref["mask"]), what
    if ref["status"] != 0:
        assert out["scale"][k] == 0 and not out["R"][k].any() and not out["t"][k].any(), what


def _close(out, k, want, what):
    err = A.model_error((out["scale"][k], out["R"][k], out["t"][k]), want)
    bound = _bound()
    print(what, "device error  s %.2e  R %.2e  t %.2e   bound  s %.2e  R %.2e  t %.2e" % (err + bound))
    assert all(e <= b for e, b in zip(err, bound)), (what, err, bound)
    return err


def test_the_family_and_the_noisy_case_in_one_batched_call(ctx):
    runs = A.family_runs(False)
    noisy = A.noisy_case()
    ref_noisy = A.sim3_ransac(noisy["src"], noisy["dst"], noisy["max_error"])
    assert ref_noisy["nearest"] > A.PREMISE
    out = _batch(ctx, [(c["src"], c["dst"]) for c, _ in runs] + [(noisy["src"], noisy["dst"])])
    print("the checker's own error  s %.2e  R %.2e  t %.2e" % A.checker_error())
    worst = np.zeros(3)
    for k, (c, r) in enumerate(runs):
        what = "family n=%d" % len(c["src"])
        _equal(out, k, r, what)
        worst = np.maximum(worst, _close(out, k, c["model"], what))
    print("the device's largest error against the generating similarity  s %.2e  R %.2e  t %.2e" % tuple(worst))
    k = len(runs)
    _equal(out, k, ref_noisy, "noisy")
    print("noisy: the checker's distance to the generating similarity  s %.2e  R %.2e  t %.2e"
          % A.model_error((ref_noisy["scale"], ref_noisy["R"], ref_noisy["t"]), noisy["model"]))
    _close(out, k, (ref_noisy["scale"], ref_noisy["R"], ref_noisy["t"]), "noisy against the checker")
    # the same input, the same bytes
    again = _batch(ctx, [(c["src"], c["dst"]) for c, _ in runs] + [(noisy["src"], noisy["dst"])])
    for key in ("status", "scale", "R", "t", "n_inl", "mask"):
        assert out[key].tobytes() == again[key].tobytes(), key


def test_every_family_case_alone_under_seed_n(ctx):
    for c, r in A.family_runs(True):
        what = "alone n=%d seed=%d iters=%d" % (len(c["src"]), c["seed"], r["iters"])
        out = _batch(ctx, [(c["src"], c["dst"])], seed=c["seed"])
        _equal(out, 0, r, what)
        _close(out, 0, c["model"], what)


def test_failing_problems_between_good_ones(ctx):
    cases = A.branch_cases()
    good = cases["default_seed"][:2]
    order = ["g", "n0", "g", "n1", "n2", "n3_collinear", "g", "identical", "collinear", "g"]
    out = _batch(ctx, [good if k == "g" else cases[k][:2] for k in order])
    ref_good = A.sim3_ransac(*good, A.MAX_ERROR)
    alone = _batch(ctx, [good])
    for k, name in enumerate(order):
        if name == "g":
            _equal(out, k, ref_good, "good at %d" % k)
            for key in ("scale", "R", "t"):
                assert out[key][k].tobytes() == alone[key][0].tobytes(), (k, key)          # a failed neighbour does not touch it
            assert out["masks"][k].tobytes() == alone["masks"][0].tobytes()
        else:
            s, d, o, want = cases[name]
            ref = A.sim3_ransac(s, d, A.MAX_ERROR, **o)
            assert ref["status"] == want
            _equal(out, k, ref, name)


@pytest.mark.parametrize("name", ("past_lds", "min_inliers_above", "min_inliers_met", "iterations_1", "iterations_65", "other_seed"))
def test_the_other_branches(ctx, name):
    s, d, o, want = A.branch_cases()[name]
    ref = A.sim3_ransac(s, d, A.MAX_ERROR, **o)
    assert ref["nearest"] > A.PREMISE and (want is None or ref["status"] == want)
    out = _batch(ctx, [(s, d)], **o)
    print(name, "status", int(out["status"][0]), "n_inl", int(out["n_inl"][0]), "checker iters", ref["iters"])
    _equal(out, 0, ref, name)
    if ref["status"] == 0:
        _close(out, 0, (ref["scale"], ref["R"], ref["t"]), name + " against the checker")


def test_the_single_problem_entry_and_the_refusals(ctx):
    from visual_odometry_amd import _lib, geometry
    c = A.family_case(64, 32, 4.0)
    ref = A.sim3_ransac(c["src"], c["dst"], c["max_error"])
    one = geometry.estimate_similarity(c["src"], c["dst"], c["max_error"], ctx=ctx)
    assert one["status"] == 0 and one["n_inl"] == ref["n_inl"] and np.array_equal(one["mask"], ref["mask"]) and one["R"].shape == (3, 3)
    first = _batch(ctx, [(c["src"], c["dst"])])
    assert one["R"].tobytes() == first["R"][0].tobytes() and one["scale"] == first["scale"][0] and one["t"].tobytes() == first["t"][0].tobytes()
    for bad in (dict(max_error=0.0), dict(max_error=-1.0), dict(max_error=float("nan")), dict(confidence=1.0), dict(confidence=0.0)):
        with pytest.raises(_lib.VoError) as e:
            _batch(ctx, [(c["src"], c["dst"])], **bad)
        assert e.value.code == _lib.VO_ERR_INVALID, bad
        again = _batch(ctx, [(c["src"], c["dst"])])
        for key in ("status", "scale", "R", "t", "n_inl", "mask"):
            assert first[key].tobytes() == again[key].tobytes(), (bad, key)
    with pytest.raises(_lib.VoError) as e:
        geometry.estimate_similarity_batch(c["src"], c["dst"], [0, 40, 30, 64], 0.1, ctx=ctx)
    assert e.value.code == _lib.VO_ERR_INVALID
    empty = geometry.estimate_similarity_batch(np.zeros((0, 3)), np.zeros((0, 3)), [0], 0.1, ctx=ctx)
    assert len(empty["status"]) == 0

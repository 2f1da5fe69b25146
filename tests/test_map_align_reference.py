"""CPU: tests/map_align_reference.py — the statement vo_sim3_ransac_batch and vo_map_align are held to on the GPU
(tests/test_gpu_sim3.py, tests/test_gpu_map_align.py) — against first principles; the premise of those tests (no squared error
within 1e-6 of the bound, relative, in any hypothesis the checker consumes) on every chosen case; the pure helpers
frontend.apply_similarity / join_segments against algebraic identities; and the header against the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_align_reference as A
import relocalize_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(r):
    return r["scale"], r["R"], r["t"]


def test_the_closed_form_recovers_a_generating_similarity_on_both_branches_of_S():
    rng = np.random.default_rng(1)
    branches = set()
    for k in range(200):
        R = RR.rotation(rng.normal(size=3), rng.uniform(0.1, 3.0)); t = rng.uniform(-5, 5, 3); s = float(rng.uniform(0.1, 8))
        b = rng.uniform(-20, 20, (3 if k % 2 else 12, 3))
        a = s * (b @ R.T) + t
        got = A.fit(b, a)
        ds, dR, dt = A.model_error(got, (s, R, t))
        assert ds < 1e-12 and dR < 1e-12 and dt < 1e-11, (k, ds, dR, dt)
        assert abs(np.linalg.det(got[1]) - 1) < 1e-12
        if len(b) == 3:                                      # rank-2 H: which sign S took is up to the SVD's third vectors
            m = len(b); H = (a - a.mean(0)).T @ (b - b.mean(0)) / m
            U, _, Vt = np.linalg.svd(H)
            branches.add(bool(np.linalg.det(U) * np.linalg.det(Vt) < 0))
    assert branches == {False, True}                         # about half of all three-point samples: not a corner case
    assert A.fit(np.zeros((5, 3)), rng.uniform(-1, 1, (5, 3))) is None            # var_b == 0
    line = np.outer(np.arange(3.0), [1.0, 2.0, 3.0])
    assert A.minimal(line, line) is None and A.minimal(rng.uniform(-1, 1, (3, 3)), line) is None
    two = np.array([[0.0, 0, 0], [0, 0, 0], [1, 0, 0]])
    assert not A.side_ok(two) and A.side_ok(np.eye(3))
    # 0.996: 5.1 degrees between the difference vectors is refused, 5.2 degrees passes
    for deg, ok in ((5.1, False), (5.2, True)):
        th = np.radians(deg)
        assert A.side_ok(np.array([[0.0, 0, 0], [1, 0, 0], [np.cos(th), np.sin(th), 0]])) == ok


def test_the_rng_stream_is_opencvs():
    # cv::RNG(0xffffffff... default state 2^64 - 1): state' = (uint32)state * 4164903690 + (state >> 32)
    st = 0xFFFFFFFFFFFFFFFF
    want = []
    for _ in range(3):
        st = ((st & 0xFFFFFFFF) * 4164903690 + (st >> 32)) % (1 << 64)
        want.append(st % (1 << 32))
    assert A.rng_stream(A.DEFAULT_SEED, 3) == want and A.rng_stream(0, 2) == A.rng_stream(0xFFFFFFFF, 2)
    assert A.update_num_iters(0.99, 0.5, 3, 1000) == 34 and A.update_num_iters(0.99, 0.0, 3, 1000) == 0
    assert A.update_num_iters(0.99, 1.0, 3, 1000) == 1000


def _runs():
    """(name, case, run) for every problem the GPU tests send: the family under seed = n and under the default seed, the noisy
    case, the branch cases."""
    out = []
    for f, c in zip(A.FAMILY, A.family()):
        out.append((f"family{f}/seed=n", c, A.sim3_ransac(c["src"], c["dst"], c["max_error"], seed=c["seed"])))
        out.append((f"family{f}/default", c, A.sim3_ransac(c["src"], c["dst"], c["max_error"])))
    c = A.noisy_case()
    out.append(("noisy", c, A.sim3_ransac(c["src"], c["dst"], c["max_error"])))
    for name, (s, d, o, want) in A.branch_cases().items():
        out.append((name, dict(want=want), A.sim3_ransac(s, d, A.MAX_ERROR, **o)))
    return out


@pytest.fixture(scope="module")
def runs():
    return _runs()


def test_the_premise_holds_on_every_chosen_case(runs):
    nearest = min(r["nearest"] for _, _, r in runs)
    print("nearest approach of e / max_error^2 to 1 over every consumed hypothesis of every case:", nearest)
    for name, _, r in runs:
        assert r["nearest"] > A.PREMISE, (name, r["nearest"])


def test_the_family_recovers_its_similarity_and_its_outliers(runs):
    worst = np.zeros(3)
    for name, c, r in runs:
        if not name.startswith("family"):
            continue
        assert r["status"] == A.VO_OK and np.array_equal(r["mask"] > 0, ~c["outlier"]), name
        assert r["n_inl"] == int((~c["outlier"]).sum())
        worst = np.maximum(worst, A.model_error(_model(r), c["model"]))
    print("the checker's own error against the generating similarity on exact data: s %.2e  R %.2e  t %.2e" % tuple(worst))
    assert worst[0] < 1e-13 and worst[1] < 1e-13 and worst[2] < 1e-12


def test_the_family_reaches_what_its_sizes_are_for(runs):
    by = {name: r for name, _, r in runs}
    assert by["family(3, 0, 4.0, False)/seed=n"]["iters"] == 1 and by["family(3, 0, 4.0, False)/seed=n"]["numbers"] == 0
    assert by["family(4, 1, 0.25, False)/seed=n"]["redraws"] > 0 and by["family(5, 2, 4.0, False)/seed=n"]["redraws"] > 0
    assert sum(r["rejected"] for name, _, r in runs if name.startswith("family")) > 0          # the subset check refuses samples of random data too
    r = by["family(65, 40, 0.25, False)/seed=n"]
    assert 64 < r["iters"] < 128                                                                # the stop falls in the second round of 64
    r = by["family(2000, 1700, 0.25, False)/seed=n"]
    assert r["iters"] == 1000 and 3000 <= r["numbers"] < 8192                                   # the whole budget, inside the 8192-entry table
    assert len(by["family(1000, 800, 4.0, False)/seed=n"]["best_at"]) >= 1
    for name, c, r in runs:
        if "want" in c and c["want"] is not None:
            assert r["status"] == c["want"], name
    assert by["collinear"]["rejected"] == by["collinear"]["iters"] == 1000 and by["collinear"]["numbers"] < 8192
    assert by["identical"]["rejected"] == 1000
    assert by["min_inliers_above"]["n_inl"] == 32 and not by["min_inliers_above"]["R"].any()
    assert by["iterations_65"]["iters"] == 65 and by["iterations_1"]["iters"] == 1
    assert by["past_lds"]["n_inl"] == 2790 and len(by["past_lds"]["mask"]) > 3072
    r = by["noisy"]
    assert r["status"] == 0 and r["n_inl"] == 200


@pytest.mark.parametrize("detector", ("sift", "orb"))
def test_two_maps_of_the_same_ground_align(oracle, detector):
    for npt, n in ((257, 257), (513, 65), (3, 64), (257, 2), (513, 0)):
        c = A.align_case(detector, npt, n)
        r = A.map_align(c["map_rows"], c["map_pts"], c["rows"], c["pts"], c["max_error"])
        bi, ai, d = RR.match_map_loops(c["rows"], c["map_rows"])
        assert np.array_equal(r["bi"], bi) and np.array_equal(r["ai"], ai) and np.array_equal(r["dist"], d)
        assert np.array_equal(r["src"], c["pts"][bi]) and np.array_equal(r["dst"], c["map_pts"][ai])
        assert r["nearest"] > A.PREMISE
        if r["n_match"] < 3:
            assert r["status"] == A.VO_ERR_TOO_FEW
        elif npt >= 257 and n >= 65:
            ds, dR, dt = A.model_error(_model(r), c["model"])
            assert r["status"] == 0 and r["n_inl"] >= 0.6 * r["n_match"] and ds < 1e-12 and dR < 1e-12 and dt < 1e-11, (npt, n, ds, dR, dt)


# ------------------------------------------------------------------ the pure helpers
def _project(T, X):
    x = X @ T[:, :3].T + T[:, 3]
    return x[:, :2] / x[:, 2:]


def _sim(rng):
    return float(rng.uniform(0.2, 5)), RR.rotation(rng.normal(size=3), rng.uniform(0.1, 3)), rng.uniform(-5, 5, 3)


def test_apply_similarity_keeps_every_projection_and_scales_the_camera_frame():
    from visual_odometry_amd.frontend import apply_similarity
    rng = np.random.default_rng(5)
    s, R, t = _sim(rng)
    poses = np.stack([np.hstack([RR.rotation(rng.normal(size=3), rng.uniform(0, 1)), rng.uniform(-1, 1, (3, 1)) + [[0], [0], [8]]]) for _ in range(6)])
    X = rng.uniform(-2, 2, (50, 3))
    got = apply_similarity(poses, s, R, t)
    assert got.shape == poses.shape
    Xa = A.transform((s, R, t), X)
    for T, Ta in zip(poses, got):
        assert np.abs(_project(Ta, Xa) - _project(T, X)).max() < 1e-12
        assert np.abs((Xa @ Ta[:, :3].T + Ta[:, 3]) - s * (X @ T[:, :3].T + T[:, 3])).max() < 1e-12      # the camera frame in A's units
        assert np.abs(Ta[:, :3] @ Ta[:, :3].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Ta[:, :3]) - 1) < 1e-14
        centre, centre_a = -T[:, :3].T @ T[:, 3], -Ta[:, :3].T @ Ta[:, 3]
        assert np.abs(centre_a - A.transform((s, R, t), centre)).max() < 1e-12                         # camera centres move like points
    assert np.array_equal(apply_similarity(poses, 1.0, np.eye(3), np.zeros(3)), poses)
    assert apply_similarity(poses[0], s, R, t).shape == (3, 4)
    with pytest.raises(ValueError):
        apply_similarity(np.zeros((2, 4, 4)), s, R, t)


def test_join_segments_composes_and_reports_what_is_not_connected():
    from visual_odometry_amd.frontend import apply_similarity, compose_similarity, join_segments
    rng = np.random.default_rng(6)
    f, g, h = _sim(rng), _sim(rng), _sim(rng)
    X = rng.uniform(-3, 3, (20, 3))
    # composition: the function it says it is, and associative
    fg = compose_similarity(f, g)
    assert np.abs(A.transform(fg, X) - A.transform(f, A.transform(g, X))).max() < 1e-12
    left, right = compose_similarity(compose_similarity(f, g), h), compose_similarity(f, compose_similarity(g, h))
    assert max(A.model_error(left, right)) < 1e-12
    segs = []
    for k in range(4):
        P = np.stack([np.hstack([RR.rotation(rng.normal(size=3), 0.3), rng.uniform(-1, 1, (3, 1))]) for _ in range(3 + k)])
        segs.append(dict(first_pair=10 * k, n_pairs=2 + k, poses_pnp=P, poses=P + 0.0))
    keep = [s["poses"].copy() for s in segs]
    joined, loose = join_segments(segs, [f, dict(scale=g[0], R=g[1], t=g[2]), h])
    assert loose == [] and [j["index"] for j in joined] == [0, 1, 2, 3]
    assert np.array_equal(joined[0]["poses"], segs[0]["poses"]) and joined[0]["first_pair"] == 0
    assert np.abs(joined[1]["poses"] - apply_similarity(segs[1]["poses"], *f)).max() < 1e-13
    assert np.abs(joined[2]["poses_pnp"] - apply_similarity(apply_similarity(segs[2]["poses_pnp"], *g), *f)).max() < 1e-12
    assert np.abs(joined[3]["poses"] - apply_similarity(segs[3]["poses"], *left)).max() < 1e-12
    assert max(A.model_error(joined[3]["sim"], left)) < 1e-12
    assert all(np.array_equal(s["poses"], k) for s, k in zip(segs, keep))                      # copies: the input is left alone
    # a missing link cuts everything behind it off, a later similarity notwithstanding
    joined, loose = join_segments(segs, [f, None, h])
    assert [j["index"] for j in joined] == [0, 1] and loose == [2, 3]
    joined, loose = join_segments(segs[:1], [])
    assert len(joined) == 1 and loose == []
    assert join_segments([], []) == ([], [])
    with pytest.raises(ValueError):
        join_segments(segs, [f])


# ------------------------------------------------------------------ the ABI
def _declared(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared in include/vo_hip.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append("pointer" if "*" in a or "[" in a else a.rsplit(" ", 1)[0])
    return out


def test_the_prototypes_match_the_bindings():
    from visual_odometry_amd import _lib, frontend, geometry
    P, I = "pointer", "int"
    for name, kinds in (("vo_sim3_ransac_batch", [P, P, P, P, I, P, P, P, P, P]), ("vo_map_align", [P, P, P, P, I, P, P, P, P, P]),
                        ("vo_map_align_matches", [P, I, P, P, P, P, I, P])):
        restype, argtypes = _lib._SIGS[name]
        assert _declared(name) == kinds and restype is C.c_int
        assert [C.c_void_p if k == P else C.c_int for k in kinds] == list(argtypes)
    header = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    fields = re.search(r"typedef struct \{([^}]*)\} vo_align_opts;", header).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [n for n, _ in _lib.AlignOpts._fields_] == ["max_distance", "max_error", "iterations", "confidence", "seed", "min_inliers"]
    assert C.sizeof(_lib.AlignOpts) == 48
    assert int(re.search(r"#define\s+VO_STAGE_COUNT\s+(\d+)", header).group(1)) == _lib.VO_STAGE_COUNT == 30
    for name in ("align_maps", "map_align_matches"):
        assert callable(getattr(frontend.FrontEnd, name))
    import inspect
    assert inspect.signature(geometry.estimate_similarity).parameters["max_error"].default is inspect.Parameter.empty
    assert inspect.signature(frontend.FrontEnd.align_maps).parameters["max_error"].default is inspect.Parameter.empty

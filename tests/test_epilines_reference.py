"""CPU: the numpy checker of vo_correspond_epilines / vo_pairs_epipolar (tests/epilines_reference.py), checked by properties.
Every tolerance is derived below from float64's unit roundoff u = eps / 2 and the magnitudes involved."""
import numpy as np
import pytest

import epilines_reference as ER

EPS = np.finfo(np.float64).eps          # 2 u


def _cross(e):
    return np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0.0]])


def _exact_F():
    """F = [e2]x A with small integers: every entry is an exactly representable integer and e2^T F = 0 holds exactly, so the
    epipole test below measures the rounding of the line evaluation alone.  e1 (F e1 = 0) is A^-1 e2 up to scale; A is chosen
    with an integer inverse-times-e2."""
    e2 = np.array([37.0, -12.0, 1.0])
    A = np.array([[2.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])         # det 1: A^-1 = [[1, -1, 0], [-1, 2, 0], [0, 0, 1]]
    e1 = np.array([[1.0, -1.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]) @ e2  # integers; [e2]x A e1 = [e2]x e2 = 0
    return _cross(e2) @ A, e1, e2


def _points(n, seed=0):
    return np.random.default_rng(seed).uniform(-500, 1500, (n, 2))


def test_lines_are_unit_normals():
    # s = fl(fl(a a) + fl(b b)) carries <= 2u, sqrt halves that and adds u, the division adds u: nu is within 3u of
    # 1 / sqrt(a^2 + b^2); a nu and b nu add u each, squaring doubles: a'^2 + b'^2 = 1 + 8u at first order.  Evaluating the sum
    # here adds three more roundings.  Bound: 16 u = 8 eps.
    F, _, _ = _exact_F()
    for which in (1, 2):
        l = ER.correspond_epilines(_points(500, which), which, F)[:, 0]
        assert np.abs(l[:, 0] ** 2 + l[:, 1] ** 2 - 1.0).max() <= 8 * EPS


def test_lines_pass_through_the_epipole():
    # whichImage 1: l = nu F x lies in image 2 and contains e2 (e2^T F = 0 exactly here); whichImage 2: l = nu F^T x contains e1.
    # l . e is nu * sum_ij e_i F_ij x_j evaluated with roundings: each of the 9 terms passes through at most 6 operations
    # (product, two sums of the row, the scale by nu, the product with e_i, two sums here), each <= u relative on partial sums
    # bounded by S = nu * sum_ij |e_i| |F_ij| |x_j|.  Bound: 8 u S = 4 eps S.
    F, e1, e2 = _exact_F()
    assert np.array_equal(e2 @ F, np.zeros(3)) and np.array_equal(F @ e1, np.zeros(3))
    for which, e, M in ((1, e2, F), (2, e1, F.T)):
        p = _points(500, 10 + which)
        l = ER.correspond_epilines(p, which, F)[:, 0]
        xh = np.c_[p, np.ones(len(p))]
        raw = xh @ M.T
        nu = 1.0 / np.sqrt(raw[:, 0] ** 2 + raw[:, 1] ** 2)
        S = nu * (np.abs(xh) @ np.abs(M).T @ np.abs(e))
        assert (np.abs(l @ e) <= 4 * EPS * S).all()


def test_transpose_rule_between_the_two_images():
    F = np.random.default_rng(3).normal(size=(3, 3))
    p = _points(100, 4)
    assert np.array_equal(ER.correspond_epilines(p, 2, F), ER.correspond_epilines(p, 1, F.T))
    assert not np.array_equal(ER.correspond_epilines(p, 2, F), ER.correspond_epilines(p, 1, F))


def test_zero_norm_branch_leaves_the_line_unscaled():
    F = np.array([[0, 0, 0], [0, 0, 0], [0.5, -2.0, 3.0]])
    p = _points(50, 5)
    l = ER.correspond_epilines(p, 1, F)[:, 0]
    assert np.array_equal(l[:, :2], np.zeros((50, 2)))
    assert np.array_equal(l[:, 2], 0.5 * p[:, 0] + -2.0 * p[:, 1] + 3.0)      # nu = 1: c as computed, no inf / nan
    l2 = ER.correspond_epilines(np.array([[37.0, -12.0]]), 2, _exact_F()[0])  # a point AT the epipole e2: F^T e2 = 0 exactly
    assert np.array_equal(l2, np.zeros((1, 1, 3)))


@pytest.mark.parametrize("dtype,out", [(np.float64, np.float64), (np.float32, np.float32), (np.int32, np.float32)])
def test_output_depth_is_max_of_input_depth_and_float32(dtype, out):
    F, _, _ = _exact_F()
    p = (_points(64, 6) if dtype != np.int32 else np.rint(_points(64, 6))).astype(dtype)
    l = ER.correspond_epilines(p, 1, F)
    assert l.dtype == out and l.shape == (64, 1, 3)
    ref = ER.correspond_epilines(p.astype(np.float64), 1, F)                  # computed in float64, cast once at the end
    assert np.array_equal(l, ref.astype(out))
    assert ER.correspond_epilines(np.zeros((0, 2), dtype), 1, F).shape == (0, 1, 3)
    with pytest.raises(TypeError):
        ER.correspond_epilines(p.astype(np.int64), 1, F)


def test_pixel_fundamental_is_Kinv_T_E_Kinv():
    # against the same product through np.linalg.inv: both are a dozen roundings away from the exact product, whose terms are
    # bounded entrywise by T = |K^-T| |E| |K^-1|.  Bound: 16 u T = 8 eps T.
    rng = np.random.default_rng(7)
    E = rng.normal(size=(3, 3))
    K = np.array([[802.832, 0, 565.427], [0, 790.1, 240.124], [0, 0, 1.0]])
    Ki = np.linalg.inv(K)
    T = np.abs(Ki.T) @ np.abs(E) @ np.abs(Ki)
    assert (np.abs(ER.pixel_fundamental(E, K) - Ki.T @ E @ Ki) <= 8 * EPS * T).all()
    assert ER.k_supported(K)
    for bad in ((0, 1, 0.1), (2, 2, 2.0), (2, 0, 1e-9), (0, 0, 0.0), (1, 1, np.inf)):
        Kb = K.copy(); Kb[bad[0], bad[1]] = bad[2]
        assert not ER.k_supported(Kb)


def test_distances_and_statistics():
    # exact correspondences of a synthetic two-view scene lie on their epilines: d_k is rounding noise relative to the pixel
    # magnitudes (~1e3) -> far below 1e-6 px; displaced by 1 px along the line normal, d_k grows by about 1 + 1
    rng = np.random.default_rng(8)
    K = np.array([[700.0, 0, 320], [0, 700, 240], [0, 0, 1]])
    R = np.eye(3); t = np.array([1.0, 0.2, 0.1])
    X = np.c_[rng.uniform(-2, 2, (40, 2)), rng.uniform(4, 8, 40)]
    x1 = (K @ X.T).T; x1 = x1[:, :2] / x1[:, 2:]
    x2 = (K @ (R @ X.T + t[:, None])).T; x2 = x2[:, :2] / x2[:, 2:]
    E = _cross(t) @ R
    r = ER.pairs_epipolar(x1, x2, E, K)
    assert r["n"] == 40 and r["max"] < 1e-6 and r["dist"].shape == (40,)
    F = ER.pixel_fundamental(E, K)
    l1 = ER.correspond_epilines(x1, 1, F)[:, 0]
    x2m = x2 + l1[:, :2]                                                      # one pixel along the unit normal of its line
    moved = ER.pairs_epipolar(x1, x2m, E, K)
    # first term: 1 (the displacement); second: x2m^T F x1 = |(F x1)[:2]| over the norm of x2m's own line, |(F^T x2m)[:2]|
    n1 = np.linalg.norm((np.c_[x1, np.ones(40)] @ F.T)[:, :2], axis=1)
    n2 = np.linalg.norm((np.c_[x2m, np.ones(40)] @ F)[:, :2], axis=1)
    assert np.abs(moved["dist"] - (1.0 + n1 / n2)).max() < 1e-9               # rounding noise of ~1e3-pixel products, as above
    # sequential vs numpy's pairwise sums: n terms of size <= max, each partial sum rounded once: |difference| <= 2 n u max
    d = rng.uniform(0, 3, 1000)
    n, mean, sd, mx = ER.stats(d)
    assert n == 1000 and mx == d.max()
    assert abs(mean - np.mean(d)) <= 1000 * EPS * d.max() and abs(sd - np.std(d)) <= 1000 * EPS * d.max()
    assert ER.stats(d[:1])[1:] == (d[0], 0.0, d[0])                           # one inlier: std = 0
    assert ER.stats(d[:0]) == (0, 0.0, 0.0, 0.0)
    failed = ER.pairs_epipolar(x1, x2, E, K, status=-4)
    assert (failed["n"], failed["mean"], failed["std"], failed["max"]) == (0, 0.0, 0.0, 0.0)

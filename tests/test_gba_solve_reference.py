"""CPU: the checker of tests/test_gpu_ba_large_solve.py checked on its own (tests/gba_solve_reference.py).  The device's blocking
(panels of 48 columns, a left-looking diagonal block, a row solve, the trailing update with the panel's columns ascending) changes
no bit of the unblocked right-looking column Cholesky; that one agrees with LAPACK within what a symmetric permutation of the
system moves; the exact-integer systems factor exactly; every system built to fail stops at its chosen column."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gba_solve_reference as G  # noqa: E402

PLACES = lambda n: [0, 47, 48, 49, n - 7, n - 1]  # noqa: E731


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("L", "y", "x")) and a["fail_col"] is None and b["fail_col"] is None


@pytest.mark.parametrize("F", [1, 7, 8, 9, 16, 17, 25, 40])
def test_blocking_changes_no_bit(F):
    A, b = G.dense_spd(6 * F, seed=F)
    assert _same(G.blocked(A, b), G.right_looking(A, b))


@pytest.mark.parametrize("n", [6, 54, 102, 240])
def test_right_looking_against_lapack(n):
    A, b = G.dense_spd(n, seed=n)
    r = G.right_looking(A, b)
    x, floor = G.order_floor(A, b, n)
    d = float(np.abs(r["x"] - x).max())
    print("n", n, "floor", floor, "right_looking - lapack", d)
    assert d <= G.tolerance(x, floor)
    assert np.abs(r["L"] - np.linalg.cholesky(A)).max() < 1e-13 and np.abs(r["L"] @ r["y"] - b).max() < 1e-12


@pytest.mark.parametrize("n", [54, 102, 150, 768])
def test_integer_systems_factor_exactly(n):
    A, b, L0, s, x0 = G.integer_system(n, None, None, seed=n)
    if n > 61:                                                                                # a band wider than a panel
        assert np.count_nonzero(np.diag(L0, -60)) and not np.count_nonzero(np.diag(L0, -61))
    ref = G.right_looking(A, b)
    assert ref["fail_col"] is None
    assert ref["L"].tobytes() == (L0 * np.sqrt(s)[None]).tobytes() and ref["x"].tobytes() == x0.tobytes()
    if n <= 150:
        assert _same(G.blocked(A, b), ref)


@pytest.mark.parametrize("n", [54, 102, 150])
def test_bad_systems_stop_at_their_column(n):
    for p in PLACES(n):
        systems = [G.integer_system(n, p, 0, seed=n + p)[:2], G.integer_system(n, p, -1, seed=n + p)[:2], G.dense_indefinite(n, p, seed=n + p),
                   G.dense_nonfinite(n, p, n + p, np.inf), G.dense_nonfinite(n, p, n + p, np.nan)]
        for k, (A, b) in enumerate(systems):
            for solve in (G.right_looking, G.blocked):
                r = solve(A, b)
                assert r["fail_col"] == p and r["x"] is None, (n, p, k, solve.__name__, r["fail_col"])


def test_bad_systems_stop_at_their_column_768():
    n = 768
    for p in PLACES(n):
        for d_p in (0, -1):
            A, b = G.integer_system(n, p, d_p, seed=n + p)[:2]
            assert G.right_looking(A, b)["fail_col"] == p

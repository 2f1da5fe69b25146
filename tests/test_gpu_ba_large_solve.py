"""GPU: the blocked Cholesky of the large bundle adjustment (k_gba_panel, k_gba_update, k_gba_backsub) handed systems directly
through vo_ba_large_solve, against tests/gba_solve_reference.py (checked on its own by tests/test_gba_solve_reference.py).
  bytes     dense systems, every tile non-zero: L, y and x have the bytes of the unblocked right-looking column Cholesky.  F = 7 / 8 /
            9 straddle a panel (48 columns), 16 / 17 the trailing update's second tile row, 24 / 25 its third, 128 has 16 panels;
            the last panel is narrow at 7, 9, 17 and 25.
  exact     integer systems A = L0 diag(s) L0^T, b = A x0: L = L0 diag(sqrt s), y and x exactly, in any summation order, so a
            difference is addressing or synchronisation, not rounding; n = 3072 walks every panel and tile of the capacity.
  capacity  a dense system at n = 3072 against LAPACK within 100 x what a symmetric permutation of the system moves in LAPACK's x.
  pivots    a pivot that is 0, -1, about -1, inf or nan at the first column, the last column of panel 0, the first and second column
            of panel 1 (reached after a trailing update), inside the narrow last panel and at the last column: reported, and x, L
            and y keep the bytes they came with — also right after a good system of the same size, whose factor then lies in the
            scratch: a panel kernel that returned without raising the flag would let the back-substitution solve against it.
References are computed once per system and shared."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gba_solve_reference as G  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xFFF85EA71E5EA71E)          # a NaN no arithmetic produces
FLAG0 = -77
KINDS = ["integer_zero", "integer_minus_one", "dense_indefinite", "inf", "nan"]


def _filled(shape):
    return np.full(shape, SENTINEL, np.uint64).view(np.float64)


def _untouched(a):
    return a is None or bool(np.all(a.view(np.uint64) == SENTINEL))


def _call(ctx, A, b, n=None, factor=True, fwd=True, null=()):
    """vo_ba_large_solve on outputs prefilled with SENTINEL: (return code, x, L, y, pivot_failed)"""
    n = len(b) if n is None else n
    m = max(n, 1) if n <= 6 * 512 else 6
    x, y, L = _filled(m), _filled(m) if fwd else None, _filled((m, m)) if factor else None
    flag = np.full(1, FLAG0, np.int32)
    ptr = lambda name, a: None if a is None or name in null else a.ctypes.data  # noqa: E731
    rc = ctx.lib.vo_ba_large_solve(ctx.handle, ptr("A", A), ptr("b", b), n, ptr("x", x), ptr("L", L), ptr("y", y), ptr("flag", flag))
    return rc, x, L, y, int(flag[0])


def _first_difference(got, want):
    d = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    return None if len(d) == 0 else tuple(int(v) for v in d[0])


def _assert_factor(L, want, label):
    """the lower triangle has want's bytes, the strict upper triangle was not written"""
    low = np.tril(np.ones(L.shape, bool))
    d = _first_difference(np.where(low, L, 0.0), np.where(low, want, 0.0))
    assert d is None, f"{label}: L differs first at (row, column) {d}: {L[d]!r} vs {want[d]!r}"
    assert np.all(L.view(np.uint64)[~low] == SENTINEL), f"{label}: the upper triangle of L was written"


def _assert_vector(got, want, name, label):
    d = _first_difference(got, want)
    assert d is None, f"{label}: {name} differs first at {d}: {got[d]!r} vs {want[d]!r}"


@functools.lru_cache(maxsize=None)
def _dense(F):
    A, b = G.dense_spd(6 * F, seed=F)
    return A, b, G.right_looking(A, b)


@functools.lru_cache(maxsize=None)
def _integer(n):
    return G.integer_system(n, None, None, seed=n)


@pytest.mark.parametrize("F", [1, 7, 8, 9, 16, 17, 24, 25, 128])
def test_factor_has_the_bits_of_the_column_cholesky(ctx, F):
    A, b, ref = _dense(F)
    rc, x, L, y, failed = _call(ctx, A, b)
    assert (rc, failed) == (0, 0)
    _assert_factor(L, ref["L"], f"F = {F}")
    _assert_vector(y, ref["y"], "y", f"F = {F}")
    _assert_vector(x, ref["x"], "x", f"F = {F}")


def test_only_the_lower_triangle_is_read_and_optional_outputs(ctx):
    A, b, ref = _dense(9)
    U = np.where(np.tril(np.ones(A.shape, bool)), A, np.nan)
    rc, x, L, y, failed = _call(ctx, U, b)
    assert (rc, failed) == (0, 0)
    _assert_factor(L, ref["L"], "upper triangle nan")
    _assert_vector(x, ref["x"], "x", "upper triangle nan")
    rc, x, L, y, failed = _call(ctx, A, b, factor=False, fwd=False)              # L and y are optional
    assert (rc, failed, L, y) == (0, 0, None, None)
    _assert_vector(x, ref["x"], "x", "x alone")
    from visual_odometry_amd import map_filters as mf
    r = mf.ba_large_solve(A, b, want_factor=True)
    assert not r["pivot_failed"] and r["x"].tobytes() == ref["x"].tobytes() and r["y"].tobytes() == ref["y"].tobytes()
    assert r["L"].tobytes() == ref["L"].tobytes()                                # the wrapper's upper triangle is zero
    assert "L" not in mf.ba_large_solve(A, b)
    bad = mf.ba_large_solve(*G.integer_system(54, 49, -1, seed=3)[:2], want_factor=True)
    assert bad == dict(x=None, y=None, L=None, pivot_failed=True)


@pytest.mark.parametrize("n", [54, 102, 768, 3072])
def test_exact_integer_systems(ctx, n):
    A, b, L0, s, x0 = _integer(n)
    rc, x, L, y, failed = _call(ctx, A, b)
    assert (rc, failed) == (0, 0)
    _assert_factor(L, L0 * np.sqrt(s)[None], f"n = {n}")
    _assert_vector(y, np.sqrt(s) * (L0.T @ x0), "y", f"n = {n}")                 # L y = b in integers
    _assert_vector(x, x0, "x", f"n = {n}")


def test_capacity_dense_against_lapack(ctx):
    n = 6 * 512
    A, b = G.dense_spd(n, seed=512)
    ref, floor = G.order_floor(A, b, 512)
    tol = G.tolerance(ref, floor)
    rc, x, L, y, failed = _call(ctx, A, b)
    assert (rc, failed) == (0, 0)
    d = float(np.abs(x - ref).max())
    resid = float(np.abs(np.tril(L) @ y - b).max())
    print(f"n = {n}: max|x| {np.abs(ref).max():.3g}, order floor {floor:.2e}, tolerance {tol:.2e}, device - lapack {d:.2e}, |L y - b| {resid:.2e}")
    assert np.all(np.isfinite(x)) and d <= tol, (d, tol)


def _bad_system(kind, n, p):
    seed = n + p
    if kind == "integer_zero":
        return G.integer_system(n, p, 0, seed)[:2]
    if kind == "integer_minus_one":
        return G.integer_system(n, p, -1, seed)[:2]
    F = n // 6                                                                   # the dense ones share _dense(F) and its factor
    if kind == "dense_indefinite":
        return G.dense_indefinite(n, p, F, L=_dense(F)[2]["L"])
    return G.dense_nonfinite(n, p, F, np.inf if kind == "inf" else np.nan)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [102, 768])
def test_pivot_failures_are_reported_and_write_nothing(ctx, n, kind):
    A, b, ref = _dense(n // 6)
    rc, x, _, _, failed = _call(ctx, A, b, factor=False)                         # a finite factor of this size now lies in the scratch
    assert (rc, failed) == (0, 0) and x.tobytes() == ref["x"].tobytes()
    for p in (0, 47, 48, 49, n - 7, n - 1):
        Ab, bb = _bad_system(kind, n, p)
        rc, x, L, y, failed = _call(ctx, Ab, bb)
        assert rc == 0 and failed == 1, f"{kind}, n = {n}, column {p}: return {rc}, pivot_failed {failed}"
        assert _untouched(x) and _untouched(L) and _untouched(y), f"{kind}, n = {n}, column {p}: an output was written"


def test_a_failed_call_leaves_nothing_behind(ctx):
    """good, bad, good at one size: the bad call reports the failure, the third call returns the first one's bytes"""
    A, b, ref = _dense(17)
    first = _call(ctx, A, b)
    Ab, bb = G.integer_system(102, 49, -1, seed=5)[:2]
    rc, x, L, y, failed = _call(ctx, Ab, bb)
    assert (rc, failed) == (0, 1) and _untouched(x) and _untouched(L) and _untouched(y)
    third = _call(ctx, A, b)
    assert first[0] == third[0] == 0 and first[4] == third[4] == 0
    for k in (1, 2, 3):
        assert first[k].tobytes() == third[k].tobytes()
    _assert_vector(third[1], ref["x"], "x", "third call")


def test_refusals(ctx):
    from visual_odometry_amd import map_filters as mf, _lib
    A, b, _ = _dense(1)
    for n, code in ((0, _lib.VO_ERR_INVALID), (7, _lib.VO_ERR_INVALID), (-6, _lib.VO_ERR_INVALID), (6 * 513, _lib.VO_ERR_UNSUPPORTED)):
        rc, x, L, y, failed = _call(ctx, A, b, n=n)
        assert rc == code and failed == FLAG0 and _untouched(x) and _untouched(L) and _untouched(y), n
    for name in ("A", "b", "x", "flag"):
        rc, x, L, y, failed = _call(ctx, A, b, null=(name,))
        assert rc == _lib.VO_ERR_INVALID and failed == FLAG0 and _untouched(x) and _untouched(L) and _untouched(y), name
    assert b"vo_ba_large_solve" in ctx.lib.vo_last_error(ctx.handle)
    with pytest.raises(_lib.VoError) as e:
        mf.ba_large_solve(np.eye(7), np.ones(7))
    assert e.value.code == _lib.VO_ERR_INVALID
    with pytest.raises(_lib.VoError) as e:
        mf.ba_large_solve(np.eye(6 * 513), np.ones(6 * 513))
    assert e.value.code == _lib.VO_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        mf.ba_large_solve(np.eye(6), np.ones(12))

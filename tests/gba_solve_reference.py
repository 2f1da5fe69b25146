"""The checker of vo_ba_large_solve, the blocked Cholesky of the large bundle adjustment handed a system directly
(docs/kernels/k_bundle_adjust_large.md): the unblocked right-looking column Cholesky in numpy, whose bits the device states it
has; the same arithmetic in the device's blocking (for tests/test_gba_solve_reference.py: the blocking changes no bit); seeded
systems, dense and exact-integer, good and with a pivot that fails at a chosen column; and the order floor for sizes at which the
unblocked reference is too slow to compare bytes.  numpy rounds every product and every difference (it does not fuse), as the
kernels do under -ffp-contract=off.  A plain helper module (like tests/ba_reference.py), no test in it."""
import numpy as np

P = 48                                            # columns of a panel, rows and columns of a trailing-update tile
DBL_MAX = np.finfo(np.float64).max


def _bad(piv):
    return not (piv > 0) or not (piv <= DBL_MAX)


def _carry(A, b):
    """the lower triangle of A with b as row n: [n + 1][n]"""
    n = len(b)
    M = np.zeros((n + 1, n))
    M[:n] = np.tril(np.asarray(A, np.float64))
    M[n] = b
    return M, n


def _back(M, n):
    """L^T x = y in descending row order: x[j] = y[j] / L[j, j]; y[:j] -= L[j, :j] x[j]"""
    y = M[n].copy()
    for j in range(n - 1, -1, -1):
        y[j] = y[j] / M[j, j]
        y[:j] -= M[j, :j] * y[j]
    return y


def _result(M, n, fail):
    if fail is not None:
        return dict(L=None, y=None, x=None, fail_col=fail)
    with np.errstate(all="ignore"):
        return dict(L=M[:n].copy(), y=M[n].copy(), x=_back(M, n), fail_col=None)


def right_looking(A, b):
    """The unblocked column Cholesky, b carried as the last row: for k ascending the square root, the divide of the column
    below, the rank-one update of what lies right of it.  Stops at the first pivot that is not > 0 or not finite.
    dict(L [n][n] lower, y = L^-1 b, x, fail_col: None or that column)."""
    M, n = _carry(A, b)
    with np.errstate(all="ignore"):
        for k in range(n):
            if _bad(M[k, k]):
                return _result(M, n, k)
            M[k, k] = np.sqrt(M[k, k])
            M[k + 1:, k] /= M[k, k]
            c = M[k + 1:, k]
            M[k + 1:, k + 1:] -= np.tril(np.outer(c, c[:n - k - 1]))
    return _result(M, n, None)


def blocked(A, b):
    """right_looking's arithmetic in the device's order of work: per panel of P columns the diagonal block left-looking, column
    by column (k_gba_panel), the rows below solved against it one by one, then the trailing update, the panel's columns
    ascending (k_gba_update)."""
    M, n = _carry(A, b)
    with np.errstate(all="ignore"):
        for c0 in range(0, n, P):
            nb = min(P, n - c0)
            r0 = c0 + nb
            D = M[c0:r0, c0:r0]
            for j in range(nb):
                sjj, col = D[j, j], D[j + 1:, j].copy()
                for k in range(j):
                    sjj = sjj - D[j, k] * D[j, k]
                    col -= D[j + 1:, k] * D[j, k]
                if _bad(sjj):
                    return _result(M, n, c0 + j)
                D[j, j] = np.sqrt(sjj)
                D[j + 1:, j] = col / D[j, j]
            R = M[r0:, c0:r0]
            for j in range(nb):
                s = R[:, j].copy()
                for k in range(j):
                    s -= R[:, k] * D[j, k]
                R[:, j] = s / D[j, j]
            for k in range(nb):
                c = M[r0:, c0 + k]
                M[r0:, r0:] -= np.tril(np.outer(c, c[:n - r0]))
    return _result(M, n, None)


# ---------------------------------------------------------------- seeded systems
def dense_spd(n, seed):
    """M M^T / n + I and a normal b: every tile of the factorisation is non-zero"""
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(n, n))
    return M @ M.T / n + np.eye(n), rng.normal(size=n)


def integer_system(n, p, d_p, seed):
    """A = L0 diag(s) L0^T and b = A x0 in integers: L0 unit lower triangular with entries in -2 .. 2 inside a band of 60 (wider
    than a panel), s from {1, 4, 9}, x0 in -3 .. 3.  Every intermediate of the Cholesky and of both substitutions is an integer
    far below 2^53, whatever the order of the subtractions: the factor is exactly L0 diag(sqrt s) and x exactly x0.  With
    p given, s[p] = d_p (0 or -1): the pivot of column p is exactly d_p and the columns before it are as without.
    Returns A, b, L0, s, x0 (float64, all integers)."""
    rng = np.random.default_rng(seed)
    L0 = np.tril(rng.integers(-2, 3, (n, n)), -1).astype(np.float64)
    i, j = np.indices((n, n))
    L0[i - j > 60] = 0
    L0 += np.eye(n)
    s = rng.choice(np.array([1.0, 4.0, 9.0]), n)
    if p is not None:
        s[p] = d_p
    x0 = rng.integers(-3, 4, n).astype(np.float64)
    A = (L0 * s[None]) @ L0.T                     # integers below 2^53 throughout: exact in float64 in any order
    b = A @ x0
    assert np.abs(A).max() < 2 ** 20 and np.abs(b).max() < 2 ** 30
    return A, b, L0, s, x0


def dense_indefinite(n, p, seed, L=None):
    """dense_spd with A[p, p] lowered to sum_k L[p, k]^2 - 1 (L: the reference factor of dense_spd(n, seed), computed here
    unless given): the pivot of column p is about -1"""
    A, b = dense_spd(n, seed)
    if L is None:
        L = right_looking(A, b)["L"]
    A[p, p] = float(np.sum(L[p, :p] ** 2)) - 1.0
    return A, b


def dense_nonfinite(n, p, seed, value):
    """dense_spd with A[p, p] = inf or nan: the pivot of column p is not finite"""
    A, b = dense_spd(n, seed)
    A[p, p] = value
    return A, b


# ---------------------------------------------------------------- the order floor, where bytes are out of reach
def lapack_solve(A, b):
    L = np.linalg.cholesky(A)
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def order_floor(A, b, seed):
    """A x = b by LAPACK as given and under a seeded symmetric permutation P A P^T: the first x and the largest difference of
    the two, i.e. what the order of the elimination alone moves."""
    x = lapack_solve(A, b)
    q = np.random.default_rng(2000 + seed).permutation(len(b))
    xq = np.empty_like(x)
    xq[q] = lapack_solve(A[np.ix_(q, q)], b[q])
    return x, float(np.abs(x - xq).max())


def tolerance(x, floor):
    """ba_reference.tolerances' rule: 100 x the order floor, floored at 1e-12 relative to the largest magnitude"""
    return max(100 * floor, 1e-12 * float(np.abs(x).max()))

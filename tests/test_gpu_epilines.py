"""GPU: vo_correspond_epilines (k_epilines) against the numpy checker, byte for byte: the kernel makes the same IEEE operations
in the same order (-ffp-contract=off), and float64 division and sqrt are correctly rounded on the device, as k_reprojection's
bit-exact test already relies on."""
import numpy as np
import pytest

import epilines_reference as ER
from visual_odometry_amd import geometry

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 257)             # wavefront and block edges (64 lanes per block), more than one block
DTYPES = (np.float64, np.float32, np.int32)


def _F():
    return np.array([[1.3e-6, -4.1e-5, 0.011], [3.9e-5, 2.2e-6, -0.027], [-0.012, 0.024, 1.0]])


def _points(n, dtype, seed):
    p = np.random.default_rng(seed).uniform(-200, 1400, (n, 2))
    return np.rint(p).astype(dtype) if dtype == np.int32 else p.astype(dtype)


@pytest.fixture(scope="module")
def expected():
    """The checker's lines for every (N, dtype, whichImage), computed once."""
    return {(n, dt, which): ER.correspond_epilines(_points(n, dt, n), which, _F()) for n in SIZES for dt in DTYPES for which in (1, 2)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [1, 2])
def test_lines_equal_the_checker(ctx, expected, dtype, which):
    for n in SIZES:
        got = geometry.computeCorrespondEpilines(_points(n, dtype, n), which, _F(), ctx=ctx)
        want = expected[(n, dtype, which)]
        assert got.shape == (n, 1, 3) and got.dtype == want.dtype
        assert np.array_equal(got, want), (n, np.abs(got.astype(np.float64) - want).max())


def test_zero_norm_and_epipole(ctx):
    F0 = np.array([[0, 0, 0], [0, 0, 0], [0.5, -2.0, 3.0]])                  # a = b = 0 for every point: nu = 1
    for dt in DTYPES:
        p = _points(65, dt, 5)
        got = geometry.computeCorrespondEpilines(p, 1, F0, ctx=ctx)
        assert np.array_equal(got, ER.correspond_epilines(p, 1, F0)) and np.isfinite(got).all() and not got[:, 0, :2].any()
    e2 = np.array([37.0, -12.0, 1.0])                                        # F = [e2]x A, integers: F^T e2 = 0 exactly
    F = np.array([[0, -e2[2], e2[1]], [e2[2], 0, -e2[0]], [-e2[1], e2[0], 0.0]]) @ np.array([[2.0, 1, 0], [1, 1, 0], [0, 0, 1]])
    p = np.array([[37.0, -12.0], [5.0, 6.0]])
    got = geometry.computeCorrespondEpilines(p, 2, F, ctx=ctx)
    assert np.array_equal(got, ER.correspond_epilines(p, 2, F)) and not got[0].any() and got[1].any()


def test_input_forms(ctx):
    big = _points(2 * 257, np.float64, 9)
    view = big[::2]                                                          # non-contiguous rows
    assert not view.flags.c_contiguous
    want = ER.correspond_epilines(np.ascontiguousarray(view), 1, _F())
    assert np.array_equal(geometry.computeCorrespondEpilines(view, 1, _F(), ctx=ctx), want)
    assert np.array_equal(geometry.computeCorrespondEpilines(view.reshape(-1, 1, 2), 1, _F(), ctx=ctx), want)
    assert np.array_equal(geometry.computeCorrespondEpilines([tuple(r) for r in view[:7].tolist()], 1, _F(), ctx=ctx), want[:7])   # the script's list of kp.pt
    cols = np.asfortranarray(np.ascontiguousarray(view).astype(np.float32))  # column-major float32
    assert np.array_equal(geometry.computeCorrespondEpilines(cols, 2, _F().T.copy().T, ctx=ctx), ER.correspond_epilines(np.ascontiguousarray(cols), 2, _F()))
    with pytest.raises(NotImplementedError):
        geometry.computeCorrespondEpilines(np.ones((4, 3)), 1, _F(), ctx=ctx)
    with pytest.raises(ValueError):
        geometry.computeCorrespondEpilines(view, 3, _F(), ctx=ctx)

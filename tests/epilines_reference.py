"""numpy restatement of vo_correspond_epilines and vo_pairs_epipolar (include/vo_hip.h): elementwise float64, the order of
operations written out (every `*` and `+` below is one IEEE rounding, evaluated left to right, no fused multiply-add), sums as
sequential loops from 0.0 (seq_sum, as tests/ba_reference.py).  Not a cv2 run: what OpenCV 4.7's computeCorrespondEpilines does
is restated here from its source as remembered, and parity with a cv2 build is unpinned."""
import numpy as np

POINT_TYPES = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2}


def seq_sum(v):
    t = 0.0
    for x in np.asarray(v, np.float64).tolist():
        t += x
    return t


def _lines64(x, y, f):
    """x, y [N] float64, f: 9 floats (already transposed for whichImage 2) -> (a, b, c) each [N] float64, normalised."""
    f = [np.float64(v) for v in np.asarray(f, np.float64).ravel()]
    a = f[0] * x + f[1] * y + f[2]
    b = f[3] * x + f[4] * y + f[5]
    c = f[6] * x + f[7] * y + f[8]
    nu = a * a + b * b
    with np.errstate(divide="ignore"):
        nu = np.where(nu != 0.0, np.float64(1.0) / np.sqrt(nu), np.float64(1.0))
    return a * nu, b * nu, c * nu


def correspond_epilines(points, which_image, F):
    """points [N, 2] float64 / float32 / int32 -> lines [N, 1, 3]: float64 for float64 points, float32 otherwise (the values
    are computed in float64 and cast once at the end)."""
    p = np.asarray(points)
    if p.dtype not in POINT_TYPES:
        raise TypeError("points must be float64, float32 or int32")
    p = p.reshape(-1, 2)
    F = np.asarray(F, np.float64).reshape(3, 3)
    if which_image == 2:
        F = F.T
    elif which_image != 1:
        raise ValueError("whichImage must be 1 or 2")
    x = p[:, 0].astype(np.float64); y = p[:, 1].astype(np.float64)
    a, b, c = _lines64(x, y, F.ravel())
    out = np.stack([a, b, c], axis=1).reshape(-1, 1, 3)
    return out if p.dtype == np.float64 else out.astype(np.float32)


def pixel_fundamental(E, K):
    """F = K^-T E K^-1 with K^-1 as the pair path normalises pixels (k_match_select / k_prepare_points: xn = px ifx + bx):
    only K[0, 0], K[1, 1], K[0, 2], K[1, 2] are read."""
    E = np.asarray(E, np.float64).reshape(3, 3); K = np.asarray(K, np.float64).reshape(3, 3)
    ifx = np.float64(1.0) / K[0, 0]; ify = np.float64(1.0) / K[1, 1]
    bx = -K[0, 2] * ifx; by = -K[1, 2] * ify
    G = np.zeros((3, 3)); F = np.zeros((3, 3))
    for r in range(3):
        G[r, 0] = E[r, 0] * ifx
        G[r, 1] = E[r, 1] * ify
        G[r, 2] = E[r, 0] * bx + E[r, 1] * by + E[r, 2]
    for c in range(3):
        F[0, c] = ifx * G[0, c]
        F[1, c] = ify * G[1, c]
        F[2, c] = bx * G[0, c] + by * G[1, c] + G[2, c]
    return F


def k_supported(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return bool(K[0, 1] == 0 and K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1 and K[0, 0] != 0 and K[1, 1] != 0
                and np.isfinite(K[[0, 1, 0, 1], [0, 1, 2, 2]]).all())


def symmetric_distances(x1, x2, F):
    """x1, x2 [n, 2] float64 pixel points, F the pixel fundamental matrix -> d [n]:
    d_k = |l1_k . (x2_k, 1)| + |l2_k . (x1_k, 1)|, each dot product as l0 x + l1 y + l2."""
    x1 = np.asarray(x1, np.float64).reshape(-1, 2); x2 = np.asarray(x2, np.float64).reshape(-1, 2)
    F = np.asarray(F, np.float64).reshape(3, 3)
    a1, b1, c1 = _lines64(x1[:, 0], x1[:, 1], F.ravel())
    a2, b2, c2 = _lines64(x2[:, 0], x2[:, 1], F.T.ravel())
    return np.abs(a1 * x2[:, 0] + b1 * x2[:, 1] + c1) + np.abs(a2 * x1[:, 0] + b2 * x1[:, 1] + c2)


def stats(d):
    """(n, mean, std, max) of the distances: sequential sums in order from 0.0, population standard deviation in two passes."""
    d = np.asarray(d, np.float64).ravel()
    n = len(d)
    if n == 0:
        return 0, 0.0, 0.0, 0.0
    mean = seq_sum(d) / np.float64(n)
    e = d - mean
    return n, float(mean), float(np.sqrt(seq_sum(e * e) / np.float64(n))), float(d.max())


def pairs_epipolar(inliers1, inliers2, E, K, status=0):
    """One pair of vo_pairs_epipolar: the pixel inliers in match order, the pair's E and status -> dict(n, mean, std, max, dist)."""
    if status != 0 or len(inliers1) == 0:
        return dict(n=0, mean=0.0, std=0.0, max=0.0, dist=np.zeros(0))
    d = symmetric_distances(inliers1, inliers2, pixel_fundamental(E, K))
    n, mean, sd, mx = stats(d)
    return dict(n=n, mean=mean, std=sd, max=mx, dist=d)

"""The checker of vo_undistort_points / vo_frames_undistort: cv2.undistortPoints(src, K, dist, R, P) with its default termination,
restated in numpy with the operation order include/vo_hip.h fixes — OpenCV 4.7's undistort.dispatch.cpp as remembered; parity
with a cv2 build is unpinned.  Five fixed-point iterations, no epsilon test; 4, 5 or 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]]).

Every line below is ONE float64 ufunc on whole arrays: numpy rounds each of them once per element and can neither fuse two of
them nor reorder them, so an element's value is the value of the scalar expression evaluated left to right, one rounding per
operation — which is what the kernel computes (-ffp-contract=off).  The contract between the two is byte equality.

Also here: the forward model distort() (ideal normalised -> distorted normalised) for the round-trip tests, and the reference's
own coefficients (src/image_and_keypoints.py:21-25)."""
import numpy as np

# src/image_and_keypoints.py:21-25: k1, k2, p1, p2, k3 of the drone camera's manual calibration
REFERENCE_DIST = np.array([0.0097935857180804498, -0.021794052829051412, 0.0046443590741258711, -0.0045664024579022498,
                           0.017776502734846815])
ITERATIONS = 5


def coefficients(dist):
    """(k1, k2, p1, p2, k3, k4, k5, k6) as float64 scalars; absent ones are zero.  None / empty: all zero."""
    d = np.zeros(0) if dist is None else np.asarray(dist, np.float64).ravel()
    if d.size in (12, 14):
        raise NotImplementedError("thin-prism and tilt coefficients are not built")
    if d.size not in (0, 4, 5, 8):
        raise ValueError("4, 5 or 8 distortion coefficients are needed")
    k = np.zeros(8)
    k[:d.size] = d
    return tuple(np.float64(v) for v in k)


def compose(R=None, P=None):
    """RR = P[:, :3] R, the identity where an argument is absent: RR[i][j] = P[i][0] R[0][j] + P[i][1] R[1][j] + P[i][2] R[2][j]."""
    Rm = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    Pm = np.eye(3) if P is None else np.asarray(P, np.float64)[:, :3]
    RR = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            a = Pm[i, 0] * Rm[0, j]
            b = Pm[i, 1] * Rm[1, j]
            c = Pm[i, 2] * Rm[2, j]
            RR[i, j] = (a + b) + c
    return RR


def normalise(u, v, K):
    """x = (u - cx) (1 / fx), y = (v - cy) (1 / fy)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    one = np.float64(1.0)
    ifx = one / K[0, 0]
    ify = one / K[1, 1]
    x = u - K[0, 2]
    x = x * ifx
    y = v - K[1, 2]
    y = y * ify
    return x, y


def iterate(x0, y0, dist, iterations=ITERATIONS):
    """The inverse model's fixed-point sweeps from (x0, y0) (normalised, float64 arrays).  Returns (x, y, fell_back): an element
    whose icdist comes out negative in some sweep is restored to (x0, y0) and takes no further sweep (fell_back True)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(dist)
    one, two = np.float64(1.0), np.float64(2.0)
    x = x0.copy()
    y = y0.copy()
    live = np.ones(x.shape, bool)
    tp1 = two * p1
    tp2 = two * p2
    for _ in range(iterations):
        xx = x * x
        yy = y * y
        r2 = xx + yy
        num = k6 * r2
        num = num + k5
        num = num * r2
        num = num + k4
        num = num * r2
        num = one + num
        den = k3 * r2
        den = den + k2
        den = den * r2
        den = den + k1
        den = den * r2
        den = one + den
        icdist = num / den
        neg = icdist < 0                                   # a NaN is not negative: it takes every sweep and stays NaN
        # dx = ((2 p1) x) y + p2 (r2 + (2 x) x)
        a = tp1 * x
        a = a * y
        b = two * x
        b = b * x
        b = r2 + b
        b = p2 * b
        dx = a + b
        # dy = p1 (r2 + (2 y) y) + ((2 p2) x) y
        c = two * y
        c = c * y
        c = r2 + c
        c = p1 * c
        d = tp2 * x
        d = d * y
        dy = c + d
        nx = x0 - dx
        nx = nx * icdist
        ny = y0 - dy
        ny = ny * icdist
        stop = live & neg
        go = live & ~neg
        x = np.where(go, nx, np.where(stop, x0, x))
        y = np.where(go, ny, np.where(stop, y0, y))
        live = go
    return x, y, ~live


def project(x, y, RR):
    """xx = RR0 x + RR1 y + RR2, yy likewise, ww = 1 / (RR6 x + RR7 y + RR8); (xx ww, yy ww)."""
    one = np.float64(1.0)
    rows = []
    for i in range(3):
        a = RR[i, 0] * x
        b = RR[i, 1] * y
        s = a + b
        s = s + RR[i, 2]
        rows.append(s)
    ww = one / rows[2]
    return rows[0] * ww, rows[1] * ww


def undistort_points(src, K, dist, R=None, P=None, return_fallback=False):
    """src [N, 2] float32 or float64 -> [N, 2] of the same type: float64 arithmetic throughout, a float32 result is the float64
    value rounded once."""
    src = np.asarray(src)
    out_dtype = np.float32 if src.dtype == np.float32 else np.float64
    p = src.astype(np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        x0, y0 = normalise(p[:, 0].copy(), p[:, 1].copy(), K)
        x, y, fb = iterate(x0, y0, dist)
        ox, oy = project(x, y, compose(R, P))
    out = np.stack([ox, oy], axis=1).astype(out_dtype)
    return (out, fb) if return_fallback else out


def undistort_pixels(xy, K, dist):
    """The resident form (vo_frames_undistort): R = I, P = K, float32 pixels in and out."""
    return undistort_points(np.asarray(xy, np.float32), K, dist, None, K)


def distort(x, y, dist):
    """The forward model on ideal normalised coordinates -> distorted normalised coordinates (plain numpy, no order contract):
    r2 = x^2 + y^2, cdist = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
    xd = x cdist + 2 p1 x y + p2 (r2 + 2 x^2), yd = y cdist + p1 (r2 + 2 y^2) + 2 p2 x y."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(dist)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    r2 = x * x + y * y
    cdist = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * cdist + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cdist + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return xd, yd


def distort_pixels(uv, K, dist):
    """Ideal pixels [N, 2] -> distorted pixels [N, 2] (float64) through K."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    xd, yd = distort((uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], dist)
    return np.stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], axis=1)

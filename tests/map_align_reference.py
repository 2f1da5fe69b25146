"""The map-alignment operator (vo_sim3_ransac_batch, vo_map_align; geometry.estimate_similarity, FrontEnd.align_maps) restated with
numpy, and the chosen cases the device is held to (not a test module).

The contract (include/vo_hip.h, "map alignment"), for n correspondences (b_i, a_i) and X_a = s R X_b + t, float64 throughout:
  fit       centroids, var_b = sum |b - bc|^2 / m, H = sum (a - ac)(b - bc)^T / m, H = U D V^T (np.linalg.svd here; the device runs
            a one-sided Jacobi SVD and completes U by u1 x u2), S = diag(1, 1, sign(det U det V)), R = U S V^T, s = tr(D S) / var_b,
            t = ac - s R bc; no model for var_b == 0, a value that is not finite, s <= 0;
  subset    rejected when on either side |d1 . d2| > 0.996 sqrt(|d1|^2 |d2|^2) or a difference vector from point 0 is zero;
  sampling  OpenCV's MWC stream from `seed`, three indices next() % n, a repeat redrawn immediately;
  scoring   e_i = |s R b_i + t - a_i|^2, float32(e_i) <= float32(max_error^2);
  update    in order, iff good > max(best, 2); niters = RANSACUpdateNumIters(confidence, (n - good) / n, 3, niters);
  result    mask and n_inl of the best RANSAC model, (s, R, t) the same fit over the inliers; n < 3 VO_ERR_TOO_FEW; n == 3 one fit;
            fewer than min_inliers inliers or a refit without a model VO_ERR_NO_MODEL with zeros.
vo_map_align = tests/relocalize_reference.match_map with a query map's rows in the place of a frame's, then the above.

THE PREMISE of the GPU tests: sim3_ransac records `nearest`, the smallest |e_i / max_error^2 - 1| over every point of every
hypothesis it consumes and of the final mask.  While that stays above PREMISE (1e-6) no inlier count, and so neither the sequence of
best models nor the stop iteration, can depend on the last bits of an SVD: the device's masks may be required EQUAL.  It is a
condition on the data, not a tolerance; tests/test_map_align_reference.py establishes it for every case below."""
import functools

import numpy as np

import relocalize_reference as RR

VO_OK, VO_ERR_INVALID, VO_ERR_TOO_FEW, VO_ERR_NO_MODEL, VO_ERR_NOT_CONFIGURED, VO_ERR_UNSUPPORTED = 0, -1, -3, -4, -5, -7   # include/vo_hip.h
DEFAULT_SEED = 0xFFFFFFFFFFFFFFFF
COS = 0.996
PREMISE = 1e-6
MAX_ERROR = 0.1


# ------------------------------------------------------------------ the reference
def rng_stream(seed, count):
    """cv::RNG::next for `seed` (0 counts as 0xffffffff, as cv::RNG's constructor has it)."""
    st = seed if seed else 0xFFFFFFFF
    out = []
    for _ in range(count):
        st = ((st & 0xFFFFFFFF) * 4164903690 + (st >> 32)) & 0xFFFFFFFFFFFFFFFF
        out.append(st & 0xFFFFFFFF)
    return out


def update_num_iters(p, ep, model_points, max_iters):
    """cv::RANSACUpdateNumIters."""
    p = min(max(p, 0.0), 1.0); ep = min(max(ep, 0.0), 1.0)
    tiny = np.finfo(np.float64).tiny
    num = max(1.0 - p, tiny)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < tiny:
        return 0
    num, denom = np.log(num), np.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(np.rint(num / denom))


def fit(b, a):
    """Umeyama's closed form over all the rows -> (s, R, t), or None."""
    b = np.asarray(b, np.float64).reshape(-1, 3); a = np.asarray(a, np.float64).reshape(-1, 3)
    m = len(b)
    ac, bc = a.sum(0) / m, b.sum(0) / m
    da, db = a - ac, b - bc
    var_b = (db * db).sum() / m
    H = da.T @ db / m
    if not (var_b > 0) or not np.isfinite(H).all():
        return None
    U, D, Vt = np.linalg.svd(H)
    S = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = U @ np.diag([1.0, 1.0, S]) @ Vt
    s = (D[0] + D[1] + S * D[2]) / var_b
    t = ac - s * (R @ bc)
    if not (np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all() and s > 0):
        return None
    return float(s), R, t


def _dot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def side_ok(p):
    d1, d2 = p[1] - p[0], p[2] - p[0]
    n1, n2, dt = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2)
    return bool(n1 != 0 and n2 != 0 and not abs(dt) > COS * np.sqrt(n1 * n2))


def minimal(b, a):
    """The subset check and the fit of three correspondences."""
    return fit(b, a) if side_ok(a) and side_ok(b) else None


def sq_errors(model, b, a):
    s, R, t = model
    d = s * (b @ R.T) + t - a
    return (d * d).sum(1)


def sim3_ransac(src, dst, max_error, iterations=1000, confidence=0.99, seed=DEFAULT_SEED, min_inliers=0):
    """One problem -> dict(status, scale, R, t, n_inl, mask, and what the run met: iters (hypotheses consumed), redraws, rejected
    (samples the subset check refused), numbers (random numbers used), s_branch (fits that took S = -1 ... counted over consumed
    samples), nearest (see THE PREMISE), best_at (the iterations at which the best model changed))."""
    b = np.ascontiguousarray(np.asarray(src, np.float64).reshape(-1, 3)); a = np.ascontiguousarray(np.asarray(dst, np.float64).reshape(-1, 3))
    n = len(b)
    out = dict(status=VO_OK, scale=0.0, R=np.zeros((3, 3)), t=np.zeros(3), n_inl=0, mask=np.zeros(n, np.uint8), iters=0, redraws=0, rejected=0,
               numbers=0, nearest=np.inf, best_at=[])
    if n < 3:
        out["status"] = VO_ERR_TOO_FEW
        return out
    thr = np.float32(max_error * max_error)
    thr64 = float(max_error) * float(max_error)

    def inliers(model):
        e = sq_errors(model, b, a)
        with np.errstate(invalid="ignore", divide="ignore"):
            near = np.abs(e / thr64 - 1.0)
        out["nearest"] = min(out["nearest"], float(np.nanmin(near)) if np.isfinite(near).any() else np.inf)
        with np.errstate(over="ignore", invalid="ignore"):
            return e.astype(np.float32) <= thr

    best, best_good = None, 0
    if n == 3:
        best = minimal(b, a)
        out["iters"] = 1
        if best is not None:
            best_good = 3
            out["mask"][:] = 1
    else:
        niters = max(int(iterations), 1)
        stream = rng_stream(seed, 3 * niters + 4096)
        pos, k = 0, 0
        while k < niters:
            idx = []
            while len(idx) < 3:
                if pos >= len(stream):
                    stream = rng_stream(seed, 2 * len(stream))
                v = stream[pos] % n
                pos += 1
                if v in idx:
                    out["redraws"] += 1
                    continue
                idx.append(v)
            model = minimal(b[idx], a[idx])
            if model is None:
                out["rejected"] += 1
            else:
                good = int(inliers(model).sum())
                if good > max(best_good, 2):
                    best, best_good = model, good
                    niters = update_num_iters(confidence, (n - good) / n, 3, niters)
                    out["best_at"].append(k)
            k += 1
        out["iters"], out["numbers"] = k, pos
        if best is not None:
            out["mask"] = inliers(best).astype(np.uint8)
            assert int(out["mask"].sum()) == best_good
    if best is None:
        out["status"] = VO_ERR_NO_MODEL
        return out
    out["n_inl"] = best_good
    if best_good < min_inliers:
        out["status"] = VO_ERR_NO_MODEL
        return out
    sel = out["mask"] > 0
    refit = fit(b[sel], a[sel])
    if refit is None:
        out["status"] = VO_ERR_NO_MODEL
        return out
    out["scale"], out["R"], out["t"] = refit
    return out


def map_align(map_rows, map_pts, q_rows, q_pts, max_error, max_distance=0.0, **kw):
    """The whole operator for one query map -> sim3_ransac's dict + bi (query row), ai (staged row), dist, src, dst, n_match."""
    bi, ai, d = RR.match_map(q_rows, map_rows, max_distance)
    src = np.asarray(q_pts, np.float64).reshape(-1, 3)[bi].copy(); dst = np.asarray(map_pts, np.float64).reshape(-1, 3)[ai].copy()
    out = sim3_ransac(src, dst, max_error, **kw)
    out.update(bi=bi, ai=ai, dist=d, src=src, dst=dst, n_match=len(bi))
    return out


def transform(model, X):
    s, R, t = model
    return s * (np.asarray(X, np.float64) @ np.asarray(R).T) + np.asarray(t)


def model_error(got, want):
    """(|ds|, max |dR|, max |dt|) between two (s, R, t)."""
    return abs(got[0] - want[0]), float(np.abs(np.asarray(got[1]) - want[1]).max()), float(np.abs(np.asarray(got[2]) - want[2]).max())


# ------------------------------------------------------------------ the family of exact cases
# (n, outliers, scale, coplanar): the sizes around a round of 64 hypotheses, around the 256 lanes, and the budget's end
FAMILY = ((3, 0, 4.0, False), (4, 1, 0.25, False), (5, 2, 4.0, False), (63, 20, 0.25, False), (64, 32, 4.0, False), (65, 40, 0.25, False),
          (257, 128, 4.0, False), (300, 210, 0.25, False), (1000, 800, 4.0, False), (2000, 1700, 0.25, False), (300, 100, 4.0, True))
# generator seeds that were moved until the case met what its place in the family is for (tests/test_map_align_reference.py says what)
GEN_SEED = {}


def family_case(n, n_out, scale, coplanar=False, gen=None, noise=0.0):
    """b uniform in +-20 (z = 0 before a rotation of its own when coplanar), a = scale R b + t exactly (plus Gaussian `noise` per
    axis), the first n_out of a seeded permutation displaced by 2 .. 6 units per axis, either sign.  RANSAC seed = n."""
    gen = GEN_SEED.get((n, n_out, coplanar), 0) if gen is None else gen
    rng = np.random.default_rng(410000 + 1000 * gen + 7 * n + n_out + (50000 if coplanar else 0))
    b = rng.uniform(-20, 20, (n, 3))
    if coplanar:
        b[:, 2] = 0
        b = b @ RR.rotation(rng.normal(size=3), rng.uniform(0.3, 1.2)).T + rng.uniform(-3, 3, 3)
    R = RR.rotation(rng.normal(size=3), rng.uniform(0.2, 2.8)); t = rng.uniform(-10, 10, 3)
    a = scale * (b @ R.T) + t
    if noise:
        a = a + rng.normal(0, noise, a.shape)
    out = np.zeros(n, bool); out[rng.permutation(n)[:n_out]] = True
    a[out] += rng.uniform(2, 6, (n_out, 3)) * rng.choice([-1.0, 1.0], (n_out, 3))
    return dict(src=b, dst=a, model=(float(scale), R, t), outlier=out, max_error=MAX_ERROR, seed=n)


def family():
    return [family_case(*f) for f in FAMILY]


@functools.lru_cache(maxsize=None)
def family_runs(seed_is_n=False):
    """The checker on the whole family, once: [(case, run)], under the default seed or under seed = n."""
    return [(c, sim3_ransac(c["src"], c["dst"], c["max_error"], **(dict(seed=c["seed"]) if seed_is_n else {}))) for c in family()]


@functools.lru_cache(maxsize=None)
def checker_error():
    """The checker's own largest error against the generating similarity on the exact family (|ds|, max |dR|, max |dt|), both
    seedings: what the device's bound is a multiple of (MARGIN)."""
    worst = np.zeros(3)
    for seed_is_n in (False, True):
        for c, r in family_runs(seed_is_n):
            worst = np.maximum(worst, model_error((r["scale"], r["R"], r["t"]), c["model"]))
    return tuple(float(v) for v in worst)


MARGIN = 100.0                     # the device may be this many times the checker's own error away: two SVD algorithms and summation orders
#                                    lie inside it, a wrong branch ten orders outside


def noisy_case():
    """Gaussian noise of 0.004 per axis on a (max_error 0.1: 14 sigma of |e|), 300 points, 100 outliers."""
    return family_case(300, 100, 4.0, noise=0.004, gen=3)


def branch_cases():
    """name -> (src, dst, opts, what the status must be or None): the cases that reach the kernel's other branches."""
    rng = np.random.default_rng(420000)
    good = family_case(64, 32, 4.0)
    line = np.outer(np.arange(7.0), [1.0, 2.0, -0.5]) + [3.0, 1.0, 2.0]
    big = family_case(3100, 310, 0.25, gen=1)               # past the LDS staging path (3072 correspondences)
    c = {}
    for k in (0, 1, 2):
        c[f"n{k}"] = (good["src"][:k], good["dst"][:k], {}, VO_ERR_TOO_FEW)
    c["n3_collinear"] = (line[:3], 2.0 * line[:3] + 1.0, {}, VO_ERR_NO_MODEL)
    c["identical"] = (np.tile(rng.uniform(-5, 5, 3), (40, 1)), np.tile(rng.uniform(-5, 5, 3), (40, 1)), {}, VO_ERR_NO_MODEL)
    c["collinear"] = (line, 2.0 * line + 1.0, {}, VO_ERR_NO_MODEL)
    c["past_lds"] = (big["src"], big["dst"], dict(seed=big["seed"]), VO_OK)
    c["min_inliers_above"] = (good["src"], good["dst"], dict(seed=64, min_inliers=33), VO_ERR_NO_MODEL)
    c["min_inliers_met"] = (good["src"], good["dst"], dict(seed=64, min_inliers=32), VO_OK)
    c["iterations_1"] = (good["src"], good["dst"], dict(seed=64, iterations=1), None)
    c["iterations_65"] = (family_case(300, 210, 0.25)["src"], family_case(300, 210, 0.25)["dst"], dict(seed=300, iterations=65), None)
    c["other_seed"] = (good["src"], good["dst"], dict(seed=12345), VO_OK)
    c["default_seed"] = (good["src"], good["dst"], {}, VO_OK)
    return c


# ------------------------------------------------------------------ two maps that see the same ground
def align_case(detector, npt, n, n_wrong=None, scale=2.5, gen=0):
    """A staged map of npt rows and a query map of n rows over tests/relocalize_reference's tied rows (duplicates a lane, a group
    and a chunk apart on both sides).  The query's points are the staged points of the rows they were copied from taken through
    the INVERSE of a generating similarity — exactly, except n_wrong of them, which lie elsewhere: 3D-3D outliers whose rows still
    match.  Rows that match nothing meaningful pair up by chance and are outliers too."""
    c = RR.match_case(detector, npt, n, seed=gen)
    rng = np.random.default_rng(430000 + 1000 * gen + 7 * npt + n + (0 if detector == "orb" else 500))
    R = RR.rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)); t = rng.uniform(-4, 4, 3)
    bi, ai, _ = RR.match_map(c["rows"], c["map_rows"])
    q_pts = rng.uniform(-30, 30, (n, 3))
    Xa = c["map_pts"]
    q_pts[bi] = (Xa[ai] - t) @ R / scale                    # X_b = R^T (X_a - t) / s
    n_wrong = len(bi) // 5 if n_wrong is None else n_wrong
    wrong = rng.permutation(len(bi))[:n_wrong]
    q_pts[bi[wrong]] += rng.uniform(1, 3, (len(wrong), 3)) * rng.choice([-1.0, 1.0], (len(wrong), 3))
    return dict(map_rows=c["map_rows"], map_pts=Xa, rows=c["rows"], pts=q_pts, model=(float(scale), R, t), max_error=0.05)

"""The guided map alignment operator (vo_map_align_guided; FrontEnd.align_maps_guided) restated twice — with numpy, elementwise in
the header's operation order, and as plain Python loops with no vectorised shortcut —, frontend.merge_maps restated as a loop, and
the chosen cases the device is held to (not a test module).

The contract (include/vo_hip.h, "guided map alignment"), float64, one rounding per operation, in this order, for one query map with
points b_i and one row each against the staged points a_j, S = (s, R row-major, t):
  1 y_k = s * ((R[k][0] bx + R[k][1] by) + R[k][2] bz) + t_k; the point takes part iff all three y_k are finite;
  2 staged point j is a candidate iff (dx dx + dy dy) + dz dz <= r2, d = a_j - y componentwise, r2 = radius radius;
  3 d(i, j) the exact integer (Hamming / sum of squared differences); fd = float32(d) for ORB, sqrt(float32(d)) for SIFT rows;
  4 best = smallest (d, j); d2 = second-smallest d of the multiset; fewer than two candidates: fd2 = FLT_MAX; n_seen counts query
    points with a candidate;
  5 max_distance > 0: float64(fd) < max_distance; ratio > 0: fewer than two candidates or float64(fd) < ratio * float64(fd2);
  6 among the query points that pass 5 with best == j, the smallest (d, i) keeps staged point j;
  7 the list in ascending query-row order: (i, j, fd, fd2), src = b_i, dst = a_j.
The similarity part is tests/map_align_reference.py's sim3_ransac on those lists (map_align_guided below); the device runs
vo_sim3_ransac_batch's kernel on them, and tests/test_gpu_map_fuse.py compares it with that call byte for byte.

TILE: the query rows one workgroup of k_fuse_match owns.  GRID: k_fuse_grid's cells are GRID per axis over the staged points' own box,
an edge per axis (docs/kernels/k_map_fuse.md): the grid cases below choose a box of 160 units a side, so that cells are 10 units."""
import numpy as np

import map_align_reference as A
import relocalize_reference as R

FLT_MAX = np.float32(np.finfo(np.float32).max)
TILE, GRID = 256, 16
MAP_SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 513)
QUERY_SIZES = ((257, 0, 65), (1, 256, 3))                          # three unequal maps per call: the 256-row padding seams are reached
IDENTITY = np.array([1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def sim13(s, Rm, t):
    return np.concatenate([[float(s)], np.asarray(Rm, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


# ------------------------------------------------------------------ the reference, with numpy
def transform(S, pts):
    """(takes part [n] bool, y [n, 3]) — step 1, elementwise float64 operations in the contract's order."""
    S = np.asarray(S, np.float64).reshape(13)
    b = np.asarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        y = np.stack([S[0] * ((S[1 + 3 * k] * b[:, 0] + S[2 + 3 * k] * b[:, 1]) + S[3 + 3 * k] * b[:, 2]) + S[10 + k] for k in range(3)], axis=1)
    return np.isfinite(y).all(axis=1) if len(b) else np.zeros(0, bool), y.reshape(-1, 3)


def int_distances(rows, row):
    """exact integer distances of `rows` [n, D] to one row: Hamming for D = 32, sum of squared differences for D = 128"""
    if rows.shape[1] == 32:
        return np.unpackbits(rows ^ row, axis=1).sum(axis=1).astype(np.int64)
    return ((rows.astype(np.int64) - row.astype(np.int64)) ** 2).sum(axis=1)


def reported(d, sift):
    """cv2's float32 distance of the exact integer d"""
    return np.sqrt(np.float32(d)) if sift else np.float32(d)


def fuse_match(map_pts, map_rows, q_pts, q_rows, S, radius, ratio=0.0, max_distance=0.0):
    """Steps 1 - 7 for one query map -> dict(bi, ai int32; dist, dist2 float32; n_seen; n_match; src, dst)."""
    a = np.asarray(map_pts, np.float64).reshape(-1, 3); b = np.asarray(q_pts, np.float64).reshape(-1, 3)
    m = np.ascontiguousarray(map_rows, np.uint8); f = np.ascontiguousarray(q_rows, np.uint8)
    sift = (m.shape[1] if len(m) else f.shape[1] if len(f) else 32) == 128
    take, y = transform(S, b)
    r2 = float(radius) * float(radius)
    claim = {}                                                             # staged point -> (d, i, d2 or None)
    n_seen = 0
    for i in np.flatnonzero(take):
        with np.errstate(all="ignore"):
            dx = a[:, 0] - y[i, 0]; dy = a[:, 1] - y[i, 1]; dz = a[:, 2] - y[i, 2]
            cand = np.flatnonzero((dx * dx + dy * dy) + dz * dz <= r2)
        if len(cand) == 0:
            continue
        n_seen += 1
        d = int_distances(m[cand], f[i])
        order = np.lexsort((cand, d))
        j, db = int(cand[order[0]]), int(d[order[0]])
        d2 = int(d[order[1]]) if len(cand) > 1 else None
        fd = reported(db, sift); fd2 = FLT_MAX if d2 is None else reported(d2, sift)
        if max_distance > 0 and not float(fd) < float(max_distance):
            continue
        if ratio > 0 and d2 is not None and not float(fd) < float(ratio) * float(fd2):
            continue
        if j not in claim or (db, int(i)) < claim[j][:2]:
            claim[j] = (db, int(i), d2)
    by_row = sorted((v[1], j, v[0], v[2]) for j, v in claim.items())
    bi = np.array([e[0] for e in by_row], np.int32); ai = np.array([e[1] for e in by_row], np.int32)
    dist = np.array([reported(e[2], sift) for e in by_row], np.float32)
    dist2 = np.array([FLT_MAX if e[3] is None else reported(e[3], sift) for e in by_row], np.float32)
    return dict(bi=bi, ai=ai, dist=dist, dist2=dist2, n_seen=n_seen, n_match=len(bi), src=b[bi].copy().reshape(-1, 3), dst=a[ai].copy().reshape(-1, 3))


# ------------------------------------------------------------------ the same contract as plain loops
def _popcount_row(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def _ssd_row(a, b):
    return sum((int(x) - int(y)) ** 2 for x, y in zip(a, b))


def _finite(x):
    return x == x and x not in (float("inf"), float("-inf"))


def fuse_match_loops(map_pts, map_rows, q_pts, q_rows, S, radius, ratio=0.0, max_distance=0.0):
    """fuse_match with IEEE doubles one operation at a time and explicit loops."""
    a = [[float(c) for c in p] for p in np.asarray(map_pts, np.float64).reshape(-1, 3)]
    b = [[float(c) for c in p] for p in np.asarray(q_pts, np.float64).reshape(-1, 3)]
    m = np.ascontiguousarray(map_rows, np.uint8); f = np.ascontiguousarray(q_rows, np.uint8)
    Sv = [float(c) for c in np.asarray(S, np.float64).reshape(13)]
    sift = (m.shape[1] if len(m) else f.shape[1] if len(f) else 32) == 128
    dist_of = _ssd_row if sift else _popcount_row
    mrows = [r.tolist() for r in m]; frows = [r.tolist() for r in f]
    r2 = float(radius) * float(radius)
    owner = {}
    n_seen = 0
    with np.errstate(all="ignore"):
        for i, (bx, by, bz) in enumerate(b):
            y = []
            for k in range(3):
                inner = np.float64(Sv[1 + 3 * k]) * np.float64(bx) + np.float64(Sv[2 + 3 * k]) * np.float64(by)
                inner = inner + np.float64(Sv[3 + 3 * k]) * np.float64(bz)
                y.append(float(np.float64(Sv[0]) * inner + np.float64(Sv[10 + k])))
            if not all(_finite(v) for v in y):
                continue
            best = None; second = None; cnt = 0
            for j, (ax, ay, az) in enumerate(a):
                dx = np.float64(ax) - y[0]; dy = np.float64(ay) - y[1]; dz = np.float64(az) - y[2]
                if not (dx * dx + dy * dy) + dz * dz <= r2:
                    continue
                d = dist_of(frows[i], mrows[j])
                cnt += 1
                if best is None:
                    best = (d, j)
                elif (d, j) < best:
                    second = best[0]; best = (d, j)
                elif second is None or d < second:
                    second = d
            if cnt == 0:
                continue
            n_seen += 1
            fd = reported(best[0], sift); fd2 = FLT_MAX if cnt < 2 else reported(second, sift)
            if max_distance > 0 and not float(fd) < float(max_distance):
                continue
            if ratio > 0 and cnt >= 2 and not float(fd) < float(ratio) * float(fd2):
                continue
            j = best[1]
            if j not in owner or (best[0], i) < owner[j][:2]:
                owner[j] = (best[0], i, fd, fd2)
    by_row = sorted((v[1], j, v[2], v[3]) for j, v in owner.items())
    return dict(bi=np.array([e[0] for e in by_row], np.int32), ai=np.array([e[1] for e in by_row], np.int32),
                dist=np.array([e[2] for e in by_row], np.float32), dist2=np.array([e[3] for e in by_row], np.float32), n_seen=n_seen,
                n_match=len(by_row))


def map_align_guided(map_rows, map_pts, q_rows, q_pts, S, radius, max_error, ratio=0.0, max_distance=0.0, **kw):
    """The whole operator for one query map: fuse_match, then map_align_reference's RANSAC on its lists."""
    r = fuse_match(map_pts, map_rows, q_pts, q_rows, S, radius, ratio, max_distance)
    out = A.sim3_ransac(r["src"], r["dst"], max_error, **kw)
    out.update(r)
    return out


def merge_maps_loops(rows_a, points_a, rows_b, points_b, scale, Rm, t, a_idx, b_idx, mask):
    """frontend.merge_maps one row at a time."""
    Rm = np.asarray(Rm, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3); s = np.float64(scale)
    rows = [np.asarray(r) for r in rows_a]; pts = [np.asarray(p, np.float64) for p in np.asarray(points_a, np.float64).reshape(-1, 3)]
    to_a = {}
    for k in range(len(a_idx)):
        if mask[k]:
            to_a[int(b_idx[k])] = int(a_idx[k])
    index_b = []
    for i, p in enumerate(np.asarray(points_b, np.float64).reshape(-1, 3)):
        if i in to_a:
            index_b.append(to_a[i])
            continue
        index_b.append(len(rows))
        rows.append(np.asarray(rows_b[i]))
        pts.append(np.array([s * ((Rm[k, 0] * p[0] + Rm[k, 1] * p[1]) + Rm[k, 2] * p[2]) + t[k] for k in range(3)]))
    return dict(rows=np.array(rows), points=np.array(pts).reshape(-1, 3), index_b=np.array(index_b, np.int32), n_fused=len(to_a))


# ------------------------------------------------------------------ cases
# A case: dict(map_rows, map_pts, queries = [(rows, pts)], priors = [S] (one per query map), radius, ratio, max_distance, and `expect`:
# what the case is named for, held on the reference by tests/test_map_fuse_reference.py — per query, any of
#   pairs: (query row, staged row) entries the list must hold; absent_b / absent_a: query / staged rows it must not hold;
#   n_match, n_seen: exact counts; seconds: {query row: float32 second distance}.
def _salt(det):
    return 0 if det == "orb" else 500000


def gen_sim(seed):
    rng = np.random.default_rng(51000 + seed)
    return sim13(rng.uniform(0.5, 2.0), R.rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)), rng.uniform(-4, 4, 3))


def inverse_points(S, y):
    """b with S(b) ~ y: R^T (y - t) / s (not exact; the contract starts from b)"""
    S = np.asarray(S, np.float64)
    return (np.asarray(y, np.float64).reshape(-1, 3) - S[10:]) @ S[1:10].reshape(3, 3) / S[0]


def gen_map(det, npt):
    """npt rows and points in a slab of 16 x 16 x 1 units (a drone map: thin); rows (2, 3) and (5, 5 + TILE) duplicated, the copies
    almost where their originals stand: two staged points that look alike inside one sphere."""
    rng = np.random.default_rng(52000 + 7 * npt + _salt(det))
    rows = R.rand_rows(rng, npt, det)
    pts = np.column_stack([rng.uniform(-8, 8, npt), rng.uniform(-8, 8, npt), rng.uniform(-0.5, 0.5, npt)]).reshape(-1, 3)
    for x, c in ((2, 3), (5, 5 + TILE)):
        if c < npt:
            rows[c] = rows[x]; pts[c] = pts[x] + 1e-3
    return rows, pts


def gen_query(det, map_rows, map_pts, S, n, radius, seed=0):
    """n query points: three in four sit, once S has moved them, within 1.3 radius of a staged point and carry a nudged copy of its
    row (in or out of the sphere, several per sphere, several query points per staged point); the rest are random rows in the slab.
    Rows 10 and 11 (when there) are one row at one position: two query points that want the same staged point at equal distance."""
    npt = len(map_rows)
    rng = np.random.default_rng(53000 + 1000 * seed + 7 * npt + n + _salt(det))
    rows = R.rand_rows(rng, n, det)
    y = np.column_stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-0.5, 0.5, n)]).reshape(-1, 3)
    for i in range(n):
        if npt and i % 4 != 3:
            j = int(rng.integers(0, npt))
            v = rng.normal(size=3); v *= radius * 1.3 * np.cbrt(rng.uniform()) / np.linalg.norm(v)
            y[i] = map_pts[j] + v
            rows[i] = R.nudge(map_rows[j], int(rng.integers(0, 3)), det)
    pts = inverse_points(S, y)
    if n > 11:
        rows[11] = rows[10]; pts[11] = pts[10]
    return rows, pts


def size_case(det, npt, sizes=QUERY_SIZES[0], radius=0.4, ratio=0.0, max_distance=0.0):
    """A call of len(sizes) query maps with different priors against the staged map of npt points."""
    rows, pts = gen_map(det, npt)
    priors = [gen_sim(q) for q in range(len(sizes))]
    queries = [gen_query(det, rows, pts, priors[q], n, radius, seed=q) for q, n in enumerate(sizes)]
    return dict(map_rows=rows, map_pts=pts, queries=queries, priors=priors, radius=radius, ratio=ratio, max_distance=max_distance,
                expect=[{} for _ in sizes])


def _case(map_rows, map_pts, queries, priors, radius, expect, ratio=0.0, max_distance=0.0):
    return dict(map_rows=map_rows, map_pts=np.asarray(map_pts, np.float64), queries=queries, priors=priors, radius=radius, ratio=ratio,
                max_distance=max_distance, expect=expect)


def sphere_case(det, radius):
    """The identity prior (y = b exactly) and integer coordinates: query rows 0, 1, 2 lie at offsets (3, 4, 0), (0, 0, 5) — ON the
    sphere of radius 5 — and (2, 3, 6) — ON the sphere of radius 7 — from staged points 0, 1, 2; query row 3 coincides with staged
    point 3.  Staged points 4 (a NaN coordinate) and 5 (an infinite one) are never candidates, query rows 6 (NaN) and 7 (infinite)
    take no part; each carries the row of a partner that stands exactly where its finite coordinates point."""
    rng = np.random.default_rng(54000 + _salt(det))
    a = np.array([[10.0, 10, 10], [30, 10, 10], [50, 10, 10], [70, 10, 10], [np.nan, 20, 20], [np.inf, 30, 30], [90, 10, 10], [110, 10, 10]])
    map_rows = R.rand_rows(rng, len(a), det)
    b = np.array([[13.0, 14, 10], [30, 10, 15], [52, 13, 16], [70, 10, 10], [0, 20, 20], [1e300, 30, 30], [np.nan, 10, 10], [-np.inf, 10, 10]])
    rows = np.stack([R.nudge(map_rows[j], j % 3, det) for j in range(len(a))])
    pairs = [(3, 3)] + ([(0, 0), (1, 1)] if radius >= 5.0 else []) + ([(2, 2)] if radius >= 7.0 else [])
    e = dict(pairs=pairs, absent_b=[4, 5, 6, 7], absent_a=[4, 5, 6, 7], n_match=len(pairs), n_seen=len(pairs))
    return _case(map_rows, a, [(rows, b)], [IDENTITY], radius, [e])


def overflow_case(det):
    """Two query maps with the same arrays: under the first prior (s = 1e308, finite) every product overflows and no point takes
    part; under the identity each finds its partner."""
    rng = np.random.default_rng(54500 + _salt(det))
    a = np.array([[10.0, 10, 10], [30, 10, 10], [50, 10, 10], [20, 40, 10]])
    map_rows = R.rand_rows(rng, 4, det)
    rows = np.stack([R.nudge(map_rows[j], 1, det) for j in range(4)])
    big = IDENTITY.copy(); big[0] = 1e308
    e0 = dict(n_match=0, n_seen=0)
    e1 = dict(pairs=[(j, j) for j in range(4)], n_match=4, n_seen=4)
    return _case(map_rows, a, [(rows, a.copy()), (rows, a.copy())], [big, IDENTITY], 1.0, [e0, e1])


GRID_BOX = 160.0                                                           # the grid cases' staged box: 160 units a side, cells of 10


def grid_case(det, radius):
    """Spheres against the grid.  Staged points 0 and 1 are the corners of the box; 2 .. 10 are chosen, the rest random.  Query rows:
      2   0.35 from staged 2                       3   exactly on staged 3, which lies on a cell corner (40, 80, 120)
      4   one unit from staged 4, in the box's last cells
      5   between staged 5 and 6, one row twice in ONE cell, half a unit either side: the lower staged index wins
      6   between staged 7 and 8, one row twice in TWO cells, one unit either side, the LOWER index in the LATER cell
      7, 8   one row, both half a unit from staged 9: the lower query row keeps it (one tile)
      9, 9 + TILE   the same around staged 10 (a tile apart)
      10  far outside the box, at (5000, 5000, 5000)."""
    rng = np.random.default_rng(55000 + _salt(det))
    npt, n = 11 + TILE, 14 + TILE
    map_rows = R.rand_rows(rng, npt, det)
    a = rng.uniform(0, GRID_BOX, (npt, 3)).round()
    a[0] = 0; a[1] = GRID_BOX
    a[2] = (100, 100, 100); a[3] = (40, 80, 120); a[4] = (155, 158, 3)
    a[5] = (61, 61, 61); a[6] = (62, 61, 61); map_rows[6] = map_rows[5]
    a[7] = (71, 31, 31); a[8] = (69, 31, 31); map_rows[8] = map_rows[7]
    a[9] = (30, 130, 30); a[10] = (130, 30, 30)
    rows = R.rand_rows(rng, n, det)
    b = rng.uniform(0, GRID_BOX, (n, 3))
    for i, (pos, j, k) in {2: ((100.25, 100.25, 100), 2, 1), 3: ((40, 80, 120), 3, 0), 4: ((156, 158, 3), 4, 1), 5: ((61.5, 61, 61), 5, 1),
                           6: ((70, 31, 31), 7, 1), 7: ((30.5, 130, 30), 9, 2), 8: ((29.5, 130, 30), 9, 2), 9: ((130, 30.5, 30), 10, 0),
                           9 + TILE: ((130, 29.5, 30), 10, 0), 10: ((5000, 5000, 5000), 0, 0)}.items():
        b[i] = pos; rows[i] = R.nudge(map_rows[j], k, det)
    e = {}
    if radius == 0.5:
        e = dict(pairs=[(2, 2), (3, 3), (5, 5), (7, 9), (9, 10)], absent_b=[4, 6, 8, 9 + TILE, 10], absent_a=[4, 6, 7, 8])
    elif radius == 10.0:
        e = dict(pairs=[(2, 2), (3, 3), (4, 4), (5, 5), (6, 7), (7, 9), (9, 10)], absent_b=[10])
    elif radius >= 9000:
        e = dict(n_seen=n)
    return _case(map_rows, a, [(rows, b)], [IDENTITY], radius, [e])


def far_case(det):
    """Every query point far outside the staged box, radius small: no candidates, and a window whose cell range is clamped to the
    box's last cells on every axis."""
    c = grid_case(det, 0.5)
    rows, b = c["queries"][0]
    return _case(c["map_rows"], c["map_pts"], [(rows[:40], b[:40] + 5000.0)], [IDENTITY], 3.0, [dict(n_match=0, n_seen=0)])


def flat_case(det, kind):
    """Staged maps without extent: 'point' a single point, 'line' 20 points along x (y = z = 2), 'plane' 30 points with z = 0.  Every
    staged point has a query partner 0.25 away (off the line / plane too), radius 0.4; the neighbours are a unit or more away."""
    rng = np.random.default_rng(56000 + _salt(det) + {"point": 0, "line": 1, "plane": 2}[kind])
    if kind == "point":
        a = np.array([[5.0, 5, 5]])
    elif kind == "line":
        a = np.column_stack([np.arange(20.0), np.full(20, 2.0), np.full(20, 2.0)])
    else:
        a = np.column_stack([np.repeat(np.arange(6.0), 5) * 2, np.tile(np.arange(5.0), 6) * 2, np.zeros(30)])
    map_rows = R.rand_rows(rng, len(a), det)
    rows = np.stack([R.nudge(r, j % 3, det) for j, r in enumerate(map_rows)] + [R.rand_rows(rng, 1, det)[0]])
    off = np.array([[0.25, 0, 0], [0, 0.25, 0], [0, 0, 0.25], [0, 0, -0.25]])
    b = np.concatenate([a + off[np.arange(len(a)) % 4], [[3.5, 7.5, 1.5]]])                # (the last one is near nothing)
    e = dict(pairs=[(j, j) for j in range(len(a))], n_match=len(a), n_seen=len(a), absent_b=[len(a)])
    return _case(map_rows, a, [(rows, b)], [IDENTITY], 0.4, [e])


def filter_case(det, which):
    """'max_distance': query rows 0 and 1 each have one staged point, at reported distances EQUAL to the bound (dropped: the test is
    strict) and below it (kept).  'ratio' (0.8): row 0 has one candidate (kept); row 1 has two equal candidates (dropped); row 2 has
    staged 4 and 5 at equal distance in its sphere and fails the rule, row 3 sees staged 4 alone, from farther in descriptor space,
    and keeps it: the filters come before the uniqueness step.  'ratio_eq' (0.5): row 0 has fd = 0.5 fd2 EXACTLY (dropped), row 1,
    one step nearer, is kept."""
    rng = np.random.default_rng(57000 + _salt(det))
    sift = det == "sift"
    if which == "max_distance":
        rows = R.rand_rows(rng, 2, det)
        map_rows = np.stack([R.nudge(rows[0], 3, det), R.nudge(rows[1], 2, det)])       # d = 4, 3: ORB 4.0, 3.0; SIFT 2.0, sqrt(3)
        a = np.array([[100.0, 100, 0], [200, 100, 0]]); b = a + [1.0, 0, 0]
        e = dict(pairs=[(1, 1)], absent_b=[0], n_match=1, n_seen=2)
        return _case(map_rows, a, [(rows, b)], [IDENTITY], 3.0, [e], max_distance=2.0 if sift else 4.0)
    if which == "ratio":
        map_rows = R.rand_rows(rng, 8, det)
        map_rows[3] = map_rows[2]; map_rows[5] = map_rows[4]
        a = np.array([[100.0, 100, 0], [200, 100, 0], [300, 100, 0], [302, 100, 0], [100, 300, 0], [96, 300, 0], [400, 400, 0], [50, 450, 0]])
        rows = np.stack([R.nudge(map_rows[0], 2, det), R.nudge(map_rows[2], 1, det), R.nudge(map_rows[4], 0, det), R.nudge(map_rows[4], 2, det)])
        b = np.array([[101.0, 100, 0], [301, 100, 0], [98, 300, 0], [102.5, 300, 0]])
        e = dict(pairs=[(0, 0), (3, 4)], absent_b=[1, 2], n_match=2, n_seen=4, seconds={0: FLT_MAX, 3: FLT_MAX})
        return _case(map_rows, a, [(rows, b)], [IDENTITY], 3.0, [e], ratio=0.8)
    rows = R.rand_rows(rng, 2, det)
    far = 15 if sift else 7                                                 # d2 = 16 (SIFT: fd2 = 4) / 8 (ORB)
    map_rows = np.stack([R.nudge(rows[0], 3, det), R.nudge(rows[0], far, det), R.nudge(rows[1], 2, det), R.nudge(rows[1], far, det)])
    a = np.array([[100.0, 100, 0], [101, 100, 0], [200, 100, 0], [201, 100, 0]])
    b = np.array([[100.5, 100, 0], [200.5, 100, 0]])
    sec = np.float32(4.0 if sift else 8.0)
    e = dict(pairs=[(1, 2)], absent_b=[0], n_match=1, n_seen=2, seconds={1: sec})
    return _case(map_rows, a, [(rows, b)], [IDENTITY], 3.0, [e], ratio=0.5)


KNOWN_RADIUS, KNOWN_MAX_ERROR, KNOWN_N, KNOWN_ALIKE = 0.3, 0.05, 300, 50


def known_case(det, noise=0.004):
    """Two maps of one ground patch, half overlapping: the staged map holds 300 points of a 16 x 16 x 1 slab, the query map 300
    points of which the first 150 are staged points 150 .. 299 seen again — moved by the inverse of a generating similarity, with
    Gaussian noise of `noise` per axis (0: exactly, up to the rounding of the inverse), rows nudged — and the rest lie elsewhere.
    KNOWN_ALIKE of the true duplicates have a look-alike: a staged point among 0 .. 149, somewhere else (outside the sphere: the CPU
    test asserts it), that carries the query's row EXACTLY, so the descriptor-only match goes
    there.  The prior is the generating similarity perturbed by 0.002 rad and 0.01 units (asserted against KNOWN_RADIUS on the
    reference alone)."""
    rng = np.random.default_rng(58000 + _salt(det))
    n = KNOWN_N
    map_rows = R.rand_rows(rng, n, det)
    a = np.column_stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-0.5, 0.5, n)])
    s, Rm, t = 2.5, R.rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)), rng.uniform(-4, 4, 3)
    truth = sim13(s, Rm, t)
    rows = R.rand_rows(rng, n, det)
    y = np.column_stack([rng.uniform(8.5, 24, n), rng.uniform(-8, 8, n), rng.uniform(-0.5, 0.5, n)])   # the part of B that A does not see
    dup = np.arange(150)
    y[dup] = a[150 + dup] + rng.normal(0, noise, (150, 3))
    for i in dup:
        rows[i] = R.nudge(map_rows[150 + i], int(rng.integers(0, 3)), det)
    for i in range(KNOWN_ALIKE):
        map_rows[i] = rows[i]                                              # staged point i looks exactly like query row i
    b = inverse_points(truth, y)
    dR = R.rotation([0.3, -0.5, 0.8], 0.002)
    prior = sim13(s * 1.0005, dR @ Rm, dR @ t + np.array([0.01, -0.006, 0.008]))
    c = _case(map_rows, a, [(rows, b)], [prior], KNOWN_RADIUS, [dict(pairs=[(int(i), int(150 + i)) for i in dup])])
    c.update(truth=(s, Rm, t), dup=dup, max_error=KNOWN_MAX_ERROR)
    return c


def status_case(det):
    """Three query maps for the refinement pass against known_case's staged map: an empty one (VO_ERR_TOO_FEW in align_maps), one
    whose rows are staged rows 60 .. 99 and whose points lie on a line (every sample fails the subset check: VO_ERR_NO_MODEL), and
    known_case's (VO_OK)."""
    c = known_case(det)
    width = c["map_rows"].shape[1]
    junk = (c["map_rows"][60:100].copy(), np.outer(np.arange(40.0), [1.0, 2.0, -0.5]) + [3.0, 1.0, 2.0])
    return dict(map_rows=c["map_rows"], map_pts=c["map_pts"], queries=[(np.zeros((0, width), np.uint8), np.zeros((0, 3))), junk, c["queries"][0]],
                truth=c["truth"], max_error=c["max_error"], radius=c["radius"])


def named_cases(det):
    cases = {f"sphere r={r!r}": sphere_case(det, r) for r in (5.0, float(np.nextafter(5.0, 0.0)), 7.0, 0.0)}
    for r in (0.5, 10.0, 35.0, 9000.0):                                    # inside one cell, one cell edge, 3.5 edges, more than the box and the far point
        cases[f"grid r={r!r}"] = grid_case(det, r)
    cases["far outside"] = far_case(det)
    cases["overflow"] = overflow_case(det)
    for kind in ("point", "line", "plane"):
        cases[f"flat {kind}"] = flat_case(det, kind)
    for which in ("max_distance", "ratio", "ratio_eq"):
        cases[f"filter {which}"] = filter_case(det, which)
    cases["known similarity"] = known_case(det)
    cases["known exact"] = known_case(det, noise=0.0)                      # what the device's refit is held to map_align_reference's bound on
    return cases


def all_cases(det):
    cases = named_cases(det)
    for npt in MAP_SIZES:
        cases[f"sizes npt={npt}"] = size_case(det, npt, QUERY_SIZES[0] if npt % 2 else QUERY_SIZES[1])
    cases["sizes ratio and bound"] = size_case(det, 257, sizes=(257, 65, 256), ratio=0.9, max_distance=3.5 if det == "sift" else 12.0)
    return cases

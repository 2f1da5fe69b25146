"""The guided relocalisation operator (vo_map_localize_guided; FrontEnd.relocalize_guided) restated twice — with numpy, and as
plain Python loops with no vectorised shortcut — and the chosen cases the device is held to (not a test module).

The contract (include/vo_hip.h, "guided relocalisation"), float64, one rounding per operation, in this order:
  1 c_k = ((P[k][0] X + P[k][1] Y) + P[k][2] Z) + P[k][3]; the point takes part iff c_2 > 0; xn = c_0 / c_2, yn = c_1 / c_2;
    u = (K[0] xn + K[1] yn) + K[2], v = (K[3] xn + K[4] yn) + K[5];
  2 keypoint i is a candidate iff dx dx + dy dy <= r2, dx = float64(x_i) - u, dy = float64(y_i) - v, r2 = radius radius;
  3 d(i, j) the exact integer (Hamming / sum of squared differences); fd = float32(d) for ORB, sqrt(float32(d)) for SIFT rows;
  4 best = smallest (d, i); d2 = second-smallest d of the multiset; fewer than two candidates: fd2 = FLT_MAX; n_seen counts points
    with a candidate;
  5 max_distance > 0: float64(fd) < max_distance; ratio > 0: fewer than two candidates or float64(fd) < ratio * float64(fd2);
  6 among the points that pass 5 with best == i, the smallest (d, j) keeps keypoint i;
  7 the list in ascending keypoint order: (i, j, fd, fd2), obj = X_j, img = float64(x_i, y_i).
The pose part is vo_solve_pnp_ransac_batch on those arrays; tests/test_gpu_relocalize_guided.py compares it with that call.

TILE: the points one workgroup of k_guided_match owns.  GRID: the keypoint grid of k_guided_grid is GRID x GRID square cells over the
keypoints' own box, edge = max(larger extent / GRID, 1 px): grid_of() restates it so that a case can say where cell boundaries lie."""
import numpy as np

import relocalize_reference as R

FLT_MAX = np.float32(np.finfo(np.float32).max)
TILE, GRID = 256, 64
MAP_SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)     # 255 / 256 / 257: around one tile; 513: one past two tiles
FRAME_SIZES = (0, 1, 17, 300)                                    # ... and kp_cap, which the rig knows
K_EXACT = np.array([[512.0, 0, 256], [0, 512.0, 256], [0, 0, 1]])
P_IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


# ------------------------------------------------------------------ the reference, with numpy
def project(P, pts, Kmat):
    """(takes part [npt] bool, u [npt], v [npt]) — step 1, elementwise float64 operations in the contract's order."""
    P = np.asarray(P, np.float64).reshape(3, 4); Kmat = np.asarray(Kmat, np.float64).reshape(3, 3)
    X = np.asarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        c = [((P[k, 0] * X[:, 0] + P[k, 1] * X[:, 1]) + P[k, 2] * X[:, 2]) + P[k, 3] for k in range(3)]
        take = c[2] > 0
        xn = c[0] / c[2]; yn = c[1] / c[2]
        u = (Kmat[0, 0] * xn + Kmat[0, 1] * yn) + Kmat[0, 2]
        v = (Kmat[1, 0] * xn + Kmat[1, 1] * yn) + Kmat[1, 2]
    return take, u, v


def int_distances(rows, row):
    """exact integer distances of `rows` [n, D] to one row: Hamming for D = 32, sum of squared differences for D = 128"""
    if rows.shape[1] == 32:
        return np.unpackbits(rows ^ row, axis=1).sum(axis=1).astype(np.int64)
    return ((rows.astype(np.int64) - row.astype(np.int64)) ** 2).sum(axis=1)


def reported(d, sift):
    """cv2's float32 distance of the exact integer d"""
    return np.sqrt(np.float32(d)) if sift else np.float32(d)


def guided_match(map_pts, map_rows, kp_xy, rows, Kmat, P, radius, ratio=0.0, max_distance=0.0):
    """Steps 1 - 7 for one frame -> dict(qi, ti int32; dist, dist2 float32; n_seen; obj, img)."""
    pts = np.asarray(map_pts, np.float64).reshape(-1, 3)
    m = np.ascontiguousarray(map_rows, np.uint8); f = np.ascontiguousarray(rows, np.uint8)
    xy = np.asarray(kp_xy, np.float32).reshape(-1, 2)
    sift = (m.shape[1] if len(m) else f.shape[1] if len(f) else 32) == 128
    x64, y64 = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    take, u, v = project(P, pts, Kmat)
    r2 = float(radius) * float(radius)
    claim = {}                                                             # keypoint -> (d, j, d2 or None)
    n_seen = 0
    for j in np.flatnonzero(take):
        with np.errstate(all="ignore"):
            dx = x64 - u[j]; dy = y64 - v[j]
            cand = np.flatnonzero(dx * dx + dy * dy <= r2)
        if len(cand) == 0:
            continue
        n_seen += 1
        d = int_distances(f[cand], m[j])
        order = np.lexsort((cand, d))
        i, db = int(cand[order[0]]), int(d[order[0]])
        d2 = int(d[order[1]]) if len(cand) > 1 else None
        fd = reported(db, sift); fd2 = FLT_MAX if d2 is None else reported(d2, sift)
        if max_distance > 0 and not float(fd) < float(max_distance):
            continue
        if ratio > 0 and d2 is not None and not float(fd) < float(ratio) * float(fd2):
            continue
        if i not in claim or (db, int(j)) < claim[i][:2]:
            claim[i] = (db, int(j), d2)
    qi = np.array(sorted(claim), np.int32)
    ti = np.array([claim[i][1] for i in qi], np.int32)
    dist = np.array([reported(claim[i][0], sift) for i in qi], np.float32)
    dist2 = np.array([FLT_MAX if claim[i][2] is None else reported(claim[i][2], sift) for i in qi], np.float32)
    return dict(qi=qi, ti=ti, dist=dist, dist2=dist2, n_seen=n_seen, n_match=len(qi), obj=pts[ti].copy().reshape(-1, 3),
                img=xy[qi].astype(np.float64).reshape(-1, 2))


# ------------------------------------------------------------------ the same contract as plain loops
def _popcount_row(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def _ssd_row(a, b):
    return sum((int(x) - int(y)) ** 2 for x, y in zip(a, b))


def guided_match_loops(map_pts, map_rows, kp_xy, rows, Kmat, P, radius, ratio=0.0, max_distance=0.0):
    """guided_match with Python floats (IEEE doubles, one rounding per operation) and explicit loops."""
    pts = [[float(c) for c in p] for p in np.asarray(map_pts, np.float64).reshape(-1, 3)]
    m = np.ascontiguousarray(map_rows, np.uint8); f = np.ascontiguousarray(rows, np.uint8)
    xy = np.asarray(kp_xy, np.float32).reshape(-1, 2)
    xs = [(float(p[0]), float(p[1])) for p in xy]                          # float32 -> float64, exact
    Pm = [float(c) for c in np.asarray(P, np.float64).reshape(12)]; Km = [float(c) for c in np.asarray(Kmat, np.float64).reshape(9)]
    sift = (m.shape[1] if len(m) else f.shape[1] if len(f) else 32) == 128
    dist_of = _ssd_row if sift else _popcount_row
    mrows = [r.tolist() for r in m]; frows = [r.tolist() for r in f]
    r2 = float(radius) * float(radius)
    owner = {}
    n_seen = 0
    for j, (X, Y, Z) in enumerate(pts):
        c = [((Pm[4 * k] * X + Pm[4 * k + 1] * Y) + Pm[4 * k + 2] * Z) + Pm[4 * k + 3] for k in range(3)]
        if not c[2] > 0:
            continue
        xn, yn = c[0] / c[2], c[1] / c[2]                                  # c_2 > 0: an overflowing quotient is inf, as on the device
        u = (Km[0] * xn + Km[1] * yn) + Km[2]
        v = (Km[3] * xn + Km[4] * yn) + Km[5]
        best = None; second = None; cnt = 0
        for i, (x, y) in enumerate(xs):
            dx = x - u; dy = y - v
            if not dx * dx + dy * dy <= r2:
                continue
            d = dist_of(frows[i], mrows[j])
            cnt += 1
            if best is None:
                best = (d, i)
            elif (d, i) < best:
                second = best[0]; best = (d, i)
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
        i = best[1]
        if i not in owner or (best[0], j) < owner[i][:2]:
            owner[i] = (best[0], j, fd, fd2)
    qi = sorted(owner)
    return dict(qi=np.array(qi, np.int32), ti=np.array([owner[i][1] for i in qi], np.int32), dist=np.array([owner[i][2] for i in qi], np.float32),
                dist2=np.array([owner[i][3] for i in qi], np.float32), n_seen=n_seen, n_match=len(qi))


def grid_of(kp_xy):
    """(x0, y0, edge) of k_guided_grid's cells for a frame of finite keypoints within +-2^20 px (docs/kernels/k_map_guided.md)."""
    xy = np.asarray(kp_xy, np.float32).reshape(-1, 2).astype(np.float64)
    if len(xy) == 0:
        return 0.0, 0.0, 1.0
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    return float(lo[0]), float(lo[1]), max(float(max(hi[0] - lo[0], hi[1] - lo[1])) / GRID, 1.0)


def cell_of(x, x0, edge):
    return int(min(max(np.floor((x - x0) * (1.0 / edge)), 0), GRID - 1))


# ------------------------------------------------------------------ cases
# A case: dict(map_rows, map_pts, frames = [(rows, xy)], priors = [P] (one per frame), K, radius, ratio, max_distance, and `expect`:
# what the case is named for, held on the reference by tests/test_guided_reference.py — per frame, any of
#   pairs: (keypoint, point) entries the list must hold; absent_pts / absent_kps: points / keypoints it must not hold;
#   n_match, n_seen: exact counts; seconds: {keypoint: float32 second distance}.
def _width(det):
    return 128 if det == "sift" else 32


def _salt(det):
    return 0 if det == "orb" else 500000


def gen_prior(seed):
    rng = np.random.default_rng(41000 + seed)
    return np.hstack([R.rotation(rng.normal(size=3), rng.uniform(0.02, 0.1)), (np.array([0.1, -0.05, 0.2]) + rng.normal(0, 0.05, 3)).reshape(3, 1)])


def gen_map(det, npt):
    """npt rows and points before the camera of gen_prior (projections within ~130 px of the principal point, so that windows of a
    few pixels overlap), every seventh point BEHIND it; rows (2, 3) and (5, 5 + TILE) duplicated: two points that want one keypoint."""
    rng = np.random.default_rng(42000 + 7 * npt + _salt(det))
    rows = R.rand_rows(rng, npt, det)
    for a, b in ((2, 3), (5, 5 + TILE)):
        if b < npt:
            rows[b] = rows[a]
    pts = np.column_stack([rng.uniform(-0.5, 0.5, npt), rng.uniform(-0.5, 0.5, npt), rng.uniform(4, 8, npt)])
    pts[6::7, 2] *= -1
    for a, b in ((2, 3), (5, 5 + TILE)):                                   # ... and the copies stand almost where their originals stand
        if b < npt:
            pts[b] = pts[a] + 1e-3
    return rows, pts


def gen_frame(det, map_rows, map_pts, P, n, radius, seed=0):
    """n keypoints: three in four sit within 1.3 radius of a map point's projection under P and carry a nudged copy of its row (in
    or out of the window, several per window, several points per keypoint); the rest are random rows in the dense part of the
    image.  Keypoints 10 and 11 (when there) are one row at one position: a tie inside every window that holds them."""
    npt = len(map_rows)
    rng = np.random.default_rng(43000 + 1000 * seed + 7 * npt + n + _salt(det))
    rows = R.rand_rows(rng, n, det)
    xy = rng.uniform(150, 360, (n, 2))
    take, u, v = project(P, map_pts, K_EXACT)
    for i in range(n):
        if npt and i % 4 != 3:
            j = int(rng.integers(0, npt))
            if take[j]:
                a, r = rng.uniform(0, 2 * np.pi), radius * 1.3 * np.sqrt(rng.uniform())
                xy[i] = (u[j] + r * np.cos(a), v[j] + r * np.sin(a))
                rows[i] = R.nudge(map_rows[j], int(rng.integers(0, 3)), det)
    if n > 11:
        rows[11] = rows[10]; xy[11] = xy[10]
    return rows, xy.astype(np.float32)


def size_case(det, npt, sizes=(300, 17, 0), radius=6.0, ratio=0.0, max_distance=0.0):
    """A call of len(sizes) queries with different frames and different priors against the map of npt points."""
    rows, pts = gen_map(det, npt)
    priors = [gen_prior(q) for q in range(len(sizes))]
    frames = [gen_frame(det, rows, pts, priors[q], n, radius, seed=q) for q, n in enumerate(sizes)]
    return dict(map_rows=rows, map_pts=pts, frames=frames, priors=priors, K=K_EXACT, radius=radius, ratio=ratio, max_distance=max_distance,
                expect=[{} for _ in sizes])


def _pt(u, v, z=1.0):
    """the point at depth z that [I | 0] and K_EXACT project to pixel (u, v): exact for pixel coordinates that are multiples of 1/8"""
    return [(u - 256.0) / 512.0 * z, (v - 256.0) / 512.0 * z, z]


def exact_case(det, radius):
    """P = [I | 0], K_EXACT, X and Y multiples of 1/8 and Z in {1, 2, 4}: u, v exact integers.  Keypoint 0 lies at offset (3, 4) from
    point 0, keypoint 2 at offset (5, 0) from point 2 — ON the circle of radius 5 —, keypoint 1 exactly on point 1.  Points 3 .. 6
    must not take part (Z = 0, Z < 0, a NaN coordinate, c_2 = 5e-324 whose u overflows to infinity); keypoints 3 .. 6 carry their
    rows exactly, keypoint 4 where point 4 would land if the sign of Z were ignored."""
    rng = np.random.default_rng(44000 + _salt(det))
    pts = np.array([[0.5, 0.25, 2.0], [-1.0, -0.5, 4.0], [0.125, 0.125, 1.0],
                    [0.5, 0.5, 0.0], [0.25, 0.25, -2.0], [np.nan, 0.0, 1.0], [1.0, 1.0, 5e-324]])
    take, u, v = project(P_IDENTITY, pts, K_EXACT)
    assert list(u[:3]) == [384.0, 128.0, 320.0] and list(v[:3]) == [320.0, 192.0, 320.0]
    map_rows = R.rand_rows(rng, 7, det)
    rows = np.stack([R.nudge(map_rows[0], 1, det), map_rows[1], R.nudge(map_rows[2], 0, det)] + [map_rows[j] for j in (3, 4, 5, 6)])
    xy = np.array([[387, 324], [128, 192], [325, 320], [300, 300], [192, 192], [256, 256], [100, 400]], np.float32)
    on_circle = radius >= 5.0
    e = dict(pairs=[(1, 1)] + ([(0, 0), (2, 2)] if on_circle else []), absent_pts=[3, 4, 5, 6], n_match=3 if on_circle else 1,
             n_seen=3 if on_circle else 1)
    return dict(map_rows=map_rows, map_pts=pts, frames=[(rows, xy)], priors=[P_IDENTITY], K=K_EXACT, radius=radius, ratio=0.0, max_distance=0.0,
                expect=[e])


GRID_BOX = (-160.0, -120.0, 480.0, 520.0)                                  # the grid cases' keypoint box: 640 x 640 px, cells of 10 px


def grid_frame(det):
    """140 keypoints: the two corners of GRID_BOX (keypoints 0, 1: negative coordinates, and beyond any configured width and
    height), chosen keypoints 2 .. 13, the rest random in the box."""
    rng = np.random.default_rng(45000 + _salt(det))
    n = 140
    rows = R.rand_rows(rng, n, det)
    xy = np.column_stack([rng.uniform(GRID_BOX[0], GRID_BOX[2], n), rng.uniform(GRID_BOX[1], GRID_BOX[3], n)])
    xy[0] = GRID_BOX[:2]; xy[1] = GRID_BOX[2:]
    xy[2] = (100.25, 100.25)            # 0.35 px from point 0's projection (100, 100)
    xy[3] = (40, 80)                    # exactly on point 1's projection, which lies on a cell corner
    xy[4] = (-152.5, -111)              # negative coordinates, near point 3
    xy[5] = (475, 515)                  # beyond width and height, near point 4
    xy[6] = (201, 201); xy[7] = (202, 201); rows[7] = rows[6]              # one row twice in one cell (point 5 at (200, 200))
    xy[9] = (299, 300); xy[8] = (301, 300); rows[9] = rows[8]              # ... and in two cells, the LOWER keypoint in the later cell (point 6)
    xy[10] = (100, 300)                 # claimed by points 7 and 8 (one tile) ...
    xy[11] = (300, 100)                 # ... and by points 9 and 9 + TILE (a tile apart), at equal distance
    return rows, xy.astype(np.float32)


def grid_case(det, radius):
    """Windows against the grid: see grid_frame.  Point 2 projects far outside the box, to (5000, 5000)."""
    rng = np.random.default_rng(46000 + _salt(det))
    rows, xy = grid_frame(det)
    npt = 10 + TILE
    map_rows = R.rand_rows(rng, npt, det)
    pts = np.array([_pt(*rng.uniform(-150, 500, 2).round()) for _ in range(npt)])
    for j, (uv, kp, k) in enumerate([((100, 100), 2, 1), ((40, 80), 3, 0), ((5000, 5000), 1, 2), ((-150, -110), 4, 1), ((470, 510), 5, 0),
                                     ((200, 200), 6, 1), ((300, 300), 8, 1), ((100.5, 300), 10, 2), ((99.5, 300), 10, 2), ((300, 100.5), 11, 0)]):
        pts[j] = _pt(*uv)
        map_rows[j] = R.nudge(rows[kp], k, det)
    map_rows[8] = map_rows[7]
    pts[9 + TILE] = _pt(300, 99.5); map_rows[9 + TILE] = map_rows[9]
    e = {}
    if radius == 0.5:
        e = dict(pairs=[(2, 0), (3, 1), (10, 7), (11, 9)], absent_pts=[2, 3, 4, 5, 6, 8, 9 + TILE])
    elif radius == 10.0:
        e = dict(pairs=[(2, 0), (3, 1), (4, 3), (5, 4), (6, 5), (8, 6), (10, 7), (11, 9)], absent_pts=[2, 8, 9 + TILE], absent_kps=[7, 9])
    elif radius >= 7000:
        e = dict(n_seen=npt)
    return dict(map_rows=map_rows, map_pts=pts, frames=[(rows, xy)], priors=[P_IDENTITY], K=K_EXACT, radius=radius, ratio=0.0, max_distance=0.0,
                expect=[e])


def filter_case(det, which):
    """which = 'max_distance': points 0 and 1 each own one keypoint, at reported distances EQUAL to the bound (dropped: the test is
    strict) and below it (kept).  which = 'ratio', ratio 0.8: point 0 has one candidate (kept); point 1 has two equal candidates
    (dropped); point 2 has keypoints 4 and 5 at equal distance in its window and fails the rule, point 3 sees keypoint 4 alone, from
    farther in descriptor space, and keeps it: the filters come before the uniqueness step."""
    rng = np.random.default_rng(47000 + _salt(det))
    rows = R.rand_rows(rng, 8, det)
    xy = np.array([[100, 100], [200, 100], [300, 100], [302, 100], [100, 300], [96, 300], [400, 400], [50, 450]], np.float32)
    if which == "max_distance":
        map_rows = np.stack([R.nudge(rows[0], 3, det), R.nudge(rows[1], 2, det)])       # d = 4, 3: ORB 4.0, 3.0; SIFT 2.0, sqrt(3)
        pts = np.array([_pt(101, 100), _pt(200, 101)])
        bound = 2.0 if det == "sift" else 4.0
        e = dict(pairs=[(1, 1)], absent_pts=[0], n_match=1, n_seen=2)
        return dict(map_rows=map_rows, map_pts=pts, frames=[(rows, xy)], priors=[P_IDENTITY], K=K_EXACT, radius=3.0, ratio=0.0, max_distance=bound,
                    expect=[e])
    rows[3] = rows[2]; rows[5] = rows[4]
    map_rows = np.stack([R.nudge(rows[0], 2, det), R.nudge(rows[2], 1, det), R.nudge(rows[4], 0, det), R.nudge(rows[4], 2, det)])
    pts = np.array([_pt(101, 100), _pt(301, 100), _pt(98, 300), _pt(102.5, 300)])
    e = dict(pairs=[(0, 0), (4, 3)], absent_pts=[1, 2], n_match=2, n_seen=4, seconds={0: FLT_MAX, 4: FLT_MAX})
    return dict(map_rows=map_rows, map_pts=pts, frames=[(rows, xy)], priors=[P_IDENTITY], K=K_EXACT, radius=3.0, ratio=0.8, max_distance=0.0,
                expect=[e])


POSE_RADIUS = 8.0


def pose_prior(c):
    """The generating pose of relocalize_reference.pose_case perturbed by 0.002 rad about a fixed axis and 0.01 units: about 3 px at
    this camera and depth, asserted against POSE_RADIUS on the reference alone by tests/test_guided_reference.py."""
    dR = R.rotation([0.3, -0.5, 0.8], 0.002)
    return np.hstack([dR @ c["R"], (dR @ c["t"] + np.array([0.01, -0.006, 0.008])).reshape(3, 1)])


def pose_case(det):
    c = R.pose_case(det)
    return dict(map_rows=c["map_rows"], map_pts=c["map_pts"], frames=[(c["rows"], c["xy"])], priors=[pose_prior(c)], K=R.K, radius=POSE_RADIUS,
                ratio=0.0, max_distance=0.0, expect=[{}], truth=c)


def named_cases(det):
    cases = {f"exact r={r!r}": exact_case(det, r) for r in (5.0, float(np.nextafter(5.0, 0.0)), 0.0)}
    for r in (0.5, 10.0, 35.0, 7100.0):                                    # half a pixel, one cell edge, 3.5 edges, more than the box and the far point
        cases[f"grid r={r!r}"] = grid_case(det, r)
    cases["filter max_distance"] = filter_case(det, "max_distance")
    cases["filter ratio"] = filter_case(det, "ratio")
    cases["known pose"] = pose_case(det)
    return cases


def all_cases(det, kp_cap=512):
    cases = named_cases(det)
    for npt in MAP_SIZES:
        cases[f"sizes npt={npt}"] = size_case(det, npt)
    cases["sizes frames 1 and kp_cap"] = size_case(det, 257, sizes=(1, kp_cap, 300))
    cases["sizes ratio and bound"] = size_case(det, 257, sizes=(300, 17, 300), ratio=0.9, max_distance=3.5 if det == "sift" else 12.0)
    return cases

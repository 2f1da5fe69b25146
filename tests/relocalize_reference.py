"""The relocalisation operator (vo_map_stage / vo_map_localize; FrontEnd.relocalize) restated with numpy and the CPU oracle, and
the chosen cases the device is held to (not a test module).

The contract (include/vo_hip.h, "relocalisation"), for a map of npt points with one descriptor row each and a frame of n keypoints:
  1 matches = bf.match(frame rows, map rows) with crossCheck=True — oracle.match_l2 for 128-byte SIFT rows (as float32),
    oracle.match_hamming for 32-byte ORB rows, cross_check = 2: strict mutual nearest neighbours, ties to the lower index, ascending
    keypoint order, cv2's float32 distances — then `distance < max_distance` (strict, the float32 value against the double;
    max_distance <= 0: no filter);
  2 obj[k] = map point of trainIdx, img[k] = float64(kp_xy[queryIdx]), in match order;
  3 oracle.solve_pnp_ransac(obj, img, K): fewer than 4 correspondences VO_ERR_TOO_FEW, retval False VO_ERR_NO_MODEL, a model with
    fewer than min_inliers inliers VO_ERR_NO_MODEL with its n_inl; pose = [Rodrigues(rvec) | tvec], zeros when it failed.
`match_map_loops` is the same matcher as two plain loops over a numpy distance table, with no oracle call in it;
tests/test_relocalize_reference.py holds the two equal on every case below, and every case to what its name says.

CHUNK: the rows of the walked side one LDS stage of k_nn_map holds — 128 SIFT rows (NM_STAGE_ROWS), 256 ORB rows (NO_TILE).  A tie
"across two chunks" is a tie between rows whose indices differ in index // CHUNK."""
import numpy as np

from oracle import oracle as O

VO_OK, VO_ERR_INVALID, VO_ERR_TOO_FEW, VO_ERR_NO_MODEL, VO_ERR_NOT_CONFIGURED, VO_ERR_UNSUPPORTED = 0, -1, -3, -4, -5, -7   # include/vo_hip.h
CHUNK = {"sift": 128, "orb": 256}
MAP_SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 129, 257)      # 129, 257: one row past a SIFT chunk, one row past an ORB chunk (and past two SIFT chunks)
FRAME_SIZES = (0, 1, 17, 300)
K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]])


# ------------------------------------------------------------------ the reference
def match_map(frame_rows, map_rows, max_distance=0.0):
    """(keypoint [m], map point [m], distance [m] float32) — step 1 of the contract."""
    f = np.ascontiguousarray(frame_rows, np.uint8); m = np.ascontiguousarray(map_rows, np.uint8)
    if len(f) == 0 or len(m) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    if f.shape[1] == 128:
        qi, ti, d = O.match_l2(f.astype(np.float32), m.astype(np.float32), 2)
    else:
        qi, ti, d = O.match_hamming(f, m, 2)
    assert d.dtype == np.float32
    if max_distance > 0:
        keep = d.astype(np.float64) < float(max_distance)
        qi, ti, d = qi[keep], ti[keep], d[keep]
    return qi, ti, d


def distance_table(frame_rows, map_rows):
    """[n, npt] float32 distances as cv2's batchDistance stores them: sqrtf((float)d^2) with d^2 the exact integer for SIFT rows
    (every partial sum of normL2Sqr_ is an integer below 2^24), the popcount as float for ORB rows."""
    f = np.asarray(frame_rows, np.uint8); m = np.asarray(map_rows, np.uint8)
    out = np.zeros((len(f), len(m)), np.float32)
    for i in range(len(f)):
        if f.shape[1] == 128:
            d2 = ((m.astype(np.int64) - f[i].astype(np.int64)) ** 2).sum(axis=1)
            assert d2.max(initial=0) < (1 << 24)
            out[i] = np.sqrt(d2.astype(np.float32))
        else:
            out[i] = np.unpackbits(m ^ f[i], axis=1).sum(axis=1).astype(np.float32)
    return out


def match_map_loops(frame_rows, map_rows, max_distance=0.0):
    """match_map as two plain loops over the distance table: ascending scans with strict `<` in both directions, then the mutual test."""
    D = distance_table(frame_rows, map_rows)
    n, npt = D.shape
    fwd = [-1] * n
    rev = [-1] * npt
    for i in range(n):
        best = None
        for j in range(npt):
            if best is None or D[i, j] < best:
                best, fwd[i] = D[i, j], j
    for j in range(npt):
        best = None
        for i in range(n):
            if best is None or D[i, j] < best:
                best, rev[j] = D[i, j], i
    qi, ti, d = [], [], []
    for i in range(n):
        j = fwd[i]
        if j >= 0 and rev[j] == i and not (max_distance > 0 and not float(D[i, j]) < float(max_distance)):
            qi.append(i); ti.append(j); d.append(D[i, j])
    return np.array(qi, np.int32), np.array(ti, np.int32), np.array(d, np.float32)


def correspondences(map_points, kp_xy, qi, ti):
    pts = np.asarray(map_points, np.float64).reshape(-1, 3)
    xy = np.asarray(kp_xy, np.float32).reshape(-1, 2)
    return pts[ti].copy(), xy[qi].astype(np.float64)


def relocalize(map_points, map_rows, kp_xy, frame_rows, Kmat, max_distance=0.0, iterations=100, reproj_err=8.0, confidence=0.99,
               seed=0xFFFFFFFFFFFFFFFF, min_inliers=0, matcher=match_map):
    """The whole operator for one frame -> dict(status, pose [3, 4], n_match, n_inl, qi, ti, dist, mask, obj, img, rvec, tvec)."""
    qi, ti, d = matcher(frame_rows, map_rows, max_distance)
    obj, img = correspondences(map_points, kp_xy, qi, ti)
    out = dict(qi=qi, ti=ti, dist=d, obj=obj, img=img, n_match=len(qi), n_inl=0, pose=np.zeros((3, 4)), mask=np.zeros(len(qi), np.uint8),
               rvec=np.zeros(3), tvec=np.zeros(3))
    if len(qi) < 4:
        out["status"] = VO_ERR_TOO_FEW
        return out
    rc, rv, tv, mask, ninl = O.solve_pnp_ransac(obj, img, Kmat, iterations, reproj_err, confidence, seed)
    out.update(status=rc, n_inl=ninl, mask=mask)
    if rc == VO_OK and ninl < min_inliers:
        out["status"] = VO_ERR_NO_MODEL
    if out["status"] == VO_OK:
        out.update(pose=np.hstack([O.rodrigues(rv), tv.reshape(3, 1)]), rvec=rv, tvec=tv)
    return out


# ------------------------------------------------------------------ rows
def rand_rows(rng, n, detector):
    """n descriptor rows: ORB random bytes; SIFT values 0 .. 90 (|row|^2 <= 128 * 90^2 < 2^20, the integer matcher's bound)."""
    if detector == "orb":
        return rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return rng.integers(0, 91, (n, 128), dtype=np.uint8)


def nudge(row, k, detector):
    """A copy of the row at a small distance that grows with k (so that chosen rows have chosen neighbours): k + 1 bits flipped /
    k + 1 elements moved by one."""
    r = row.copy()
    for e in range(k + 1):
        if detector == "orb":
            r[e // 8] ^= np.uint8(1 << (e % 8))
        else:
            r[e] = r[e] + 1 if r[e] < 255 else r[e] - 1
    return r


def match_map_rows(detector, npt):
    """A map of npt rows (and points) with duplicated rows where the kernels fold: a lane apart (2, 3), a 16-column group apart
    (5, 21: the same lane of two groups) and, when the map is large enough, a chunk apart (0, CHUNK), (40, 40 + CHUNK).  The lower
    index must win each of these ties."""
    rng = np.random.default_rng(77000 + 7 * npt + (0 if detector == "orb" else 500000))
    C = CHUNK[detector]
    m = rand_rows(rng, npt, detector)
    for a, b in ((2, 3), (5, 21), (0, C), (40, 40 + C)):                   # (a row, its copy)
        if b < npt:
            m[b] = m[a]
    return m, rng.uniform(-2, 2, (npt, 3)) + [0, 0, 6]


def match_frame(detector, m, n, seed=0):
    """A frame of n rows for the map rows m: every other row a nudged copy of a map row (near neighbours, mutual or not), the
    rest random; rows EQUAL to the duplicated map rows (forward ties at distance 0); and duplicated frame rows — a lane, a group
    and a chunk apart — that are copies of map rows, so the reverse direction meets the same ties."""
    npt = len(m)
    rng = np.random.default_rng(78000 + 1000 * seed + 7 * npt + n + (0 if detector == "orb" else 500000))
    C = CHUNK[detector]
    f = rand_rows(rng, n, detector)
    for i in range(0, n, 2):
        if npt:
            f[i] = nudge(m[int(rng.integers(0, npt))], int(rng.integers(0, 3)), detector)
    for i, j in ((0, 0), (1, 2), (4, 5), (6, 40)):
        if i < n and j < npt:
            f[i] = m[j]
    for a, b in ((10, 11), (12, 28), (4, 4 + C), (14, 14 + 128)):
        if b < n:
            f[b] = f[a]
    return f, rng.uniform(0, 600, (n, 2)).astype(np.float32)


def match_case(detector, npt, n, seed=0):
    m, pts = match_map_rows(detector, npt)
    f, xy = match_frame(detector, m, n, seed)
    return dict(map_rows=m, map_pts=pts, rows=f, xy=xy)


def has_tie_across_chunks(frame_rows, map_rows, detector):
    """Some keypoint's smallest distance is reached by two map rows in different chunks (forward), and some map row's by two
    keypoints in different chunks of the frame (reverse)."""
    D = distance_table(frame_rows, map_rows)
    C = CHUNK[detector]

    def any_tie(T):
        for row in T:
            at = np.flatnonzero(row == row.min())
            if len(at) > 1 and len(set((at // C).tolist())) > 1:
                return True
        return False
    return any_tie(D), any_tie(D.T)


# ------------------------------------------------------------------ poses
def rotation(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * kx @ kx


def pose_case(detector, npt=200, n_wrong=None, seed=0):
    """Known pose: npt exact points, the frame sees all of them at their projections rounded to float32, every point owns a
    distinct row and the frame's keypoints carry the same rows in a seeded permutation — but 10 % of the keypoints (n_wrong) sit at
    a WRONG pixel (their row still matches its point exactly): the 3D-2D outliers solvePnPRansac has to reject."""
    rng = np.random.default_rng(88000 + seed + (0 if detector == "orb" else 500))
    R = rotation(rng.normal(size=3), rng.uniform(0.1, 0.5)); t = np.array([0.3, -0.2, 6.0]) + rng.normal(0, 0.3, 3)
    X = rng.uniform(-2, 2, (npt, 3))
    rows = rand_rows(rng, npt, detector)
    assert len(np.unique(rows, axis=0)) == npt
    Xc = X @ R.T + t
    uv = ((Xc / Xc[:, 2:]) @ K.T)[:, :2]
    perm = rng.permutation(npt)
    n_wrong = npt // 10 if n_wrong is None else n_wrong
    wrong = np.zeros(npt, bool); wrong[rng.choice(npt, n_wrong, replace=False)] = True      # by map point
    uv[wrong] += rng.uniform(40, 120, (n_wrong, 2)) * rng.choice([-1.0, 1.0], (n_wrong, 2))
    return dict(map_rows=rows, map_pts=X, rows=rows[perm], xy=uv[perm].astype(np.float32), R=R, t=t, wrong=wrong[perm], perm=perm)


def too_few_frame(detector, map_rows, seed=0):
    """17 keypoints that all carry one of three map rows (7, 50, 120) exactly: every keypoint's nearest map row is its own, each of
    the three rows answers with the lowest keypoint that carries it, and no other map row is anybody's nearest — exactly three
    mutual matches (keypoints 0, 1, 2), one fewer than solvePnPRansac takes."""
    rng = np.random.default_rng(99000 + seed + (0 if detector == "orb" else 500))
    rows = np.stack([map_rows[(7, 50, 120)[i % 3]] for i in range(17)])
    return rows, rng.uniform(0, 600, (17, 2)).astype(np.float32)


def no_model_frame(detector, map_rows, seed=0):
    """Contradictory data: every keypoint carries its map point's row exactly and sits at a pixel that has nothing to do with it."""
    rng = np.random.default_rng(99500 + seed + (0 if detector == "orb" else 500))
    return map_rows.copy(), rng.uniform(0, 600, (len(map_rows), 2)).astype(np.float32)


def status_case(detector):
    """pose_case's map and three frames for one call: too few matches, no model, the known pose."""
    c = pose_case(detector)
    c["frames"] = [too_few_frame(detector, c["map_rows"]), no_model_frame(detector, c["map_rows"]), (c["rows"], c["xy"])]
    return c

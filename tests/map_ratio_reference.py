"""Ratio-test matching against the staged map (vo_set_map_match modes 1 and 2 of vo_map_localize / vo_map_align; FrontEnd.relocalize
and align_maps with match='ratio' | 'cross+ratio') restated with numpy and the CPU oracle, and the chosen cases the device is held
to (not a test module).

The rule (include/vo_hip.h, vo_set_map_match), for query row i — a keypoint's row or a query map's row: cv2's query — and the staged
map as train:
  m, n = knnMatch(k=2): oracle.knn2_l2 for 128-byte SIFT rows (as float32), oracle.knn2_hamming for 32-byte ORB rows — batchDistance's
  K = 2 insertion: ascending scan, strict `<`, equal distances keep train order; m.trainIdx the lowest index among the nearest rows,
  n.distance the second-smallest distance, a tie with m counting as a second neighbour;
  keep i iff the map has at least 2 rows and float64(m.distance) < ratio * float64(n.distance) on cv2's float32 distances;
  `m.distance < max_distance` (strict, <= 0: no filter) applies as well; ascending query order; several query rows may keep one map row.
mode 1 is that; mode 2 is tests/relocalize_reference.match_map (the cross-check, mode 0) filtered by the same rule on the forward
neighbours.  Then relocalize_reference.correspondences + oracle.solve_pnp_ransac, or map_align_reference.sim3_ransac.
`match_loops` is the same matcher as two plain loops over relocalize_reference.distance_table with no oracle call in it;
tests/test_map_ratio_reference.py holds the two equal on every case below, and every case to what its name says."""
import numpy as np

from oracle import oracle as O

import map_align_reference as A
import relocalize_reference as RR

VO_OK, VO_ERR_INVALID, VO_ERR_TOO_FEW, VO_ERR_NO_MODEL = RR.VO_OK, RR.VO_ERR_INVALID, RR.VO_ERR_TOO_FEW, RR.VO_ERR_NO_MODEL
K = RR.K
RATIO = 0.75
MAP_SIZES = (0, 1, 2, 3, 17, 63, 64, 65, 129, 257)
FRAME_SIZES = (0, 1, 17, 300)
FLT_MAX = np.finfo(np.float32).max
_EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))


# ------------------------------------------------------------------ the reference
def knn2(frame_rows, map_rows):
    """(idx [n, 2] int32, dist [n, 2] float32) of knnMatch(frame, map, k=2); missing neighbours -1 / FLT_MAX."""
    f = np.ascontiguousarray(frame_rows, np.uint8); m = np.ascontiguousarray(map_rows, np.uint8)
    if f.shape[1] == 128:
        return O.knn2_l2(f.astype(np.float32), m.astype(np.float32))
    return O.knn2_hamming(f, m)


def ratio_keeps(d, d2, ratio):
    """The rule on float32 arrays: float64(d) < ratio * float64(d2)."""
    return np.asarray(d, np.float32).astype(np.float64) < float(ratio) * np.asarray(d2, np.float32).astype(np.float64)


def match(frame_rows, map_rows, mode, ratio=RATIO, max_distance=0.0):
    """(query row [k], map row [k], distance [k] float32, second distance [k] float32) in modes 1 and 2."""
    assert mode in (1, 2)
    f = np.ascontiguousarray(frame_rows, np.uint8); m = np.ascontiguousarray(map_rows, np.uint8)
    if len(f) == 0 or len(m) < 2:
        return _EMPTY
    idx, dist = knn2(f, m)
    assert dist.dtype == np.float32
    keep = ratio_keeps(dist[:, 0], dist[:, 1], ratio)
    if mode == 1:
        if max_distance > 0:
            keep &= dist[:, 0].astype(np.float64) < float(max_distance)
        qi = np.flatnonzero(keep).astype(np.int32)
        return qi, idx[qi, 0].astype(np.int32), dist[qi, 0].copy(), dist[qi, 1].copy()
    qi, ti, d = RR.match_map(f, m, max_distance)
    assert np.array_equal(ti, idx[qi, 0]) and np.array_equal(d, dist[qi, 0])      # the cross-check's forward neighbour is knnMatch's m
    k = keep[qi]
    return qi[k], ti[k], d[k], dist[qi[k], 1].copy()


def match_loops(frame_rows, map_rows, mode, ratio=RATIO, max_distance=0.0):
    """`match` as two plain loops over the distance table: the K = 2 insertion with strict `<`, the rule, and for mode 2 the mutual
    test against the reverse scan."""
    D = RR.distance_table(frame_rows, map_rows)
    n, npt = D.shape
    rows = D.tolist()
    rev = [-1] * npt
    if mode == 2:
        for j in range(npt):
            best = None
            for i in range(n):
                if best is None or rows[i][j] < best:
                    best, rev[j] = rows[i][j], i
    qi, ti, d, d2 = [], [], [], []
    for i in range(n):
        b0 = b1 = None; j0 = -1
        for j in range(npt):
            v = rows[i][j]
            if b0 is None or v < b0:
                b1, b0, j0 = b0, v, j
            elif b1 is None or v < b1:
                b1 = v
        if b1 is None or not (float(b0) < float(ratio) * float(b1)):
            continue
        if max_distance > 0 and not float(b0) < float(max_distance):
            continue
        if mode == 2 and rev[j0] != i:
            continue
        qi.append(i); ti.append(j0); d.append(b0); d2.append(b1)
    return np.array(qi, np.int32), np.array(ti, np.int32), np.array(d, np.float32), np.array(d2, np.float32)


def relocalize(map_points, map_rows, kp_xy, frame_rows, Kmat, mode, ratio=RATIO, max_distance=0.0, iterations=100, reproj_err=8.0, confidence=0.99,
               seed=0xFFFFFFFFFFFFFFFF, min_inliers=0):
    """relocalize_reference.relocalize with this matcher; the dict gains dist2."""
    got = {}

    def matcher(f, m, md):
        got["m"] = match(f, m, mode, ratio, md)
        return got["m"][:3]
    out = RR.relocalize(map_points, map_rows, kp_xy, frame_rows, Kmat, max_distance, iterations, reproj_err, confidence, seed, min_inliers, matcher=matcher)
    out["dist2"] = got["m"][3]
    return out


def map_align(map_rows, map_pts, q_rows, q_pts, max_error, mode, ratio=RATIO, max_distance=0.0, **kw):
    """map_align_reference.map_align with this matcher; the dict gains dist2."""
    bi, ai, d, d2 = match(q_rows, map_rows, mode, ratio, max_distance)
    src = np.asarray(q_pts, np.float64).reshape(-1, 3)[bi].copy(); dst = np.asarray(map_pts, np.float64).reshape(-1, 3)[ai].copy()
    out = A.sim3_ransac(src, dst, max_error, **kw)
    out.update(bi=bi, ai=ai, dist=d, dist2=d2, src=src, dst=dst, n_match=len(bi))
    return out


# ------------------------------------------------------------------ cases: every size
def size_case(detector, npt, n, seed=0):
    """relocalize_reference.match_case at this module's sizes: nudged copies of map rows (kept by the rule unless the row they copy
    is duplicated in the map), random rows (rejected: every map row is about as far), exact copies of the duplicated map rows (a tie
    for nearest at distance 0: rejected) and duplicated frame rows (two query rows that keep one map row)."""
    return RR.match_case(detector, npt, n, seed)


def call_frames(detector, npt):
    """The three frames of unequal size of one call, twice: sizes (300, 17, 0) and (1, 300, 17) of one map."""
    c = {n: size_case(detector, npt, n) for n in FRAME_SIZES}
    m, pts = c[0]["map_rows"], c[0]["map_pts"]
    assert all(np.array_equal(v["map_rows"], m) for v in c.values())
    return m, pts, {n: (c[n]["rows"], c[n]["xy"]) for n in FRAME_SIZES}


# ------------------------------------------------------------------ cases: chosen first and second neighbours
def move(row, elements, detector):
    """A copy of the row with the given element (SIFT: + 1 each, d^2 = their number) / bit (ORB: flipped, d = their number) indices moved."""
    r = row.copy()
    for e in elements:
        if detector == "orb":
            r[e // 8] ^= np.uint8(1 << (e % 8))
        else:
            r[e] += 1
    return r


# name -> (map row of the nearest, map row(s) of the second, distance of the nearest, of the second).  SIFT walks the map in chunks of
# 128 rows = 8 groups of 16 columns, lane l of a 16-lane group holding columns l, l + 16, ...; ORB in chunks of 256 rows.
PLACEMENTS = {
    "one lane, second after":        (32, (48,), 1, 2),
    "one lane, second before":       (49, (33,), 1, 2),
    "two lanes, second after":       (70, (75,), 1, 2),
    "two lanes, second before":      (77, (71,), 1, 2),
    "two groups, second after":      (3, (100,), 1, 2),
    "two groups, second before":     (101, (6,), 1, 2),
    "two chunks, second after":      (20, (155,), 1, 2),
    "two chunks, second before":     (156, (21,), 1, 2),
    "256 apart, second after":       (60, (325,), 1, 2),
    "256 apart, second before":      (326, (61,), 1, 2),
    "three chunks apart, after":     (90, (590,), 1, 2),
    "three chunks apart, before":    (591, (91,), 1, 2),
    "tie for nearest, one lane":     (200, (216,), 1, 1),
    "tie for nearest, two chunks":   (470, (210,), 1, 1),
    "tie for second, two chunks":    (230, (240, 500), 1, 2),
    "tie for second, one lane":      (250, (266, 282), 1, 2),
    "bound: 3 against 4":            (300, (310,), 3, 4),       # 3 < 0.75 * 4 is false: `<` is strict
    "bound: 3 against 5":            (340, (350,), 3, 5),       # 3 < 3.75
}
SHARED = (len(PLACEMENTS), 0, 32)       # frame row 18 keeps the map row frame row 0 keeps
PLACEMENT_NPT = 600


def moves(dist, detector):
    """Elements / bits to move for cv2 to report `dist`: SIFT d^2 = their number, ORB d = their number."""
    return dist * dist if detector == "sift" else dist


def placement_case(detector):
    """A map of 600 random rows and a frame of 40: frame row i < len(PLACEMENTS) is a random row f_i of its own, and the map rows its
    placement names are copies of f_i at the stated distances (disjoint elements / bits for the nearest and for the second, so the
    copies differ from each other too; two `second` rows are the same copy).  Frame row SHARED[0] is a copy of MAP row 32 two moves
    away, so it keeps the map row that frame row 0 keeps.  The other rows are random."""
    rng = np.random.default_rng(91000 + (0 if detector == "orb" else 500))
    m = RR.rand_rows(rng, PLACEMENT_NPT, detector)
    names = list(PLACEMENTS)
    f = RR.rand_rows(rng, 40, detector)
    for i, name in enumerate(names):
        first, seconds, d1, d2 = PLACEMENTS[name]
        m[first] = move(f[i], range(0, moves(d1, detector)), detector)
        for s in seconds:
            m[s] = move(f[i], range(40, 40 + moves(d2, detector)), detector)
    f[SHARED[0]] = move(m[SHARED[2]], (100, 101), detector)
    pts = rng.uniform(-2, 2, (PLACEMENT_NPT, 3)) + [0, 0, 6]
    return dict(map_rows=m, map_pts=pts, rows=f, xy=rng.uniform(0, 600, (40, 2)).astype(np.float32), names=names)


def long_map_case(detector):
    """npt = 65536 and a 17-row frame: frame row 0 has its nearest at map row 65535 (1 moved) and its second at map row 0 (4 moved),
    frame row 1 the other way round (nearest row 0, second row 65535) — the two map rows are three moves apart."""
    rng = np.random.default_rng(92000 + (0 if detector == "orb" else 500))
    npt = 65536
    m = RR.rand_rows(rng, npt, detector)
    f = RR.rand_rows(rng, 17, detector)
    m[0] = move(m[npt - 1], (0, 1, 2), detector)
    f[0] = move(m[npt - 1], (50,), detector)
    f[1] = move(m[0], (60,), detector)
    return dict(map_rows=m, map_pts=rng.uniform(-2, 2, (npt, 3)) + [0, 0, 6], rows=f, xy=rng.uniform(0, 600, (17, 2)).astype(np.float32))


# ------------------------------------------------------------------ cases: two maps
def align_case(detector, npt, n, n_distractors=12, gen=0):
    """map_align_reference.align_case with distractor rows appended to the staged map: for n_distractors of the pairs the cross-check
    matches, a second copy of the STAGED row, with a point that lies elsewhere.  The query row is then as far from the copy as from the
    row it was matched to — a tie for nearest, n.distance == m.distance — so the ratio rule rejects it for every ratio <= 1, while the
    cross-check still keeps it (the lower index wins the tie).  c["distracted"]: those query rows."""
    c = A.align_case(detector, npt, n, gen=gen)
    rng = np.random.default_rng(93000 + 7 * npt + n + (0 if detector == "orb" else 500))
    bi, ai, _ = RR.match_map(c["rows"], c["map_rows"])
    pick = rng.permutation(len(bi))[:min(n_distractors, len(bi) // 3)]
    extra = c["map_rows"][ai[pick]]
    c["map_rows"] = np.concatenate([c["map_rows"], extra])
    c["map_pts"] = np.concatenate([c["map_pts"], rng.uniform(-40, 40, (len(extra), 3))])
    c["distracted"] = bi[pick]
    return c


ALIGN_MAPS = (513, 257, 3)           # staged rows before the distractors, in the order the GPU test stages them (the smaller maps then
ALIGN_QUERIES = (257, 0, 65, 64, 1, 2, 3)   # lie in an allocation that still holds the larger one); query maps of one call: 257, 0, 65 / 64, 1, 2, 3


def align_call(detector, npt):
    """One staged map — align_case(detector, npt, 257)'s, distractors included — and every query map of ALIGN_QUERIES against it:
    (map_rows, map_pts, {n: (rows, points)}, the 257-row query's distracted rows)."""
    big = align_case(detector, npt, 257)
    q = {}
    for n in ALIGN_QUERIES:
        c = A.align_case(detector, npt, n)
        assert np.array_equal(c["map_rows"], big["map_rows"][:npt])
        q[n] = (c["rows"], c["pts"])
    assert np.array_equal(q[257][0], big["rows"])
    return big["map_rows"], big["map_pts"], q, big["distracted"], big

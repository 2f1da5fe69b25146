"""A plain numpy statement of what the batched Hamming matchers (k_nn_fp4 / k_nn_mfma / k_nn_pairs -> k_match_select) compute for
32-byte ORB descriptor rows (cv2.BFMatcher(NORM_HAMMING)), and the seeded row sets the matcher's tests run on.

Written independently of the oracle's C (oracle/voo_match.c): tests/test_hamming_reference.py puts the two in agreement on every
case, and holds every case to what it is named for, before tests/test_gpu_match_orb_rows.py compares the device with this file.

Distances: with the 256 bits of a row written as +1 / -1, hamming = (256 - a.b) / 2.  The product runs as a float32 matmul:
every partial sum is an integer of magnitude <= 256, so the result is exact whatever order BLAS sums in.  Query rows go through in
chunks and only the two nearest of every row are kept, so a 16128-row set costs no more memory than a small one
(np.unpackbits of the XOR cube needs nq * nt * 256 bytes: test_hamming_reference.py uses it on the small cases as the check).
batchDistance selects with strict `<` in ascending train order: the lowest index among equals."""
import functools

import numpy as np

RATIO = 0.75
MODES = ("nearest", "legacy", "mutual", "ratio")      # k_match_select's modes 0, 1, 2, 3
KERNELS = ("mfma_fp4", "mfma", "popcount")            # vo_set_matcher_kernel
CHUNK = 1024


def kernel_for(setter, kp_cap):
    """The kernel vo_api.hip's nn_kernel rule runs for `setter` at a capacity: the matrix-core forms carry the column index in the
    accumulator (FP4: fewer than 8192 rows; int8: fewer than 127^2 = 16129) and fall back silently above."""
    if setter == "popcount" or kp_cap >= 16129:
        return "popcount"
    return "mfma_fp4" if setter == "mfma_fp4" and kp_cap < 8192 else "mfma"


def kp_cap_for(nfeatures):
    return (nfeatures + max(nfeatures // 8, 256) + 7) // 8 * 8


def pm1(rows):
    """[n, 32] uint8 -> [n, 256] float32 of +1 (bit set) / -1."""
    rows = np.asarray(rows, np.uint8).reshape(-1, 32)
    return np.unpackbits(rows, axis=1, bitorder="little").astype(np.float32) * 2.0 - 1.0


def hamming_matrix(q, t):
    """int32 [nq, nt], whole: for the small cases."""
    return ((256.0 - pm1(q) @ pm1(t).T) * 0.5).astype(np.int32)


def two_nearest(D):
    """idx [n, k], d [n, k] with k = min(2, columns): the first two columns of np.argsort(D, axis=1, kind='stable'), taken as two
    argmin passes (argmin returns the first, i.e. lowest, index of the minimum)."""
    n, m = D.shape
    k = min(2, m)
    idx = np.zeros((n, k), np.int64); d = np.zeros((n, k), np.int32)
    if n == 0 or k == 0:
        return idx, d
    rows = np.arange(n)
    idx[:, 0] = np.argmin(D, axis=1); d[:, 0] = D[rows, idx[:, 0]]
    if k == 2:
        M = D.copy(); M[rows, idx[:, 0]] = 1 << 20
        idx[:, 1] = np.argmin(M, axis=1); d[:, 1] = D[rows, idx[:, 1]]
    return idx, d


def two_nearest_rows(q, t):
    """two_nearest(hamming_matrix(q, t)) without the whole matrix: CHUNK query rows at a time."""
    nq, nt = len(q), len(t)
    k = min(2, nt)
    idx = np.zeros((nq, k), np.int64); d = np.zeros((nq, k), np.int32)
    if nq == 0 or k == 0:
        return idx, d
    B = np.ascontiguousarray(pm1(t).T)
    for a in range(0, nq, CHUNK):
        D = ((256.0 - pm1(q[a:a + CHUNK]) @ B) * 0.5).astype(np.int32)
        idx[a:a + CHUNK], d[a:a + CHUNK] = two_nearest(D)
    return idx, d


class Pair:
    """Everything the four rules need of one (query, train) pair, computed once."""

    def __init__(self, q, t):
        self.q, self.t = np.asarray(q, np.uint8).reshape(-1, 32), np.asarray(t, np.uint8).reshape(-1, 32)
        self.nq, self.nt = len(self.q), len(self.t)
        self.fidx, self.fd = two_nearest_rows(self.q, self.t)
        self.ridx, self.rd = two_nearest_rows(self.t, self.q)

    @functools.cached_property
    def D(self):
        return hamming_matrix(self.q, self.t)

    def knn2(self):
        """(idx [nq, k], float32 dist [nq, k]), k = min(2, nt): knnMatch(k=2)."""
        return self.fidx, self.fd.astype(np.float32)

    def select(self, mode, ratio=RATIO):
        """(query, train, float32 distance) of the matches, ascending query: k_match_select's rule `mode` (a name of MODES)."""
        nq, nt = self.nq, self.nt
        if nq == 0 or nt == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
        f0 = self.fidx[:, 0]; fd = self.fd[:, 0].astype(np.float32)
        if mode == "nearest":                              # BFMatcher(crossCheck=False).match
            keep = np.ones(nq, bool); ti = f0; d = fd
        elif mode == "mutual":                             # cv2 4.x crossCheck=True: the train row's own nearest query must be q
            keep = self.ridx[f0, 0] == np.arange(nq); ti = f0; d = fd
        elif mode == "legacy":
            # per query the minimum of (dist, train) over the train rows whose reverse nearest neighbour it is
            r0 = self.ridx[:, 0]; rd = self.rd[:, 0]
            ti = np.full(nq, -1, np.int64); best = np.full(nq, 1 << 20, np.int64)
            for t in range(nt):                            # ascending train, strict <: the earliest of equals stays
                q = r0[t]
                if rd[t] < best[q]:
                    best[q] = rd[t]; ti[q] = t
            keep = ti >= 0; d = best.astype(np.float32)
        elif mode == "ratio":                              # knnMatch(k=2) + `m.distance < ratio * n.distance` on the float distances
            if nt < 2:
                keep = np.zeros(nq, bool)
            else:
                keep = fd.astype(np.float64) < float(ratio) * self.fd[:, 1].astype(np.float32).astype(np.float64)
            ti = f0; d = fd
        else:
            raise ValueError(mode)
        return np.nonzero(keep)[0], ti[keep], d[keep].astype(np.float32)


# ------------------------------------------------------------------ seeded row generators, all uint8 [n][32]
def rand_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flipped(rng, rows, lo=1, hi=12):
    """Copies of `rows` with lo .. hi distinct bits flipped in each: the nearest neighbour of a copy is, as a rule, its source
    (two random rows lie 128 +- 8 apart)."""
    rows = np.asarray(rows, np.uint8).reshape(-1, 32).copy()
    for r in rows:
        for b in rng.choice(256, int(rng.integers(lo, hi + 1)), replace=False):
            r[b >> 3] ^= np.uint8(1 << (b & 7))
    return rows


def at_distance(rng, row, k):
    """`row` with exactly k bits flipped."""
    return flipped(rng, row[None], k, k)[0]


def tie_rows(rng, base, n, first_two):
    """n rows drawn with repetition from the rows of `base`.  first_two: {base row: (i, j)}: that row's first two occurrences are
    forced to columns i < j (it appears nowhere else below j), so that the first and second neighbour of a query equal to it are
    tied at columns the caller chose.  An entry with j >= n is left out."""
    src = rng.integers(0, len(base), n)
    use = {b: ij for b, ij in first_two.items() if ij[1] < n}
    fill = [b for b in range(len(base)) if b not in use]
    for b, (i, j) in use.items():
        for c in range(j):
            if src[c] == b:
                src[c] = fill[c % len(fill)]
    for b, (i, j) in use.items():
        src[i] = b; src[j] = b
    return base[src], src


class Group:
    """Row sets that share one FrontEnd (one kp_cap), and the launches run on them: every launch is a list of pairs that goes to
    the device in ONE run_pairs call.  modes / kernels / ratios: what the GPU test runs the group under (ratios: ratio mode once
    per value)."""

    def __init__(self, name, nfeatures, sets, launches, ratios=(RATIO,), modes=MODES, kernels=KERNELS):
        self.name, self.nfeatures, self.kp_cap, self.sets, self.launches = name, nfeatures, kp_cap_for(nfeatures), sets, launches
        self.ratios, self.modes, self.kernels = ratios, modes, kernels
        self.pairs = sorted({p for l in launches for p in l}, key=str)
        self._ref = {}

    def ref(self, a, b):
        if (a, b) not in self._ref:
            self._ref[(a, b)] = Pair(self.sets[a], self.sets[b])
        return self._ref[(a, b)]


FLAGSHIP_NFEATURES = 2000                              # kp_cap 2256: bench.py's; five 512-row blocks

REMAINDER_COUNTS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025, 1537, 2255, 2256)


def _remainders():
    # the 16-column group, two groups per FP4 step, the 64 rows of a wave and of the int8 stage, the 128-row FP4 stage, the 256-row
    # popcount tile, the 512-row block; sets are perturbed copies of one pool's prefix, so every pair has true neighbours
    rng = np.random.default_rng(9101)
    pool = rand_rows(rng, max(REMAINDER_COUNTS))
    sets = {n: flipped(rng, pool[:n])[rng.permutation(n)] for n in REMAINDER_COUNTS}       # (2256, n == kp_cap, is the last slot)
    launches = [
        [(1, 2256), (2256, 1), (0, 513), (513, 0), (2255, 2255), (15, 1537), (1537, 16), (17, 2255)],       # 8 pairs: 40 workgroups
        [(2, 1025), (1025, 2), (31, 32), (32, 33), (33, 31), (2256, 2255), (2255, 2256)],                   # 7 pairs: 35 workgroups
        [(63, 64), (64, 65), (65, 63), (127, 128), (128, 129), (129, 127), (0, 0), (1537, 2256)],
        [(255, 256), (256, 257), (257, 255), (511, 512), (512, 513), (513, 511), (16, 1025)],
    ]
    launches += [l[::-1] for l in launches]              # once more reversed: a pair's result does not depend on its index
    return Group("remainders", FLAGSHIP_NFEATURES, sets, launches)


# columns of the tied first and second neighbour, by query (= base row)
TIE_COLUMNS = {0: (3, 9),        # inside one 16-column group
               1: (37, 53),      # columns j and j + 16: the two groups (2 and 3) of one FP4 step
               2: (100, 200),    # across the 128-row FP4 stage
               3: (60, 70),      # across the 64-row int8 stage, inside one FP4 stage
               4: (250, 260),    # across the 256-row popcount tile
               5: (500, 520)}    # across the 512-row block (t900 only)
# equal QUERY rows (i, j), both the exact copy of one train row (TIE_QUERY_TRAIN): the reverse direction's ties
TIE_QUERY_ROWS = ((4, 6),        # inside a lane's row quad (rows 4 k .. 4 k + 3)
                  (21, 40),      # across 16-row blocks of one wave
                  (70, 130),     # across waves (64 rows each)
                  (300, 900))    # across 512-row blocks: decided in k_match_select's merge of the FP4 single pass
TIE_QUERY_TRAIN = (10, 11, 12, 13)
# ratio boundaries: (d0, d1) of query i's two nearest train rows.  ratio * d1 == d0 exactly at (40, 80) for 0.5 and at (3, 4) for
# 0.75: the strict `<` drops those and keeps their neighbours
RATIO_EDGE_DISTANCES = ((40, 80), (39, 80), (40, 81), (3, 4), (2, 4), (3, 5))
TIE_RATIOS = (0.5, 0.75, 1.0, 1.5)     # above 1: queries whose two neighbours tie at a distance > 0 are kept, and show which came first


def _ties():
    rng = np.random.default_rng(9102)
    base = rand_rows(rng, 12)
    t280, _ = tie_rows(rng, base, 280, TIE_COLUMNS)
    t900, _ = tie_rows(rng, base, 900, TIE_COLUMNS)
    q300 = base[np.r_[0:12, rng.integers(0, 12, 288)]].copy()
    near = rng.random(300) < 0.25        # a quarter of the queries lie NEAR a base row: ties at a distance > 0
    near[:12] = False
    q300[near] = flipped(rng, q300[near], 1, 3)
    q17 = base[np.r_[0:12, rng.integers(0, 12, 5)]].copy()
    # duplicates among the query rows
    qd = rand_rows(rng, 1100)
    for i, j in TIE_QUERY_ROWS:
        qd[j] = qd[i]
    td = flipped(rng, qd[rng.choice(np.arange(400, 900), 300, replace=False)])
    for c, (i, j) in zip(TIE_QUERY_TRAIN, TIE_QUERY_ROWS):
        td[c] = qd[i]
    # every distance 0 or 256
    zeros40, ones50 = np.zeros((40, 32), np.uint8), np.full((50, 32), 255, np.uint8)
    mix600 = np.where(rng.random(600) < 0.5, 0, 255).astype(np.uint8)[:, None].repeat(32, 1)
    mix530 = np.where(rng.random(530) < 0.5, 0, 255).astype(np.uint8)[:, None].repeat(32, 1)
    # ratio boundaries
    rq = rand_rows(rng, len(RATIO_EDGE_DISTANCES))
    rt = rand_rows(rng, 300)
    for i, (d0, d1) in enumerate(RATIO_EDGE_DISTANCES):
        rt[20 * i + 7] = at_distance(rng, rq[i], d1); rt[20 * i + 13] = at_distance(rng, rq[i], d0)
    sets = {"q300": q300, "t280": t280, "q17": q17, "t900": t900, "qd1100": qd, "td300": td, "zeros40": zeros40, "ones50": ones50,
            "mix600": mix600, "mix530": mix530, "rq": rq, "rt": rt}
    pairs = [("q300", "t280"), ("q17", "t900"), ("t280", "q300"), ("qd1100", "td300"), ("td300", "qd1100"), ("zeros40", "ones50"),
             ("ones50", "zeros40"), ("mix600", "mix530"), ("mix530", "mix600"), ("mix600", "mix600"), ("rq", "rt")]
    return Group("ties", FLAGSHIP_NFEATURES, sets, [pairs], ratios=TIE_RATIOS)


SHRINK_STEPS = ("s2256", "s17", "s0")


def _shrink():
    """One slot holds 2256 rows, then 17, then none.  Rows 17.. of the full frame are exact copies of the other set's rows (in every
    512-row block), the 17 that stay are only near some of them: whatever reads past the count finds a distance 0."""
    rng = np.random.default_rng(9103)
    o = rand_rows(rng, 2200)
    s = rand_rows(rng, 2256)
    s[:17] = flipped(rng, o[rng.choice(2200, 17, replace=False)], 4, 12)
    s[17:2217] = o
    s[2217:] = o[:39]
    sets = {"o2200": o, "s2256": s, "s17": s[:17].copy(), "s0": s[:0].copy()}
    launches = [[(k, "o2200"), ("o2200", k)] for k in SHRINK_STEPS]      # as query and as train; the same pair indices every step
    return Group("shrink", FLAGSHIP_NFEATURES, sets, launches)


def _single_pass_edge(nfeatures, na, nb):
    """The FP4 single pass runs up to kp_cap 4096 (NN_COLS_MAX), the two-sweep launch above.  Perturbed copies, with winners in the
    last column group and in the last row block, both ways round."""
    rng = np.random.default_rng(9104 + nfeatures)
    b = rand_rows(rng, nb)
    others = np.setdiff1d(np.arange(nb), [3, nb - 2, nb - 1])            # (the three rows below have one copy each)
    a = flipped(rng, b[np.r_[rng.permutation(others), 0, 1, 2][:na]])
    a[5] = flipped(rng, b[nb - 1:nb])[0]              # query 5 -> the last column
    a[na - 1] = flipped(rng, b[3:4])[0]               # the last query row -> column 3
    a[na - 2] = flipped(rng, b[nb - 2:nb - 1])[0]     # last row block -> last column group
    sets = {f"a{na}": a, f"b{nb}": b}
    pairs = [(f"a{na}", f"b{nb}"), (f"b{nb}", f"a{na}")]
    return Group(f"edge{kp_cap_for(nfeatures)}", nfeatures, sets, [pairs], modes=("nearest", "mutual"), kernels=("mfma_fp4",))


# kp_cap: (nfeatures, the kernel nn_kernel picks under the setter mfma_fp4)
INDEX_LIMITS = {8184: (7275, "mfma_fp4"), 8192: (7282, "mfma"), 16128: (14336, "mfma"), 16136: (14337, "popcount")}
LIMIT_LAST, LIMIT_FIRST = slice(0, 10), slice(10, 20)      # rows of "small": near the last row of bigA; near row 0 of both


def _index_limit(cap):
    """The last admissible column index of the kernels that carry it in the accumulator (8183 of MF_S = 8192, 16127 of MM_S =
    16129), and the first capacity of each silent fallback.  bigA: the last row is the only neighbour of small[0:10].  bigB: the
    last row is an exact duplicate of row 0, the neighbour of small[10:20]: row 0 wins."""
    nfeatures, kernel = INDEX_LIMITS[cap]
    rng = np.random.default_rng(9105 + cap)
    bigA = rand_rows(rng, cap)
    small = flipped(rng, bigA[rng.choice(np.arange(1, cap - 1), 600, replace=False)])
    small[LIMIT_LAST] = flipped(rng, bigA[cap - 1:cap].repeat(10, 0))
    small[LIMIT_FIRST] = flipped(rng, bigA[0:1].repeat(10, 0))
    bigB = bigA.copy(); bigB[cap - 1] = bigB[0]
    sets = {"small": small, "bigA": bigA, "bigB": bigB}
    pairs = [("small", "bigA"), ("bigA", "small"), ("small", "bigB"), ("bigB", "small")]
    if cap == 8184:
        pairs.append(("bigB", "bigB"))                  # the whole 8184 x 8184 matrix: every column index there is
    modes = ("nearest", "mutual", "ratio") + (("legacy",) if cap == 16128 else ())       # legacy: the kp_cap * 8-byte LDS opt-in
    g = Group(f"limit{cap}", nfeatures, sets, [pairs], modes=modes, kernels=("mfma_fp4",))
    g.kernel = kernel
    return g


GROUPS = ("remainders", "ties", "shrink", "edge4096", "edge4104") + tuple(f"limit{c}" for c in INDEX_LIMITS)


def kernels_of(name):
    """group(name).kernels without building the group (for parametrize): the edge and limit groups keep the setter at mfma_fp4."""
    return ("mfma_fp4",) if name.startswith(("edge", "limit")) else KERNELS


@functools.lru_cache(maxsize=None)
def group(name):
    """The case groups of tests/test_gpu_match_orb_rows.py, built once per process; their references are cached in them."""
    if name.startswith("limit"):
        return _index_limit(int(name[5:]))
    if name == "edge4096":
        return _single_pass_edge(3641, 4095, 4096)
    if name == "edge4104":
        return _single_pass_edge(3648, 4097, 4104)
    return {"remainders": _remainders, "ties": _ties, "shrink": _shrink}[name]()

"""A plain numpy statement of what k_nn_l2i8 + k_match_select compute for 128-element descriptor rows of integers 0..255
(cv2.BFMatcher(NORM_L2) on SIFT rows), and the seeded row sets the matcher's tests run on.

Written independently of the oracle's C (oracle/voo_match.c): tests/test_l2i8_reference.py puts the two in agreement on every
case before tests/test_gpu_match_l2i8.py compares the device with this file.

Distances: D2 = |q|^2 + |t|^2 - 2 q.t^T in a float64 matmul.  Every value is an integer below 2^53, so the result is exact
whatever order BLAS sums in.  batchDistance hands out sqrtf(D2) as float32 and selects with strict `<` in ascending train
order, i.e. the lowest index among equals: sqrtf is strictly increasing on the integers below 2^22
(tests/test_oracle_properties.py), which is why ordering by the integer D2 is the same selection."""
import functools

import numpy as np

RATIO = 0.8
MODES = ("nearest", "legacy", "mutual", "ratio")      # k_match_select's modes 0, 1, 2, 3
NORM_BOUND = 1 << 20                                  # |row|^2 above it: k_sb_descriptor's flag (bit 1)


def d2_matrix(q, t):
    q = np.asarray(q, np.float64).reshape(-1, 128); t = np.asarray(t, np.float64).reshape(-1, 128)
    return (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2.0 * (q @ t.T)


def two_nearest(D2):
    """idx [nq, k], d2 [nq, k] with k = min(2, nt): the first two columns of np.argsort(D2, axis=1, kind='stable').
    Taken as two argmin passes (argmin returns the first, i.e. lowest, index of the minimum), which is the same thing and does not
    sort 4100 x 4100 values; test_l2i8_reference.py::test_two_nearest_is_the_stable_argsort holds the two together."""
    nq, nt = D2.shape
    k = min(2, nt)
    idx = np.zeros((nq, k), np.int64); d2 = np.zeros((nq, k), np.float64)
    if nq == 0 or k == 0:
        return idx, d2
    rows = np.arange(nq)
    idx[:, 0] = np.argmin(D2, axis=1); d2[:, 0] = D2[rows, idx[:, 0]]
    if k == 2:
        M = D2.copy(); M[rows, idx[:, 0]] = np.inf
        idx[:, 1] = np.argmin(M, axis=1); d2[:, 1] = D2[rows, idx[:, 1]]
    return idx, d2


def dist32(d2):
    return np.sqrt(np.asarray(d2).astype(np.float32))


class Pair:
    """Everything the four rules need of one (query, train) pair, computed once."""

    def __init__(self, q, t):
        self.nq, self.nt = len(q), len(t)
        self.D2 = d2_matrix(q, t)
        self.fidx, self.fd2 = two_nearest(self.D2)
        self.ridx, self.rd2 = two_nearest(self.D2.T)

    def knn2(self):
        """(idx [nq, k], float32 dist [nq, k]), k = min(2, nt): knnMatch(k=2)."""
        return self.fidx, dist32(self.fd2)

    def select(self, mode, ratio=RATIO):
        """(query, train, float32 distance) of the matches, ascending query: k_match_select's rule `mode` (a name of MODES)."""
        nq, nt = self.nq, self.nt
        if nq == 0 or nt == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
        f0 = self.fidx[:, 0]; fd = dist32(self.fd2[:, 0])
        if mode == "nearest":                              # BFMatcher(crossCheck=False).match
            keep = np.ones(nq, bool); ti = f0; d = fd
        elif mode == "mutual":                             # cv2 4.x crossCheck=True: the train row's own nearest query must be q
            keep = self.ridx[f0, 0] == np.arange(nq); ti = f0; d = fd
        elif mode == "legacy":
            # per query the minimum of (dist, train) over the train rows whose reverse nearest neighbour it is
            r0 = self.ridx[:, 0]; rd = dist32(self.rd2[:, 0])
            ti = np.full(nq, -1, np.int64); d = np.full(nq, np.inf, np.float32)
            for t in range(nt):                            # ascending train, strict <: the earliest of equals stays
                q = r0[t]
                if rd[t] < d[q]:
                    d[q] = rd[t]; ti[q] = t
            keep = ti >= 0
        elif mode == "ratio":                              # knnMatch(k=2) + `m.distance < ratio * n.distance` on the float distances
            if nt < 2:
                keep = np.zeros(nq, bool)
            else:
                keep = fd.astype(np.float64) < float(ratio) * dist32(self.fd2[:, 1]).astype(np.float64)
            ti = f0; d = fd
        else:
            raise ValueError(mode)
        return np.nonzero(keep)[0], ti[keep], d[keep].astype(np.float32)


# ------------------------------------------------------------------ seeded row generators, all uint8 [n][128]
def _sift_normalise(x):
    """calcSIFTDescriptor's tail on non-negative rows: clip at 0.2 of the norm, scale to norm 512, round, saturate."""
    x = np.asarray(x, np.float64)
    n = np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    x = np.minimum(x, 0.2 * n)
    n = np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return np.clip(np.rint(x * (512.0 / n)), 0, 255).astype(np.uint8)


def sift_like(rng, n):
    return _sift_normalise(rng.gamma(0.5, 1.0, (n, 128)))


def perturbed(rng, rows, sigma=6.0):
    """SIFT-like rows near `rows`: the nearest neighbour of a copy is, as a rule, the row it was copied from."""
    return _sift_normalise(np.abs(rows.astype(np.float64) + rng.normal(0, sigma, rows.shape)))


def with_duplicates(rng, rows, fraction=0.1):
    rows = rows.copy()
    n = len(rows)
    k = int(n * fraction)
    if n >= 2 and k > 0:
        dst = rng.choice(n, k, replace=False)
        rows[dst] = rows[rng.integers(0, n, k)]
    return rows


def tie_rows(rng, base, n, first_two):
    """n rows drawn with repetition from the 12 rows of `base`.  first_two: {base row: (i, j)}: that row's first two occurrences
    are forced to columns i < j (it appears nowhere else below j), so that the first and second neighbour of a query equal to
    it are tied at columns the caller chose."""
    src = rng.integers(0, len(base), n)
    fill = [b for b in range(len(base)) if b not in first_two]
    for b, (i, j) in first_two.items():
        for c in range(min(j, n)):
            if src[c] == b:
                src[c] = fill[c % len(fill)]
    for b, (i, j) in first_two.items():
        if j < n:
            src[i] = b; src[j] = b
    return base[src], src


# A ratio <= 1 drops every query whose first neighbour ties with another column, so it never shows WHICH of the equal columns the
# knn2 form put first.  At this ratio the queries tied at a distance > 0 are kept and the index must be the lowest.
TIE_RATIO_ABOVE_ONE = 1.5

# columns of the tied first and second neighbour, by query (= base row): one 16-group / different lanes; two groups of one
# 128-row stage / different lanes; two stages; one lane (column % 16) in two groups
TIE_COLUMNS = {0: (3, 9), 1: (20, 40), 2: (100, 200), 3: (21, 37)}


def bound_rows():
    """Rows at the edge of the range argument in k_nn_l2i8's header: |row|^2 <= 2^20, d^2 <= 2^21."""
    rows = []
    rows.append(np.zeros(128, np.uint8))                                   # int8 image: -128 everywhere, norms[] = 2^21, the largest there is
    for sup in (np.arange(0, 64), np.arange(64, 128),                       # 64 elements of 128: |row|^2 = 2^20 exactly; disjoint supports ...
                np.arange(32, 96), np.arange(0, 128, 2), np.arange(1, 128, 2),     # ... and overlapping ones
                np.r_[0:32, 96:128]):
        r = np.zeros(128, np.uint8); r[sup] = 128; rows.append(r)
    for s in (0, 16, 56, 112):                                             # 16 elements of 255: |row|^2 = 1040400 < 2^20
        r = np.zeros(128, np.uint8); r[s:s + 16] = 255; rows.append(r)
    r = np.zeros(128, np.uint8); r[np.arange(0, 128, 8)] = 255; rows.append(r)
    for s in (0, 1, 63, 127):                                              # one-hot 255
        r = np.zeros(128, np.uint8); r[s] = 255; rows.append(r)
    rows.append(np.zeros(128, np.uint8))                                   # a second zero row: distance 0 twice
    return np.stack(rows)


def flagged_row():
    """|row|^2 = 2^20 + 1: one past the bound."""
    r = np.zeros(128, np.uint8); r[:64] = 128; r[64] = 1
    return r


class Group:
    """Row sets that share one FrontEnd (one kp_cap), and the pairs run on them in one launch."""

    def __init__(self, name, kp_cap, sets, pairs, ratio=RATIO):
        self.name, self.kp_cap, self.sets, self.pairs, self.ratio = name, kp_cap, sets, pairs, ratio
        self._ref = {}

    def ref(self, a, b):
        if (a, b) not in self._ref:
            self._ref[(a, b)] = Pair(self.sets[a], self.sets[b])
        return self._ref[(a, b)]


REMAINDER_COUNTS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)


def _remainders():
    # the 16-column group, the 64 rows of a wave, the 128-row stage, the 512-row workgroup; kp_cap 1280 = 3 workgroups per pair
    rng = np.random.default_rng(8101)
    pool = sift_like(rng, max(REMAINDER_COUNTS))
    sets = {}
    for n in REMAINDER_COUNTS:
        sets[n] = perturbed(rng, pool[:n])[rng.permutation(n)]
    pairs = [(1, 1025), (1025, 1), (2, 513), (513, 2), (15, 16), (16, 15), (16, 17), (17, 63), (63, 64), (64, 65), (65, 64), (65, 127),
             (127, 128), (128, 129), (129, 128), (129, 511), (511, 512), (512, 513), (513, 512), (513, 1025), (1025, 511), (1025, 1025),
             (2, 1), (17, 129)]
    return Group("remainders", 1280, sets, pairs)


def _edge4096():
    # nb <= 4096 takes the packed key (group 255 is the last that fits), above it value and group travel apart
    rng = np.random.default_rng(8102)
    a = sift_like(rng, 64)
    b = perturbed(rng, a[rng.integers(0, 64, 4097)], sigma=12.0)
    b[5] = a[7]; b[4090] = a[7]          # one row twice, lanes 5 and 10, groups 0 and 255: the lower index wins
    b[21] = a[11]; b[4085] = a[11]       # one row twice in ONE lane (column % 16 == 5), groups 1 and 255: the packed key's 255 - group decides
    b[4087] = a[3]                       # the only exact copy of a[3]: a winner in group 255
    b[4096] = a[9]                       # (4097 rows only) the only exact copy of a[9]: a winner in group 256, which no packed key can hold
    c = perturbed(rng, b[:4096][rng.permutation(4096)], sigma=12.0)
    c[4095] = b[4094]                    # (4096, 4096): winners in group 255 in both directions
    d = perturbed(rng, b[rng.integers(0, 4097, 4100)], sigma=12.0)
    d[4099] = b[4096]                    # (4097, 4100): unpacked both ways, winners in group 256 both ways
    sets = {"a64": a, "b4095": b[:4095].copy(), "b4096": b[:4096].copy(), "b4097": b, "c4096": c, "d4100": d}
    pairs = [("a64", "b4095"), ("a64", "b4096"), ("a64", "b4097"), ("c4096", "b4096"), ("b4097", "d4100")]
    return Group("edge4096", 4352, sets, pairs)


def _ties():
    rng = np.random.default_rng(8103)
    base = sift_like(rng, 12)
    t280, _ = tie_rows(rng, base, 280, TIE_COLUMNS)
    t900, _ = tie_rows(rng, base, 900, TIE_COLUMNS)
    q300 = base[np.r_[0:12, rng.integers(0, 12, 288)]].copy()
    far = rng.random(300) < 0.25         # a quarter of the queries lie NEAR a base row: ties at a distance > 0
    far[:12] = False
    q300[far] = perturbed(rng, q300[far], sigma=3.0)
    q17 = base[np.r_[0:12, rng.integers(0, 12, 5)]].copy()
    sets = {"q300": q300, "t280": t280, "q17": q17, "t900": t900}
    return Group("ties", 1024, sets, [("q300", "t280"), ("q17", "t900"), ("t280", "q300")], ratio=1.0)


def _bound():
    rng = np.random.default_rng(8104)
    b = bound_rows()
    sets = {"bound": b, "bound_r": b[::-1].copy(), "sift": sift_like(rng, 100)}
    pairs = [("bound", "bound"), ("bound", "bound_r"), ("bound", "sift"), ("sift", "bound")]
    return Group("bound", 256, sets, pairs)


def _one_train():
    rng = np.random.default_rng(8105)
    q = sift_like(rng, 40)
    sets = {"q40": q, "t1": perturbed(rng, q[13:14]), "q1": perturbed(rng, q[29:30])}
    return Group("one_train", 256, sets, [("q40", "t1"), ("q1", "q40"), ("t1", "q1"), ("t1", "t1")])


FUZZ_SEEDS = (0, 1, 2, 3, 4, 5)


def _fuzz(seed):
    rng = np.random.default_rng(8200 + seed)
    counts = [int(v) for v in rng.integers(1, 701, 4)]
    pool = sift_like(rng, 700)
    sets = {i: with_duplicates(rng, perturbed(rng, pool[:n])[rng.permutation(n)]) for i, n in enumerate(counts)}
    return Group(f"fuzz{seed}", 768, sets, [(0, 1), (1, 2), (2, 3), (3, 0)])


@functools.lru_cache(maxsize=None)
def group(name):
    """The case groups of tests/test_gpu_match_l2i8.py, built once per process; their references are cached in them."""
    if name.startswith("fuzz"):
        return _fuzz(int(name[4:]))
    return {"remainders": _remainders, "edge4096": _edge4096, "ties": _ties, "bound": _bound, "one_train": _one_train}[name]()


GROUPS = ("remainders", "edge4096", "ties", "bound", "one_train") + tuple(f"fuzz{s}" for s in FUZZ_SEEDS)


@functools.lru_cache(maxsize=None)
def stale_case():
    """A slot that held 300 rows and then holds 17: rows 17..31 of the earlier frame are exact copies of queries 0..14, so any of
    them, if it were read, would win at distance 0."""
    rng = np.random.default_rng(8106)
    q = sift_like(rng, 40)
    t300 = perturbed(rng, q[rng.integers(15, 40, 300)], sigma=12.0)      # (nothing near queries 0..14 but the copies)
    t300[17:32] = q[:15]
    t17 = t300[:17].copy()
    return dict(q=q, t300=t300, t17=t17)

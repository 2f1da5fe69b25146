"""Place recognition (vo_vocab_*, vo_places_*; FrontEnd.train_vocabulary .. places_query) restated with numpy and the CPU oracle, and
the chosen cases the device is held to (not a test module).

The rules (include/vo_hip.h, "place recognition"), all of them integers:
  quantiser  a row's word is its nearest word — Hamming distance for 32-byte ORB rows, the integer squared L2 distance for 128-byte
             SIFT rows — the lowest word index winning a tie: oracle.match_hamming / oracle.match_l2 with cross_check = 0 (cv2's
             plain nearest neighbour: ascending scan, strict `<`; for SIFT rows cv2 orders by sqrtf((float)d^2), which is the order
             of d^2 below 2^22, and every row here keeps |row|^2 <= 2^20);
  training   word w starts as training row floor(w n / K); a round = assign every row, then per word with c > 0 rows: ORB bit b = 1
             iff 2 ones_b > c, SIFT component j = (2 sum_j + c) // (2 c); c = 0 keeps the row; at most `iterations` rounds, and from
             the second round on a round whose assignment moved no row ends before its update; iterations_run = updates done;
  entry      hist[w] = min(255, rows whose word is w), sum = hist.sum();
  query      shared(q, d) = sum_w min(hist_q[w], hist_d[w]); d != q, |id_q - id_d| >= min_gap, shared >= min_shared; the top_k of
             largest shared, lower entry first among equals; unused places entry -1, shared 0.
tests/test_places_reference.py holds every function here equal to a loop-by-loop restatement on every case below.

CHUNK: the words one LDS stage of the quantiser's kernels holds — 128 SIFT rows, 256 ORB rows (tests/relocalize_reference.py)."""
import numpy as np

from oracle import oracle as O
from relocalize_reference import CHUNK, nudge, rand_rows

VO_OK, VO_ERR_INVALID, VO_ERR_TOO_FEW, VO_ERR_NOT_CONFIGURED, VO_ERR_UNSUPPORTED = 0, -1, -3, -5, -7   # include/vo_hip.h
FRAME_SIZES = (0, 1, 17, 300)
INDEX_SIZES = (1, 2, 17, 64, 65, 257)
TOP_KS = (1, 3, 16)


def width(detector):
    return 128 if detector == "sift" else 32


# ------------------------------------------------------------------ the reference
def quantise(rows, words):
    """[n] int32: the word of every row."""
    r = np.ascontiguousarray(rows, np.uint8); w = np.ascontiguousarray(words, np.uint8)
    if len(r) == 0:
        return np.zeros(0, np.int32)
    if r.shape[1] == 128:
        qi, ti, _ = O.match_l2(r.astype(np.float32), w.astype(np.float32), 0)
    else:
        qi, ti, _ = O.match_hamming(r, w, 0)
    assert np.array_equal(qi, np.arange(len(r)))
    return ti.astype(np.int32)


def update(rows, word, words):
    """The words after one update from the assignment `word`."""
    out = words.copy()
    for w in np.unique(word):
        mine = rows[word == w]
        c = len(mine)
        if rows.shape[1] == 32:
            ones = np.unpackbits(mine, axis=1, bitorder="little").astype(np.int64).sum(axis=0)
            out[w] = np.packbits((2 * ones > c).astype(np.uint8), bitorder="little")
        else:
            out[w] = ((2 * mine.astype(np.int64).sum(axis=0) + c) // (2 * c)).astype(np.uint8)
    return out


def train(frames, K, iterations=8, quantiser=quantise, updater=update):
    """(words [K, D] uint8, iterations_run) from the rows of `frames`, a list of [n_f, D] arrays in slot-list order."""
    rows = np.concatenate([np.ascontiguousarray(f, np.uint8) for f in frames])
    n = len(rows)
    assert n >= K
    words = rows[[(w * n) // K for w in range(K)]].copy()
    prev, run = None, 0
    for r in range(max(int(iterations), 1)):
        word = quantiser(rows, words)
        if r > 0 and np.array_equal(word, prev):
            break
        words = updater(rows, word, words)
        prev, run = word, run + 1
    return words, run


def histogram(word, K):
    """(hist [K] uint8, sum) of a frame whose rows have the words `word`."""
    h = np.minimum(np.bincount(np.asarray(word, np.int64), minlength=K), 255).astype(np.uint8)
    return h, int(h.astype(np.int64).sum())


def entries(frames, words):
    """(hist [F, K] uint8, sum [F] int32) of the frames' entries."""
    K = len(words)
    hs = [histogram(quantise(f, words), K) for f in frames]
    return (np.stack([h for h, _ in hs]) if hs else np.zeros((0, K), np.uint8)), np.array([s for _, s in hs], np.int32)


def shared_row(hist, q):
    """[n] int64: shared(q, d) for every entry d."""
    h = np.asarray(hist).astype(np.int64)
    return np.minimum(h, h[q]).sum(axis=1)


def query(hist, ids, queries=None, top_k=3, min_gap=0, min_shared=0):
    """(entry [Q, top_k] int32, shared [Q, top_k] int32)."""
    n = len(hist)
    queries = range(n) if queries is None else [int(q) for q in queries]
    ent = np.full((len(queries), top_k), -1, np.int32); sh = np.zeros((len(queries), top_k), np.int32)
    for row, q in enumerate(queries):
        s = shared_row(hist, q)
        cand = [(-int(s[d]), d) for d in range(n)
                if d != q and abs(int(ids[q]) - int(ids[d])) >= min_gap and s[d] >= min_shared]
        for k, (neg, d) in enumerate(sorted(cand)[:top_k]):
            ent[row, k], sh[row, k] = d, -neg
    return ent, sh


# ------------------------------------------------------------------ quantiser cases
EQUIDISTANT = (7, 9)           # two words one step either side of a row the frames carry: the lower index must win


def vocabulary_case(detector, K):
    """K words with duplicates where the kernels fold — a lane apart (2, 3), a 16-column group apart (5, 21), a staged chunk apart
    (0, CHUNK), (40, 40 + CHUNK) where K allows — and the pair EQUIDISTANT: word 9 = word 7 moved by two steps in one place."""
    rng = np.random.default_rng(31000 + K + (0 if detector == "orb" else 500000))
    w = rand_rows(rng, K, detector)
    C = CHUNK[detector]
    for a, b in ((2, 3), (5, 21), (0, C), (40, 40 + C)):
        if b < K:
            w[b] = w[a]
    a, b = EQUIDISTANT
    w[b] = w[a]
    if detector == "orb":
        w[b, 0] ^= 3
    else:
        w[b, 0] = w[a, 0] + 2
    return w


def equidistant_row(detector, words):
    r = words[EQUIDISTANT[0]].copy()
    if detector == "orb":
        r[0] ^= 1
    else:
        r[0] += 1
    return r


def frame_case(detector, words, n, seed=0):
    """A frame of n rows: every other row a nudged copy of a word (of the duplicated ones first, so that their ties are met), the
    rest random; row 1 is the equidistant row."""
    K = len(words)
    rng = np.random.default_rng(32000 + 1000 * seed + 7 * K + n + (0 if detector == "orb" else 500000))
    f = rand_rows(rng, n, detector)
    C = CHUNK[detector]
    dup = [a for a, b in ((2, 3), (5, 21), (0, C), (40, 40 + C)) if b < K]
    for k, i in enumerate(range(0, n, 2)):
        src = dup[k] if k < len(dup) else int(rng.integers(0, K))
        f[i] = words[src] if k < len(dup) else nudge(words[src], int(rng.integers(0, 3)), detector)
    if n > 1:
        f[1] = equidistant_row(detector, words)
    return f


# ------------------------------------------------------------------ training cases
def planted_case(detector, K=256):
    """K distinct centres, each observed three times: observation 0 and 1 each disturb a few places of their own (ORB: flipped bits,
    no bit in both; SIFT: +1 and -1 on the same elements, so that the sum is three times the centre), observation 2 is clean.  The
    observations of a centre are consecutive, so the start words are observation 0 of every centre.  Returns (frames — three of K
    rows each —, centres)."""
    rng = np.random.default_rng(33000 + K + (0 if detector == "orb" else 500000))
    if detector == "orb":
        c = rand_rows(rng, K, detector)
    else:
        c = rng.integers(1, 90, (K, 128), dtype=np.uint8)
    assert len(np.unique(c, axis=0)) == K
    rows = np.repeat(c, 3, axis=0)
    for w in range(K):
        if detector == "orb":
            bits = rng.choice(256, 10, replace=False)
            for o, mine in enumerate((bits[:5], bits[5:])):
                for b in mine:
                    rows[3 * w + o, b // 8] ^= np.uint8(1 << (b % 8))
        else:
            at = rng.choice(128, 6, replace=False)
            rows[3 * w, at] += 1
            rows[3 * w + 1, at] -= 1
    return [rows[:K], rows[K:2 * K], rows[2 * K:]], c


def training_case(detector, name):
    """dict(frames, K, iterations) of a named case:
      exact        n = K: every row starts a word; rows 4 and 5 are equal, so word 5 never gets a row and keeps its own
      plus_one     n = K + 1: the start words are rows 0 .. K - 1; row K is row 10 changed in a few places, so word 10 gets two rows:
                   ORB bits on which they differ are majority ties (0), SIFT components whose sum is odd end in .5 (rounded up)
      three_slots  slots of 300, 17 and 120 crowded rows, two rounds: the assignments are still moving then
      planted      planted_case: stops after one update"""
    rng = np.random.default_rng(34000 + (0 if detector == "orb" else 500000))
    K = 256
    if name == "exact":
        rows = rand_rows(rng, K, detector)
        rows[5] = rows[4]
        return dict(frames=[rows], K=K, iterations=8)
    if name == "plus_one":
        rows = rand_rows(rng, K + 1, detector)
        if detector == "orb":
            rows[10, 0] = 0xF0; rows[K] = rows[10]; rows[K, 0] = 0x3C          # differ in bits 2, 3, 6, 7; both 1 in bits 4, 5
        else:
            rows[10, :2] = (40, 40); rows[K] = rows[10]; rows[K, :2] = (41, 39)   # means 40.5 -> 41 and 39.5 -> 40
        return dict(frames=[rows], K=K, iterations=8)
    if name == "three_slots":
        # ORB: rows scattered around 40 centres; SIFT: one row varied in two components.  Several words to a neighbourhood: the words
        # go on trading rows for a few rounds
        base = rand_rows(rng, 40, detector)
        rows = base[rng.integers(0, 40, 437)]
        if detector == "orb":
            rows = rows ^ np.packbits(rng.random((437, 256)) < 0.08, axis=1)
        else:
            rows = np.repeat(base[:1], 437, axis=0)           # in 128 dimensions nothing moves after one round: vary two
            rows[:, :2] = rng.integers(0, 91, (437, 2))
        return dict(frames=[rows[:300], rows[300:317], rows[317:]], K=K, iterations=2)
    if name == "planted":
        return dict(frames=planted_case(detector, K)[0], K=K, iterations=8)
    raise KeyError(name)


TRAINING_CASES = ("exact", "plus_one", "three_slots", "planted")


# ------------------------------------------------------------------ scorer cases
def histogram_case(n, K=256, seed=0):
    """n chosen histograms [n, K] uint8: mostly 0 .. 3 with some 255; entries 9 and 70 repeat entry 5 (equal shared with every
    query, in one block of 64 entries and in two), entry 3 repeats entry 1; entries 4, 12 and 13 repeat entry 8 and entries 15 and 16
    repeat entry 20: the best candidates of queries 8 and 20 lie 4 and 5 ids away on either side, around min_gap = 5."""
    rng = np.random.default_rng(35000 + 100 * seed + n + K)
    h = rng.integers(0, 4, (n, K)).astype(np.uint8)
    h[rng.random((n, K)) < 0.5] = 0
    h[rng.random((n, K)) < 0.01] = 255
    for a, b in ((5, 9), (5, 70), (1, 3), (8, 4), (8, 12), (8, 13), (20, 15), (20, 16)):
        if max(a, b) < n:
            h[b] = h[a]
    return h


def extreme_ids(n):
    """ids at both ends of int32: differences that do not fit 32 bits"""
    ids = np.arange(n, dtype=np.int64) * 3
    ids[::2] = -(1 << 31) + ids[::2]
    ids[1::2] = (1 << 31) - 1 - ids[1::2]
    return ids.astype(np.int32)


def scorer_queries(hist):
    """The query calls every index of the scorer tests is asked: a list of dict(ids, queries (None: all), top_k, min_gap, min_shared).
    ids are 0 .. n - 1 unless the call is about ids; min_shared of the last but one call is query 0's best shared, so that an entry
    lies exactly on the bound."""
    n = len(hist)
    ids = np.arange(n, dtype=np.int32)
    calls = [dict(ids=ids, queries=None, top_k=k, min_gap=0, min_shared=0) for k in TOP_KS]
    calls.append(dict(ids=ids, queries=None, top_k=16, min_gap=5, min_shared=0))            # entries q - 5 and q + 5 are on the bound
    calls.append(dict(ids=extreme_ids(n), queries=None, top_k=3, min_gap=(1 << 31) - 1, min_shared=0))
    best = int(np.delete(shared_row(hist, 0), 0).max(initial=0))
    calls.append(dict(ids=ids, queries=None, top_k=3, min_gap=0, min_shared=best))
    calls.append(dict(ids=ids, queries=[n - 1, 0, n - 1], top_k=3, min_gap=0, min_shared=0))
    calls.append(dict(ids=ids, queries=[n // 2], top_k=1, min_gap=0, min_shared=0))
    return calls

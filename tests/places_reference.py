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
tests/test_places_reference.py holds every function here equal to a loop-by-loop restatement on every case below (on a stated part
of the largest ones).  The cases of tests/test_gpu_places.py come first in every section; the "wide" cases of
tests/test_gpu_places_shapes.py — more than one tile of entries a workgroup, more than one quantiser workgroup a slot, a second pass
of the accumulate grid, 1024 and 4096 words — follow them, with split_plan(), the host's dealing rule restated.

CHUNK: the words one LDS stage of the quantiser's kernels holds — 128 SIFT rows, 256 ORB rows (tests/relocalize_reference.py)."""
import numpy as np

from oracle import oracle as O
from relocalize_reference import CHUNK, nudge, rand_rows

VO_OK, VO_ERR_INVALID, VO_ERR_TOO_FEW, VO_ERR_NOT_CONFIGURED, VO_ERR_UNSUPPORTED = 0, -1, -3, -5, -7   # include/vo_hip.h
FRAME_SIZES = (0, 1, 17, 300)
INDEX_SIZES = (1, 2, 17, 64, 65, 257)
TOP_KS = (1, 3, 16)
BLOCK_ROWS = 512               # NM_BLOCK_ROWS = NO_BLOCK_ROWS (reloc_kernels.hip): the rows of a slot one workgroup of the quantiser takes


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


def query_vec(hist, ids, queries=None, top_k=3, min_gap=0, min_shared=0):
    """query() without the loop over candidates, for indexes of thousands of entries: the same rules as array operations, the
    order by a stable sort on (-shared, entry).  tests/test_places_reference.py holds it equal to query() on every scorer case."""
    h = np.ascontiguousarray(hist, np.uint8)
    n = len(h)
    wide = np.asarray(ids).astype(np.int64)
    queries = range(n) if queries is None else [int(q) for q in queries]
    ent = np.full((len(queries), top_k), -1, np.int32); sh = np.zeros((len(queries), top_k), np.int32)
    every = np.arange(n)
    for row, q in enumerate(queries):
        s = np.minimum(h, h[q]).sum(axis=1, dtype=np.int64)
        cand = np.flatnonzero((every != q) & (np.abs(wide - wide[q]) >= min_gap) & (s >= min_shared))
        best = cand[np.lexsort((cand, -s[cand]))[:top_k]]
        ent[row, :len(best)], sh[row, :len(best)] = best, s[best]
    return ent, sh


def query_list(hist, ids, queries, top_k=3, min_gap=0, min_shared=0):
    """query_vec() for a list that names entries many times: asked once over the distinct entries, then indexed by the list."""
    queries = np.asarray(queries, np.int64)
    distinct = np.unique(queries)
    ent, sh = query_vec(hist, ids, distinct, top_k, min_gap, min_shared)
    at = np.searchsorted(distinct, queries)
    return ent[at], sh[at]


MAX_SPLITS = 64                # VO_PLACES_MAX_SPLITS (visual_odometry_amd/csrc/vo_internal.h)


def split_plan(n, Q):
    """(splits, per_split, tiles_per_split, used_splits, empty_splits): how vo_places_query deals an index of n entries over the
    workgroups of Q query entries.  Restated from visual_odometry_amd/csrc/places_api.hip, vo_places_query, the three lines under
    "the entries are dealt over `splits` workgroups per block of 64 queries":
        qblocks = (Q + 63) / 64, tiles = (P.n + 63) / 64
        splits = max(1, min(min(VO_PLACES_MAX_SPLITS, tiles), (1024 + qblocks - 1) / qblocks))
        per_split = (tiles + splits - 1) / splits * 64
    Workgroup (query block, sp) of k_places_score walks the entries [sp per_split, min(n, (sp + 1) per_split)), 64 at a time; a split
    that starts at or past n walks nothing and leaves sixteen zero keys."""
    qblocks, tiles = (Q + 63) // 64, (n + 63) // 64
    splits = max(1, min(MAX_SPLITS, tiles, (1024 + qblocks - 1) // qblocks))
    per_split = (tiles + splits - 1) // splits * 64
    used = min(splits, (n + per_split - 1) // per_split)
    return splits, per_split, per_split // 64, used, splits - used


# ------------------------------------------------------------------ quantiser cases
EQUIDISTANT = (7, 9)           # two words one step either side of a row the frames carry: the lower index must win
FIRST_AGAINST_LAST = 1         # from K = 1024 on word K - 1 repeats this word: a tie between the first chunk and the last


def vocabulary_case(detector, K):
    """K words with duplicates where the kernels fold — a lane apart (2, 3), a 16-column group apart (5, 21), a staged chunk apart
    (0, CHUNK), (40, 40 + CHUNK) where K allows — and the pair EQUIDISTANT: word 9 = word 7 moved by two steps in one place.
    From K = 1024 on (8 to 32 staged chunks) word K - 1 repeats word 1 as well."""
    rng = np.random.default_rng(31000 + K + (0 if detector == "orb" else 500000))
    w = rand_rows(rng, K, detector)
    C = CHUNK[detector]
    for a, b in ((2, 3), (5, 21), (0, C), (40, 40 + C)):
        if b < K:
            w[b] = w[a]
    if K >= 1024:
        w[K - 1] = w[FIRST_AGAINST_LAST]
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
    rest random; row 1 is the equidistant row.  A frame of more than 512 rows meets the same ties again from row 512 on, and one
    of more than 1024 rows from row 1024 on (BLOCK_ROWS: the rows one workgroup of the quantiser takes), as far as it has rows."""
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
    for base in range(BLOCK_ROWS, n, BLOCK_ROWS):
        for k, src in enumerate(dup):
            if base + 2 * k < n:
                f[base + 2 * k] = words[src]
        if base + 1 < n:
            f[base + 1] = equidistant_row(detector, words)
    return f


def tail_frame(words):
    """Rows that copy the last four words, K - 4 .. K - 1, some of them twice: the last dword of the histogram.  From K = 1024 on
    word K - 1 repeats word FIRST_AGAINST_LAST, so its copies count for that word."""
    K = len(words)
    return words[[K - 4, K - 1, K - 3, K - 2, K - 1, K - 2, K - 2]].copy()


def histogram_frames(detector, words):
    """The frames of the histogram tests: 300 identical rows (saturation), none, an ordinary frame, the last four words."""
    return [np.repeat(words[11:12], 300, axis=0), np.zeros((0, width(detector)), np.uint8), frame_case(detector, words, 300), tail_frame(words)]


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


# ------------------------------------------------------------------ scorer cases past one tile, one split and 512 words
# name: (n, Q) and the plan split_plan(n, Q) must give — (splits, per_split, tiles_per_split, used_splits, empty_splits):
#   two_tiles         splits 0 and 1 walk two tiles each, split 2 holds entry 256 alone, split 3 starts past n
#   one_workgroup     five tiles through one list, the last tile one entry
#   one_workgroup_65  a full tile, then one entry
#   full_merge        every split leaves 16 keys: k_places_merge holds 1024
#   past_the_merge    33 splits in use, the last of one entry; 31 start past n
WIDE_CASES = {"two_tiles": (257, 19200), "one_workgroup": (257, 65536), "one_workgroup_65": (65, 65536), "full_merge": (4096, 70),
              "past_the_merge": (4097, 71)}
WIDE_PLANS = {"two_tiles": (4, 128, 2, 3, 1), "one_workgroup": (1, 320, 5, 1, 0), "one_workgroup_65": (1, 128, 2, 1, 0),
              "full_merge": (64, 64, 1, 64, 0), "past_the_merge": (64, 128, 2, 33, 31)}
COPIES_OF_5 = (9, 70, 130, 200, 256, 4095, 4096)          # where n allows: one tile, two tiles of a split, two splits, the last short tile
LAST_QUERY, FIRST_QUERY = 30, 32
FIRST16 = tuple(range(33, 49))                             # the sixteen best of FIRST_QUERY: all in the first tile
LAST16_AT = {65: 49, 257: 240, 4096: 4079, 4097: 4079}     # the sixteen best of LAST_QUERY start here, see histogram_case_wide


def last16(n):
    return tuple(range(LAST16_AT[n], LAST16_AT[n] + 16))


def histogram_case_wide(n, K=256):
    """histogram_case(n, K) — its seeded entries and copies stay — with
      * exact copies of entry 5 at COPIES_OF_5 as far as n allows: equal scores in one tile (9), in two tiles of one split, in two
        splits and in a last tile of one entry (256 of 257, 4096 of 4097); the lower entry must come first;
      * the sixteen best candidates of entry LAST_QUERY at last16(n), their scores ASCENDING with the entry (entry last16[i] is
        LAST_QUERY's histogram with 16 - i of its words one lower: shared = sum - (16 - i)): each of them passes every key the list
        holds, lands at position 0 and shifts a full list.  They end at the end of a 64-entry tile that is the last one a
        workgroup walks wherever the plan has such a tile of 16 entries (257: tile 3, the last of split 1 of `two_tiles` and the
        fourth of five in `one_workgroup`, whose last tile is entry 256 alone; 4096, 4097: the last tile of the last full split);
        with n = 65 they are entries 49 .. 64: the best of all is the one entry of the last tile;
      * the sixteen best candidates of entry FIRST_QUERY at FIRST16, in the first tile, scores in a seeded order: every candidate
        of a later tile is turned away at `key <= worst`."""
    h = histogram_case(n, K)
    rng = np.random.default_rng(36000 + n + K)
    for b in COPIES_OF_5:
        if b < n:
            h[b] = h[5]

    def lower(q, steps):
        r = h[q].copy()
        r[rng.choice(np.flatnonzero(r), steps, replace=False)] -= 1
        return r

    for i, e in enumerate(last16(n)):
        h[e] = lower(LAST_QUERY, 16 - i)
    for e, p in zip(FIRST16, rng.permutation(16)):
        h[e] = lower(FIRST_QUERY, int(p) + 1)
    return h


def wide_queries(name):
    """The query list of a wide case.  257 and 65 entries: every entry, repeated to Q places in a seeded shuffle.  4096 and 4097
    entries: 70 chosen entries (two blocks of queries) — the entries with copies and their copies, LAST_QUERY, FIRST_QUERY, both
    ends of tiles and of the index, seeded others — and for 4097 entry 4096 after them."""
    n, Q = WIDE_CASES[name]
    if n <= 257:
        q = np.resize(np.arange(n, dtype=np.int32), Q)
        np.random.default_rng(37000 + n + Q).shuffle(q)
        return q
    rng = np.random.default_rng(37000)
    fixed = [0, 1, 3, 5, 8, 9, 20, LAST_QUERY, FIRST_QUERY, 33, 48, 63, 64, 70, 130, 200, 256, 4032, 4079, 4094, 4095]
    rest = [int(e) for e in rng.permutation(4096) if e not in fixed][:70 - len(fixed)]
    q = np.array(fixed + rest, np.int32)
    rng.shuffle(q)
    return q if n == 4096 else np.append(q, np.int32(4096))


def wide_calls(hist):
    """The calls every wide case is asked, as dict(ids, top_k, min_gap, min_shared): top_k 1, 3, 16; min_gap 5 on ids 0 .. n - 1;
    ids at both ends of int32; min_shared = the third best score query 0 reports (entry 0 is in every list), an entry on the bound."""
    n = len(hist)
    ids = np.arange(n, dtype=np.int32)
    calls = [dict(ids=ids, top_k=k, min_gap=0, min_shared=0) for k in TOP_KS]
    calls.append(dict(ids=ids, top_k=16, min_gap=5, min_shared=0))
    calls.append(dict(ids=extreme_ids(n), top_k=3, min_gap=(1 << 31) - 1, min_shared=0))
    calls.append(dict(ids=ids, top_k=16, min_gap=0, min_shared=int(query_vec(hist, ids, [0], top_k=3)[1][0, 2])))
    return calls


ALL_255, ALL_0 = 40, 41


def histogram_case_k(K):
    """65 histograms of K = 1024 or 4096 words: histogram_case(65, K) with entry ALL_255 all 255 (sum 255 K: 1 044 480 at K = 4096,
    the largest L1 the scorer's accumulators see, against ALL_0) and entry ALL_0 all 0."""
    h = histogram_case(65, K)
    h[ALL_255] = 255
    h[ALL_0] = 0
    return h


# ------------------------------------------------------------------ cases for a rig of three quantiser workgroups a slot
WIDE_KP_CAP = 1536                                         # 3 BLOCK_ROWS
WIDE_FRAMES = {"sift": 22, "orb": 172}                     # max_frames of the wide rigs
ACCUMULATE_ROWS = {"sift": 4, "orb": 32}                   # rows a workgroup of k_vocab_accumulate takes in one pass
ACCUMULATE_GRID = 8192                                     # its grid's cap (launch_vocab_accumulate): flat rows past GRID * ROWS are a second pass
WIDE_FRAME_SIZES = (513, 1024, 1025, 1536)


def crowded_rows(rng, n, detector, centres=40):
    """n rows that keep the words trading rows for a few rounds (training_case's `three_slots`): ORB rows scattered around a few
    centres, SIFT one row varied in two components."""
    base = rand_rows(rng, centres, detector)
    if detector == "orb":
        return base[rng.integers(0, centres, n)] ^ np.packbits(rng.random((n, 256)) < 0.08, axis=1)
    rows = np.repeat(base[:1], n, axis=0)
    rows[:, :2] = rng.integers(0, 91, (n, 2))
    return rows


def training_case_wide(detector, name):
    """dict(frames, slots, K, iterations) for the wide rigs; frames in slot-list order, slots the list:
      planted_1024  planted_case(detector, 1024): three slots of 1024 rows, stops after one update
      crowded_1024  slots of 1025, 17 and 513 crowded rows, K = 1024, two rounds, still moving then
      stride        every slot of the rig, in a seeded order: most hold 0 .. 3 rows, three hold 300, 600 and 450, the last of the
                    list 1025 — rows whose flat index q kp_cap + i is at or past ACCUMULATE_GRID * ACCUMULATE_ROWS; K = 256, two
                    rounds; the start rows of words 6 and 7 are equal, so word 7 gets no row in the first round and keeps its own"""
    sift = 0 if detector == "orb" else 500000
    if name == "planted_1024":
        return dict(frames=planted_case(detector, 1024)[0], slots=[5, 2, 9], K=1024, iterations=8)
    if name == "crowded_1024":
        rows = crowded_rows(np.random.default_rng(38000 + sift), 1555, detector)
        return dict(frames=[rows[:1025], rows[1025:1042], rows[1042:]], slots=[4, 1, 3], K=1024, iterations=2)
    if name == "stride":
        F = WIDE_FRAMES[detector]
        rng = np.random.default_rng(38500 + sift)
        counts = rng.integers(0, 4, F)
        counts[[2, F // 2, F - 3]] = (300, 600, 450)
        counts[F - 1] = 1025
        n = int(counts.sum())
        rows = crowded_rows(rng, n, detector)
        rows[(7 * n) // 256] = rows[(6 * n) // 256]
        at = np.concatenate([[0], np.cumsum(counts)])
        slots = [int(s) for s in rng.permutation(F)]
        assert slots != sorted(slots)
        return dict(frames=[rows[at[q]:at[q + 1]] for q in range(F)], slots=slots, K=256, iterations=2)
    raise KeyError(name)


WIDE_TRAINING_CASES = ("planted_1024", "crowded_1024", "stride")

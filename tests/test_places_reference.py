"""No GPU: tests/places_reference.py (numpy + the CPU oracle) against a second, loop-by-loop restatement written from the rules in
include/vo_hip.h ("place recognition") on every case tests/test_gpu_places.py and tests/test_gpu_places_shapes.py use, and every case
against what it is named for: planted centres come back exactly, an empty cluster keeps its word, ORB majority ties give 0, SIFT
means ending in .5 round up; for the wide cases, the plan table of vo_places_query's dealing rule, copies in ascending entry order,
the sixteen best of the "last tile" query in that tile, the rows past the accumulate grid's first pass, the saturated sums.  Where a
wide case is too large for the loops in a few seconds (4096 entries, 4096 words, thousands of training rows) they run over a stated
part of it: rows and words at a fixed step, chosen queries.
The scene test flies the example's course (examples/find_loops.py) at a small size and prints its margins."""
import importlib.util
import os

import numpy as np
import pytest

import places_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETECTORS = ("sift", "orb")


# ------------------------------------------------------------------ the restatement: plain loops, no oracle call
def distance(a, b):
    if len(a) == 32:
        return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))
    return sum((int(x) - int(y)) ** 2 for x, y in zip(a, b))


def quantise_loops(rows, words):
    out = []
    wide = words.astype(np.int64)
    for r in rows:
        if words.shape[1] == 32:
            d = np.unpackbits(words ^ r, axis=1).sum(axis=1)
        else:
            d = ((wide - r.astype(np.int64)) ** 2).sum(axis=1)
        best, at = None, -1
        for w in range(len(words)):
            if best is None or d[w] < best:
                best, at = d[w], w
        out.append(at)
    return np.array(out, np.int32)


def update_loops(rows, word, words, only=None):
    """`only`: the words to update (every word when None), for spot checks of large cases"""
    out = words.copy()
    D = rows.shape[1]
    for w in (range(len(words)) if only is None else only):
        mine = [rows[i] for i in range(len(rows)) if word[i] == w]
        c = len(mine)
        if c == 0:
            continue
        if D == 32:
            for b in range(256):
                ones = sum((int(r[b // 8]) >> (b % 8)) & 1 for r in mine)
                bit = 1 if 2 * ones > c else 0
                out[w, b // 8] = (int(out[w, b // 8]) & ~(1 << (b % 8))) | (bit << (b % 8))
        else:
            for j in range(128):
                out[w, j] = (2 * sum(int(r[j]) for r in mine) + c) // (2 * c)
    return out


def query_loops(hist, ids, queries, top_k, min_gap, min_shared):
    n = len(hist)
    queries = list(range(n)) if queries is None else list(queries)
    ent = np.full((len(queries), top_k), -1, np.int32); sh = np.zeros((len(queries), top_k), np.int32)
    h = hist.astype(np.int64)
    for row, q in enumerate(queries):
        best = []                                             # (shared, entry), kept in report order
        for d in range(n):
            if d == q or abs(int(ids[q]) - int(ids[d])) < min_gap:
                continue
            s = int(np.minimum(h[q], h[d]).sum())
            if s < min_shared:
                continue
            at = len(best)
            while at > 0 and best[at - 1][0] < s:             # a later entry passes only strictly smaller scores
                at -= 1
            best.insert(at, (s, d))
            del best[top_k:]
        for k, (s, d) in enumerate(best):
            ent[row, k], sh[row, k] = d, s
    return ent, sh


# ------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("det", DETECTORS)
@pytest.mark.parametrize("K", (256, 512))
def test_quantiser_cases(oracle, det, K):
    words = P.vocabulary_case(det, K)
    C = P.CHUNK[det]
    for n in P.FRAME_SIZES:
        f = P.frame_case(det, words, n)
        w = P.quantise(f, words)
        assert np.array_equal(w, quantise_loops(f, words)), (det, K, n)
        assert len(w) == n and w.dtype == np.int32
        if n >= 17:
            # rows equal to a duplicated word take the lower copy; the equidistant row takes the lower of its two words
            dup = [a for a, b in ((2, 3), (5, 21), (0, C), (40, 40 + C)) if b < K]
            assert [int(w[2 * k]) for k in range(len(dup)) if 2 * k != 1] == dup
            a, b = P.EQUIDISTANT
            r = P.equidistant_row(det, words)
            assert distance(r, words[a]) == distance(r, words[b]) == 1 and w[1] == a
    assert (C < K) == (det == "sift" or K == 512)             # the ORB chunk pair needs K = 512


# ------------------------------------------------------------------ training
@pytest.mark.parametrize("det", DETECTORS)
@pytest.mark.parametrize("name", P.TRAINING_CASES)
def test_training_cases(oracle, det, name):
    c = P.training_case(det, name)
    words, run = P.train(c["frames"], c["K"], c["iterations"])
    words2, run2 = P.train(c["frames"], c["K"], c["iterations"], quantiser=quantise_loops, updater=update_loops)
    assert run == run2 and np.array_equal(words, words2)
    rows = np.concatenate(c["frames"]); n, K = len(rows), c["K"]
    print(det, name, "n", n, "iterations_run", run)
    if name == "exact":
        assert n == K and run == 1
        expect = rows.copy()                                   # every word keeps its row: word 5 because no row reaches it
        assert np.array_equal(rows[4], rows[5]) and np.array_equal(words, expect)
        assert 5 not in P.quantise(rows, words).tolist()
    elif name == "plus_one":
        assert n == K + 1 and run == 1
        assert P.quantise(rows[K:], rows[:K])[0] == 10
        expect = rows[:K].copy()
        if det == "orb":
            expect[10] = rows[10] & rows[K]                     # two rows: a bit is kept only where both have it
            assert expect[10, 0] == 0x30 and not np.array_equal(expect[10], rows[10])
        else:
            expect[10, :2] = (41, 40)                          # 40.5 -> 41, 39.5 -> 40
        assert np.array_equal(words, expect)
    elif name == "three_slots":
        assert [len(f) for f in c["frames"]] == [300, 17, 120] and run == c["iterations"] == 2
        assert P.train(c["frames"], K, 3)[1] == 3               # still moving: a third round would have run
    elif name == "planted":
        centres = P.planted_case(det, K)[1]
        assert run == 1 < c["iterations"] and np.array_equal(words, centres)
        assert np.array_equal(P.quantise(rows, words), np.arange(n) // 3)


def test_rounding_and_ties_in_isolation():
    rows = np.zeros((4, 32), np.uint8); rows[0, 0] = 0b0111; rows[1, 0] = 0b0011; rows[2, 0] = 0b0001; rows[3, 0] = 0b1001
    out = P.update(rows, np.zeros(4, np.int32), np.zeros((1, 32), np.uint8))
    assert out[0, 0] == 0b0001                                  # ones 4, 2, 1, 1 of 4 rows: only bit 0 has a strict majority
    s = np.zeros((2, 128), np.uint8); s[0, :3] = (1, 2, 255); s[1, :3] = (2, 2, 254)
    out = P.update(s, np.zeros(2, np.int32), np.zeros((1, 128), np.uint8))
    assert out[0, :3].tolist() == [2, 2, 255]                   # 1.5 -> 2, 2 -> 2, 254.5 -> 255


# ------------------------------------------------------------------ histograms and scores
@pytest.mark.parametrize("det", DETECTORS)
def test_histograms(oracle, det):
    words = P.vocabulary_case(det, 256)
    frames = [np.repeat(words[11:12], 300, axis=0), np.zeros((0, P.width(det)), np.uint8), P.frame_case(det, words, 300), P.frame_case(det, words, 17)]
    hist, s = P.entries(frames, words)
    assert hist.dtype == np.uint8 and hist.shape == (4, 256)
    assert hist[0, 11] == 255 and s[0] == 255 and hist[0].astype(int).sum() == 255      # saturated: the sum is not the row count
    assert not hist[1].any() and s[1] == 0
    for f, h, t in zip(frames, hist, s):
        w = quantise_loops(f, words)
        assert [min(255, int((w == k).sum())) for k in range(256)] == h.tolist() and t == h.astype(int).sum()
    assert s[2] == 300 and s[3] == 17


@pytest.mark.parametrize("n", P.INDEX_SIZES)
def test_scorer_cases(n):
    hist = P.histogram_case(n)
    assert n < 2 or (hist == 0).any() and (n < 17 or (hist == 255).any())
    for c in P.scorer_queries(hist):
        ent, sh = P.query(hist, **c)
        ent2, sh2 = query_loops(hist, **c)
        assert np.array_equal(ent, ent2) and np.array_equal(sh, sh2), c
        queries = list(range(n)) if c["queries"] is None else c["queries"]
        ids = c["ids"].astype(np.int64)
        for row, q in enumerate(queries):
            got = ent[row][ent[row] >= 0]
            assert q not in got and len(set(got.tolist())) == len(got)
            assert (np.abs(ids[got] - ids[q]) >= c["min_gap"]).all() and (sh[row][:len(got)] >= c["min_shared"]).all()
            assert (np.diff(sh[row]) <= 0).all() and not sh[row][len(got):].any()
        if c["min_gap"] == 5 and n >= 17:
            assert ent[8, 0] == 13 and 4 not in ent[8] and 12 not in ent[8]      # 13 is on the bound above, 4 and 12 are inside it
            assert n <= 20 or ent[20, 0] == 15 and 16 not in ent[20]            # 15 is on the bound below
        if c["min_gap"] == 0 and c["min_shared"] == 0 and c["queries"] is None and c["top_k"] == 3 and n >= 17:
            assert ent[8].tolist() == [4, 12, 13] and len(set(sh[8].tolist())) == 1
        if c["min_gap"] > 5 and n >= 2:                          # differences beyond 32 bits: only the pairs across both ends pass
            far = int((np.abs(ids - ids[0]) >= c["min_gap"]).sum())
            assert 0 < far < n - (n > 2) and (ent[0] >= 0).sum() == min(3, far)
        if c["min_shared"] > 0:
            assert sh[0, 0] == c["min_shared"]
    if n > 70:                                                  # equal scores: ascending entries, in one block and across two
        ent, sh = P.query(hist, np.arange(n), [0], top_k=16)
        s = P.shared_row(hist, 0)
        assert s[5] == s[9] == s[70]
        at = {int(e): k for k, e in enumerate(ent[0])}
        if 5 in at:
            assert at[9] == at[5] + 1 and at.get(70, at[9] + 1) == at[9] + 1


def test_a_larger_vocabulary_changes_nothing_in_the_scorer():
    hist = P.histogram_case(65, K=512)
    for c in P.scorer_queries(hist)[:3]:
        a, b = P.query(hist, **c), query_loops(hist, **c)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ the wide cases (tests/test_gpu_places_shapes.py)
@pytest.mark.parametrize("name", tuple(P.WIDE_CASES))
def test_the_plan_of_every_wide_case(name):
    """vo_places_query's dealing rule as places_reference.split_plan restates it: each case reaches the path it is named for.  If
    the host's rule changes, this table fails and the cases are chosen again."""
    n, Q = P.WIDE_CASES[name]
    plan = P.split_plan(n, Q)
    assert plan == P.WIDE_PLANS[name]
    splits, per_split, tiles_per_split, used, empty = plan
    walked = [(sp * per_split, min(n, (sp + 1) * per_split)) for sp in range(splits)]          # k_places_score's e_begin, e_end
    tiles = [max(0, -(-(b - a) // 64)) for a, b in walked]
    assert sum(t > 0 for t in tiles) == used and sum(t == 0 for t in tiles) == empty and sum(max(0, b - a) for a, b in walked) == n
    assert len(P.wide_queries(name)) == Q
    if name == "two_tiles":
        assert tiles == [2, 2, 1, 0] and walked[2] == (256, 257) and walked[3][0] >= n
    elif name == "one_workgroup":
        assert tiles == [5] and n - 4 * 64 == 1
    elif name == "one_workgroup_65":
        assert tiles == [2] and n - 64 == 1
    elif name == "full_merge":
        assert tiles == [1] * 64 and splits * 16 == 1024 and min(b - a for a, b in walked) >= 16 and -(-Q // 64) == 2
    elif name == "past_the_merge":
        assert tiles == [2] * 32 + [1] + [0] * 31 and walked[32] == (4096, 4097) and -(-Q // 64) == 2
    # the cases of tests/test_gpu_places.py walk one tile a split, as that file's sibling says
    assert all(P.split_plan(m, Q)[2] == 1 for m in P.INDEX_SIZES for Q in (1, 3, m))


@pytest.mark.parametrize("n", P.INDEX_SIZES)
def test_the_vectorised_query_equals_the_loop_form(n):
    hist = P.histogram_case(n)
    for c in P.scorer_queries(hist):
        a, b = P.query(hist, **c), P.query_vec(hist, **c)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype, c
    if n == 65:
        wide = P.histogram_case(65, K=512)
        for c in P.scorer_queries(wide)[:3]:
            a, b = P.query(wide, **c), P.query_vec(wide, **c)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


LOOP_QUERIES = (5, 9, P.LAST_QUERY, P.FIRST_QUERY, 0)          # the queries the loops answer in every call of a wide case


@pytest.mark.parametrize("n", sorted({n for n, _ in P.WIDE_CASES.values()}))
def test_wide_scorer_cases(n):
    hist = P.histogram_case_wide(n)
    base = P.histogram_case(n)
    moved = sorted(set(np.flatnonzero((hist != base).any(axis=1)).tolist()))
    copies = [b for b in P.COPIES_OF_5 if b < n]
    assert set(moved) <= set(copies) | set(P.last16(n)) | set(P.FIRST16)                      # the seeded entries stay
    assert (hist == 0).any() and (hist == 255).any() and all(np.array_equal(hist[b], hist[5]) for b in copies)
    names = [k for k, v in P.WIDE_CASES.items() if v[0] == n]
    lists = {k: P.wide_queries(k) for k in names}
    for k, q in lists.items():
        assert {5, P.LAST_QUERY, P.FIRST_QUERY, 0} | set(copies) <= set(q.tolist()) and q.min() >= 0 and q.max() < n
        assert n > 257 or set(q.tolist()) == set(range(n))
        assert n <= 257 or len(set(q.tolist())) == len(q)
    if n > 257:
        assert np.array_equal(lists["past_the_merge" if n == 4097 else "full_merge"][:70], P.wide_queries("full_merge"))
    calls = P.wide_calls(hist)
    assert [(c["top_k"], c["min_gap"]) for c in calls] == [(1, 0), (3, 0), (16, 0), (16, 5), (3, (1 << 31) - 1), (16, 0)] and calls[5]["min_shared"] > 0
    distinct = np.unique(np.concatenate(list(lists.values())))
    for i, c in enumerate(calls):
        # The loops answer the call that ranks all candidates (top_k 16, no bound: top_k 1 and 3 are its first columns, asserted
        # below) for every entry of 65 and 257 and every sixth chosen query of 4096 and 4097, and LOOP_QUERIES in every call.
        asked = np.array(LOOP_QUERIES)
        if i == 2:
            asked = np.union1d(asked, distinct if n <= 257 else distinct[::6])
        ent, sh = P.query_vec(hist, c["ids"], asked, c["top_k"], c["min_gap"], c["min_shared"])
        ent2, sh2 = query_loops(hist, c["ids"], asked, c["top_k"], c["min_gap"], c["min_shared"])
        assert np.array_equal(ent, ent2) and np.array_equal(sh, sh2), (n, c["top_k"], c["min_gap"], c["min_shared"])
    ids = calls[0]["ids"]
    full, full_sh = P.query_vec(hist, ids, distinct, 16)
    for k in (1, 3):
        e, s = P.query_vec(hist, ids, distinct[::4], k)
        assert np.array_equal(e, full[::4, :k]) and np.array_equal(s, full_sh[::4, :k])
    for k, q in lists.items():                                 # a repeated list is the distinct answers indexed by the list
        e, s = P.query_list(hist, ids, q, 16)
        assert np.array_equal(e, full[np.searchsorted(distinct, q)]) and np.array_equal(s, full_sh[np.searchsorted(distinct, q)]) and len(e) == len(q)
        pick = np.random.default_rng(n).integers(0, len(q), 8)
        single = P.query_vec(hist, ids, q[pick], 16)
        assert np.array_equal(e[pick], single[0]) and np.array_equal(s[pick], single[1])
    row = {int(q): i for i, q in enumerate(distinct)}
    # the copies of entry 5: equal scores with every query, reported in ascending entry order at top_k 1, 3 and 16
    five = [5] + copies
    for q in five:
        others = [d for d in five if d != q]
        for k in P.TOP_KS:
            e, s = P.query_vec(hist, ids, [q], k)
            assert e[0].tolist()[:len(others)] == others[:k] and len(set(s[0][:len(others)].tolist())) == 1
    s0 = P.shared_row(hist, 0)
    assert len({int(s0[d]) for d in five}) == 1
    # the "last tile" query: sixteen best at last16, scores ascending with the entry — each lands at position 0 of the list
    last = list(P.last16(n))
    assert full[row[P.LAST_QUERY]].tolist() == last[::-1] and (np.diff(full_sh[row[P.LAST_QUERY]]) == -1).all()
    beyond = np.delete(P.shared_row(hist, P.LAST_QUERY), [P.LAST_QUERY] + last).max()
    assert beyond < full_sh[row[P.LAST_QUERY], 15]
    if n == 65:
        assert last[-1] == 64 and full[row[P.LAST_QUERY], 0] == 64          # the best of all is the one entry of the last tile
    else:
        tile = last[0] // 64
        assert last[-1] // 64 == tile and last[0] > 16                      # one tile, and not the first: the list is full before
        for k in names:
            _, per_split, tiles_per_split, _, _ = P.split_plan(*P.WIDE_CASES[k])
            if k == "one_workgroup":                                        # there only entry 256, a copy of 5, comes later
                assert tile == tiles_per_split - 2 and n - (tile + 1) * 64 == 1
            else:
                assert (tile + 1) % tiles_per_split == 0                    # the last tile its workgroup walks
    # the "first tile" query: sixteen best in tile 0, every later candidate below the sixteenth
    first = full[row[P.FIRST_QUERY]]
    assert sorted(first.tolist()) == list(P.FIRST16) and max(P.FIRST16) < 64 and first.tolist() != sorted(first.tolist())
    assert np.delete(P.shared_row(hist, P.FIRST_QUERY), [P.FIRST_QUERY] + list(P.FIRST16)).max() < full_sh[row[P.FIRST_QUERY], 15]
    # the bound of the last call is a score query 0 reports, so an entry lies on it
    e, s = P.query_vec(hist, ids, [0], 16, 0, calls[5]["min_shared"])
    assert (s[0][e[0] >= 0] >= calls[5]["min_shared"]).all() and s[0][(e[0] >= 0).sum() - 1] == calls[5]["min_shared"] and (e[0] >= 0).sum() >= 3


@pytest.mark.parametrize("K", (1024, 4096))
def test_wide_vocabulary_scorer_case(K):
    hist = P.histogram_case_k(K)
    assert hist.shape == (65, K) and (hist == 0).any() and (hist == 255).any()
    wide = hist.astype(np.int64)
    assert wide[P.ALL_255].sum() == 255 * K and wide[P.ALL_0].sum() == 0 and np.abs(wide[P.ALL_255] - wide[P.ALL_0]).sum() == 255 * K
    assert K != 4096 or 255 * K == 1044480
    ids = np.arange(65)
    for top_k in (3, 16):
        a, b = P.query_vec(hist, ids, None, top_k), query_loops(hist, ids, None, top_k, 0, 0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    e, s = P.query_vec(hist, ids, [P.ALL_255, P.ALL_0], 16)
    assert np.array_equal(s[0], np.sort(np.delete(wide.sum(axis=1), P.ALL_255))[::-1][:16])    # all 255 shares every entry's whole sum
    assert not s[1].any() and e[1].tolist() == list(range(16))


@pytest.mark.parametrize("det", DETECTORS)
@pytest.mark.parametrize("K", (1024, 4096))
def test_wide_vocabulary_histograms(oracle, det, K):
    words = P.vocabulary_case(det, K)
    C = P.CHUNK[det]
    assert np.array_equal(words[K - 1], words[P.FIRST_AGAINST_LAST]) and (K - 1) // C == K // C - 1 and P.FIRST_AGAINST_LAST // C == 0
    assert np.array_equal(P.vocabulary_case(det, 256), P.vocabulary_case(det, 256)) and K // C in (4, 8, 16, 32)
    frames = P.histogram_frames(det, words)
    assert [len(f) for f in frames] == [300, 0, 300, 7]
    word = [P.quantise(f, words) for f in frames]
    hist, s = np.stack([P.histogram(w, K)[0] for w in word]), [P.histogram(w, K)[1] for w in word]      # P.entries, the words kept
    step = 2 if K == 1024 else 16                             # the loops take every second row at K = 1024, every sixteenth at K = 4096
    for f, w, h, t in zip(frames, word, hist, s):
        keep = np.arange(0, len(f), step) if len(f) > 7 else np.arange(len(f))
        assert np.array_equal(w[keep], quantise_loops(f[keep], words)), (det, K, len(f))
        assert [min(255, int((w == k).sum())) for k in range(K)] == h.tolist() and t == h.astype(int).sum()
    assert hist[0, 11] == 255 and s[0] == 255 and s[1] == 0 and s[2] == 300 and s[3] == 7
    assert word[3].tolist() == [K - 4, 1, K - 3, K - 2, 1, K - 2, K - 2]                        # the lowest index wins the tie of 1 with K - 1
    assert hist[3, K - 4:].tolist() == [1, 1, 3, 0] and hist[3, 1] == 2
    # the ordinary frame meets the other ties too
    dup = [a for a, b in ((2, 3), (5, 21), (0, C), (40, 40 + C)) if b < K]
    w = word[2]
    assert [int(w[2 * k]) for k in range(len(dup)) if 2 * k != 1] == dup and w[1] == P.EQUIDISTANT[0] and len(dup) == 4


@pytest.mark.parametrize("det", DETECTORS)
def test_wide_frames(oracle, det):
    words = P.vocabulary_case(det, 256)
    C = P.CHUNK[det]
    dup = [a for a, b in ((2, 3), (5, 21), (0, C), (40, 40 + C)) if b < 256]
    for n in P.FRAME_SIZES:                                    # frames of one workgroup are what they were
        assert len(P.frame_case(det, words, n)) == n
    for n in P.WIDE_FRAME_SIZES:
        f = P.frame_case(det, words, n)
        w = P.quantise(f, words)
        assert len(w) == n and n > P.BLOCK_ROWS and n <= P.WIDE_KP_CAP
        # the loops take the rows around every workgroup's first row and every sixteenth row
        keep = sorted(set(range(0, n, 16)) | {i for b in range(0, n, P.BLOCK_ROWS) for i in range(b, min(n, b + 12))} | {n - 1})
        assert np.array_equal(w[keep], quantise_loops(f[keep], words)), (det, n)
        for base in range(0, n, P.BLOCK_ROWS):                 # the ties are met in every workgroup's rows, as far as it has rows
            for k, src in enumerate(dup):
                if base + 2 * k < n and 2 * k != 1:
                    assert w[base + 2 * k] == src and np.array_equal(f[base + 2 * k], words[src])
            if base + 1 < n:
                assert w[base + 1] == P.EQUIDISTANT[0]
        assert (n - 1) // P.BLOCK_ROWS == (1 if n <= 1024 else 2)
    assert [(n - 1) % P.BLOCK_ROWS + 1 for n in P.WIDE_FRAME_SIZES] == [1, 512, 1, 512]        # a workgroup of one row, and full ones


def _spot_checked(rows_step, words_step):
    """P.quantise and P.update as P.train calls them, each call held to the loops on every rows_step-th row / words_step-th word"""
    def quantiser(rows, words):
        w = P.quantise(rows, words)
        at = np.arange(0, len(rows), rows_step)
        assert np.array_equal(w[at], quantise_loops(rows[at], words))
        return w

    def updater(rows, word, words):
        out = P.update(rows, word, words)
        only = list(range(0, len(words), words_step))
        assert np.array_equal(out[only], update_loops(rows, word, words, only)[only])
        return out
    return quantiser, updater


@pytest.mark.parametrize("det", DETECTORS)
@pytest.mark.parametrize("name", P.WIDE_TRAINING_CASES)
def test_wide_training_cases(oracle, det, name):
    c = P.training_case_wide(det, name)
    K, frames = c["K"], c["frames"]
    rows = np.concatenate(frames); n = len(rows)
    quantiser, updater = _spot_checked(32 if K == 1024 else 8, 16 if K == 1024 else 4)
    words, run = P.train(frames, K, c["iterations"], quantiser=quantiser, updater=updater)
    print(det, name, "n", n, "iterations_run", run)
    assert len(c["slots"]) == len(frames) == len(set(c["slots"])) and max(len(f) for f in frames) <= P.WIDE_KP_CAP
    assert max(c["slots"]) < P.WIDE_FRAMES[det]
    if name == "planted_1024":
        centres = P.planted_case(det, K)[1]
        assert [len(f) for f in frames] == [1024] * 3 and run == 1 < c["iterations"] and np.array_equal(words, centres)
        assert np.array_equal(P.quantise(rows[::4], words), np.arange(0, n, 4) // 3)
    elif name == "crowded_1024":
        assert [len(f) for f in frames] == [1025, 17, 513] and run == c["iterations"] == 2
        assert P.train(frames, K, 3)[1] == 3                    # still moving: a third round would have run
    elif name == "stride":
        F, cap = P.WIDE_FRAMES[det], P.WIDE_KP_CAP
        counts = [len(f) for f in frames]
        assert len(frames) == F and sorted(c["slots"]) == list(range(F)) and c["slots"] != sorted(c["slots"])
        assert counts[-1] == 1025 and sorted(counts)[-4:] == [300, 450, 600, 1025] and sorted(counts)[-5] <= 3 and 0 in counts
        assert 2000 <= n <= 3200 and run == c["iterations"] == 2 and P.train(frames, K, 3)[1] == 3
        # rows whose flat index q kp_cap + i is at or past the first pass of k_vocab_accumulate's grid
        edge = P.ACCUMULATE_GRID * P.ACCUMULATE_ROWS[det]
        assert edge == (32768 if det == "sift" else 262144) and F * cap > edge
        live = [(q, i) for q in range(F) for i in range(counts[q]) if q * cap + i >= edge]
        assert len(live) >= P.BLOCK_ROWS and (F - 1) * cap + counts[-1] > edge
        # they count: without them the first update gives other words
        first = P.train(frames, K, 1)[0]
        at = np.concatenate([[0], np.cumsum(counts)])
        flat = np.array([at[q] + i for q, i in live])
        word = P.quantise(rows, rows[[(w * n) // K for w in range(K)]])
        cut = np.delete(np.arange(n), flat)
        assert not np.array_equal(P.update(rows[cut], word[cut], rows[[(w * n) // K for w in range(K)]]), first)
        # the start rows of words 6 and 7 are equal: word 7 gets no row in the first round and keeps its own
        a, b = (6 * n) // K, (7 * n) // K
        assert a != b and np.array_equal(rows[a], rows[b]) and 7 not in word.tolist() and 6 in word.tolist()
        assert np.array_equal(first[7], rows[b]) and not np.array_equal(first[6], rows[a])


# ------------------------------------------------------------------ the scene: a course flown 1 1/4 times
SCENE = dict(lap=16, per_step=24, seed=0, K=256, min_shared=31)


def _example():
    spec = importlib.util.spec_from_file_location("find_loops", os.path.join(ROOT, "examples", "find_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_revisits_are_found_and_nothing_else(oracle):
    ex = _example()
    course = ex.loop_course(SCENE["lap"], SCENE["per_step"], seed=SCENE["seed"])
    frames = course["frames"]
    n, lap = len(frames), SCENE["lap"]
    assert n == 20 and ex.MAX_FLIPS == 10
    for f in frames:                                           # at most 10 of 256 bits flipped per observation
        flips = np.unpackbits(f["rows"] ^ course["rows"][f["landmarks"]], axis=1).sum(axis=1)
        assert flips.max() <= 10
    min_gap = lap // 2
    truth = ex.true_revisits(course, min_gap, overlap=0.6)
    revisiting = [i for i in range(n) if truth[i]]
    # the second lap's frames and the first quarter they fly over again; frame 15 too: on a closed course it neighbours frame 0
    assert set(range(lap, n)) <= set(revisiting) and set(range(lap // 4)) <= set(revisiting) and 6 <= n - len(revisiting)
    words, run = P.train([f["rows"] for f in frames[:lap]], SCENE["K"])
    hist, _ = P.entries([f["rows"] for f in frames], words)
    ids = np.arange(n)
    ent, sh = P.query(hist, ids, top_k=1, min_gap=min_gap, min_shared=SCENE["min_shared"])
    free, free_sh = P.query(hist, ids, top_k=n, min_gap=min_gap, min_shared=0)
    true_low = min(int(free_sh[i, 0]) for i in revisiting)                       # the best candidate of a revisiting frame
    false_high = max(int(free_sh[i, 0]) for i in range(n) if i not in revisiting)   # ... of a frame that revisits nothing
    print(f"scene: {n} frames, {run} updates, smallest true top-1 shared {true_low}, largest shared of a frame without a revisit {false_high}, "
          f"min_shared {SCENE['min_shared']}")
    for i in range(n):
        if i in revisiting:
            assert ent[i, 0] in truth[i], (i, ent[i], truth[i])
        else:
            assert ent[i, 0] == -1, (i, ent[i], sh[i])
    assert false_high < SCENE["min_shared"] <= true_low

"""No GPU: tests/places_reference.py (numpy + the CPU oracle) against a second, loop-by-loop restatement written from the rules in
include/vo_hip.h ("place recognition") on every case tests/test_gpu_places.py uses, and every case against what it is named for:
planted centres come back exactly, an empty cluster keeps its word, ORB majority ties give 0, SIFT means ending in .5 round up.
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


def update_loops(rows, word, words):
    out = words.copy()
    D = rows.shape[1]
    for w in range(len(words)):
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

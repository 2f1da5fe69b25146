"""GPU: place recognition at the sizes the benchmark and examples/find_loops.py run and tests/test_gpu_places.py does not reach — more
than one tile of entries a workgroup, more than one quantiser workgroup a slot, a second pass of k_vocab_accumulate's grid, 1024 and
4096 words — on rows and histograms the test CHOSE, against tests/places_reference.py; tests/test_places_reference.py holds every
case here equal, on the CPU, to the loop-by-loop restatement and to what it is named for, and asserts the plan table below.  Both
detectors; everything is integers, so everything is array_equal.

Held here (the plan of a query is places_reference.split_plan(n, Q), restated from vo_places_query):
  scorer      n 257, Q 19 200   4 splits of 128   splits 0 and 1 walk two tiles, split 2 holds one entry, split 3 starts past n
              n 257, Q 65 536   1 split of 320    five tiles through one list of the best, the last tile one entry
              n 65,  Q 65 536   1 split of 128    a full tile, then one entry
              n 4096, Q 70      64 splits of 64   k_places_merge holds 1024 keys
              n 4097, Q 71      64 splits of 128  33 splits in use, the last of one entry; 31 start past n
              each with copies of entry 5 in one tile, in two tiles of a split, in two splits and in the last short tile; a query
              whose sixteen best arrive last and in ascending order (every insertion at position 0 of a full list) and one whose
              sixteen best lie in the first tile (every later key turned away); top_k 1, 3, 16, min_gap 5, ids at both ends of int32,
              min_shared on a reported score;
  K           1024 and 4096 words: the scorer's K loop beyond two LDS stages with an all-255 and an all-0 entry (sum and L1
              1 044 480), k_places_sums, k_places_hist with a vocabulary of 8 to 32 staged chunks whose last word repeats word 1,
              a frame on the histogram's last dword; training at K = 1024 (planted centres; a crowded case that uses two rounds);
  wide rigs   kp_cap 1536 — three quantiser workgroups a slot — with 22 SIFT slots and 172 ORB slots, as the issue states them
              (configuring the 172 ORB slots takes 0.01 s, measured): frames of 513, 1024, 1025 and 1536 rows in slots other than 0, a slot that
              held 1536 rows and then 513, entries of 1025, 17 and 513 rows in slot-list order, and a training over every slot in a
              seeded order whose last list position holds 1025 rows: flat rows at and past 8192 workgroups x 4 (SIFT) / 32 (ORB)
              rows, k_vocab_accumulate's second pass.
Each of five deliberate mistakes in reloc_kernels.hip — the list of the best cleared at every tile, the merge reading 128 keys, one pass
of the accumulate grid, row0 = 0 in the quantiser, the scorer's K loop ending at 512 — fails tests of this file; which ones is in
docs/kernels/k_places.md, "Parity".
The whole file takes 2.9 s on an MI355X (28 tests; measured, one run, the reference's side included); the slowest test 0.56 s."""
import functools

import numpy as np
import pytest

import places_reference as P
import relocalize_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=("sift", "orb"))
def wide(request):
    from visual_odometry_amd.frontend import FrontEnd
    det = request.param
    F = P.WIDE_FRAMES[det]
    if det == "sift":
        fe = FrontEnd(32, 32, max_frames=F, max_pairs=1, detector="sift", kp_cap=P.WIDE_KP_CAP)
    else:
        fe = FrontEnd(64, 64, max_frames=F, max_pairs=1, nfeatures=1280, nlevels=1)
    # a change of the capacity rule must not quietly undo the cases: three quantiser workgroups a slot, and a second accumulate pass
    assert fe.kp_cap == P.WIDE_KP_CAP == 3 * P.BLOCK_ROWS
    assert (F * fe.kp_cap > 32768) if det == "sift" else (F * fe.kp_cap > 262144)
    assert F * fe.kp_cap > P.ACCUMULATE_GRID * P.ACCUMULATE_ROWS[det]
    yield det, fe
    fe.ctx.close()


def _put(fe, det, slot, rows):
    (fe.set_sift_rows if det == "sift" else fe.set_orb_rows)(slot, np.ascontiguousarray(rows, np.uint8))


# ------------------------------------------------------------------ the scorer past one tile and one split
@functools.lru_cache(maxsize=None)
def _scorer_case(name):
    """(hist, queries, [(call, entry, shared)]): computed once, shared by both detectors, never changed"""
    n, Q = P.WIDE_CASES[name]
    hist = P.histogram_case_wide(n)
    queries = P.wide_queries(name)
    assert len(hist) == n and len(queries) == Q
    return hist, queries, [(c,) + P.query_list(hist, c["ids"], queries, c["top_k"], c["min_gap"], c["min_shared"]) for c in P.wide_calls(hist)]


@pytest.mark.parametrize("name", tuple(P.WIDE_CASES))
def test_queries_past_one_tile_and_one_split(wide, name):
    det, fe = wide
    hist, queries, calls = _scorer_case(name)
    n, Q = P.WIDE_CASES[name]
    assert P.split_plan(n, Q) == P.WIDE_PLANS[name]
    fe.set_vocabulary(R.rand_rows(np.random.default_rng(1), 256, det))
    last_ids = None
    for c, ent, sh in calls:
        if last_ids is None or not np.array_equal(last_ids, c["ids"]):
            fe.places_open(n)
            assert fe.places_add_histograms(hist, c["ids"]) == 0
            last_ids = c["ids"]
            e = fe.places_entries()
            assert np.array_equal(e["hist"], hist) and np.array_equal(e["sum"], hist.astype(np.int64).sum(axis=1)) and np.array_equal(e["id"], c["ids"])
        out = fe.places_query(queries, top_k=c["top_k"], min_gap=c["min_gap"], min_shared=c["min_shared"])
        where = (name, c["top_k"], c["min_gap"], c["min_shared"])
        assert out["entry"].dtype == np.int32 and out["entry"].shape == (Q, c["top_k"]) and np.array_equal(out["entry"], ent), where
        assert np.array_equal(out["shared"], sh), where
        assert np.array_equal(out["id"], np.where(ent >= 0, c["ids"][np.maximum(ent, 0)], 0)), where
        assert not (out["entry"] == queries[:, None]).any()    # an entry never meets itself
    again = fe.places_query(queries, top_k=c["top_k"], min_gap=c["min_gap"], min_shared=c["min_shared"])
    assert np.array_equal(again["entry"], out["entry"]) and np.array_equal(again["shared"], out["shared"])


# ------------------------------------------------------------------ 1024 and 4096 words
@pytest.mark.parametrize("K", (1024, 4096))
def test_the_scorer_on_wide_vocabularies(wide, K):
    """every histogram passes through LDS in 4 and 16 stages; k_places_sums takes 4 and 16 loads a lane"""
    det, fe = wide
    hist = P.histogram_case_k(K)
    ids = np.arange(65, dtype=np.int32)
    fe.set_vocabulary(R.rand_rows(np.random.default_rng(3), K, det))
    fe.places_open(65)
    assert fe.places_add_histograms(hist, ids) == 0
    e = fe.places_entries()
    assert np.array_equal(e["hist"], hist) and np.array_equal(e["sum"], hist.astype(np.int64).sum(axis=1))
    assert e["sum"][P.ALL_255] == 255 * K and e["sum"][P.ALL_0] == 0
    for top_k in (3, 16):
        ent, sh = P.query_vec(hist, ids, None, top_k)
        out = fe.places_query(top_k=top_k)
        assert np.array_equal(out["entry"], ent) and np.array_equal(out["shared"], sh), (K, top_k)
    assert (out["shared"][P.ALL_0] == 0).all() and out["entry"][P.ALL_0].tolist() == [d for d in range(17) if d != P.ALL_0][:16]


@functools.lru_cache(maxsize=None)
def _entries_case(det, K):
    words = P.vocabulary_case(det, K)
    frames = P.histogram_frames(det, words)
    return words, frames, P.entries(frames, words), [P.quantise(f, words) for f in frames]


@pytest.mark.parametrize("K", (1024, 4096))
def test_entries_on_wide_vocabularies(wide, oracle, K):
    """k_places_hist with 4 and 16 counters' dwords a lane; the quantiser over 8 to 32 staged chunks, first chunk tied with the last"""
    det, fe = wide
    words, frames, (hist, s), word = _entries_case(det, K)
    fe.set_vocabulary(words)
    assert fe.vocabulary().tobytes() == words.tobytes()
    slots = [4, 1, 3, 2]
    for slot, f in zip(slots, frames):
        _put(fe, det, slot, f)
    ids = np.array([7, -3, 2 ** 31 - 1, -2 ** 31], np.int32)
    fe.places_open(4)
    assert fe.places_add(slots, ids) == 0
    got = fe.places_entries()
    assert got["hist"].shape == (4, K) and np.array_equal(got["hist"], hist)
    assert np.array_equal(got["sum"], s) and np.array_equal(got["id"], ids)
    for slot, f, w in zip(slots, frames, word):
        assert np.array_equal(fe.words(slot), w), (det, K, len(f))
    tail = fe.words(slots[3])
    assert P.FIRST_AGAINST_LAST in tail and K - 1 not in tail      # the lowest index wins the tie of word 1 with word K - 1
    assert got["hist"][3, K - 4:].tolist() == [1, 1, 3, 0] and got["hist"][0, 11] == 255 and got["sum"][0] == 255


# ------------------------------------------------------------------ three quantiser workgroups a slot
@functools.lru_cache(maxsize=None)
def _frames_case(det):
    words = P.vocabulary_case(det, 256)
    frames = {n: P.frame_case(det, words, n) for n in P.WIDE_FRAME_SIZES + (17,)}
    return words, frames, {n: P.quantise(f, words) for n, f in frames.items()}


def test_words_of_rows_past_the_first_workgroup(wide, oracle):
    det, fe = wide
    words, frames, want = _frames_case(det)
    fe.set_vocabulary(words)
    slots = dict(zip(P.WIDE_FRAME_SIZES, (3, 7, 12, P.WIDE_FRAMES[det] - 1)))
    for n, slot in slots.items():
        _put(fe, det, slot, frames[n])
    for n, slot in slots.items():
        got = fe.words(slot)
        assert got.dtype == np.int32 and len(got) == n and np.array_equal(got, want[n]), (det, n)
    # a slot that held 1536 rows and then 513: rows 513 .. still hold the old frame, whose rows are copies of words
    _put(fe, det, slots[1536], frames[513])
    assert np.array_equal(fe.words(slots[1536]), want[513])


def test_entries_in_slot_list_order(wide, oracle):
    """word + q * kp_cap for q > 0 with three workgroups a slot"""
    det, fe = wide
    words, frames, want = _frames_case(det)
    fe.set_vocabulary(words)
    slots, sizes = [9, 2, 5], (1025, 17, 513)
    for slot, n in zip(slots, sizes):
        _put(fe, det, slot, frames[n])
    ids = np.array([40, -1, 3], np.int32)
    fe.places_open(3)
    assert fe.places_add(slots, ids) == 0
    got = fe.places_entries()
    hs = [P.histogram(want[n], 256) for n in sizes]
    assert np.array_equal(got["hist"], np.stack([h for h, _ in hs])) and got["sum"].tolist() == [t for _, t in hs] and np.array_equal(got["id"], ids)


# ------------------------------------------------------------------ training: K = 1024, and the grid's second pass
@functools.lru_cache(maxsize=None)
def _training_case(det, name):
    c = P.training_case_wide(det, name)
    return c, P.train(c["frames"], c["K"], c["iterations"])


@pytest.mark.parametrize("name", P.WIDE_TRAINING_CASES)
def test_training_on_the_wide_rig(wide, oracle, name):
    det, fe = wide
    c, (want, want_run) = _training_case(det, name)
    slots, frames = c["slots"], c["frames"]
    if name == "stride":
        # rows of the last list positions lie at and past the flat index the grid's first pass ends at
        edge = P.ACCUMULATE_GRID * P.ACCUMULATE_ROWS[det]
        live = sum(max(0, q * fe.kp_cap + len(f) - max(edge, q * fe.kp_cap)) for q, f in enumerate(frames))
        assert len(slots) == fe.max_frames and sorted(slots) == list(range(fe.max_frames)) and live >= P.BLOCK_ROWS, (det, live)
    for slot, f in zip(slots, frames):
        _put(fe, det, slot, f)
    run = fe.train_vocabulary(slots, K=c["K"], iterations=c["iterations"])
    got = fe.vocabulary()
    print(det, name, "rows", sum(len(f) for f in frames), "iterations_run", run, "reference", want_run)
    assert run == want_run == {"planted_1024": 1, "crowded_1024": 2, "stride": 2}[name]
    assert got.shape == want.shape and np.array_equal(got, want)
    for slot, f in zip(slots, frames):
        if len(f) > 3:
            assert np.array_equal(fe.words(slot), P.quantise(f, want)), (det, name, slot)
    again = fe.train_vocabulary(slots, K=c["K"], iterations=c["iterations"])
    assert again == run and fe.vocabulary().tobytes() == got.tobytes()

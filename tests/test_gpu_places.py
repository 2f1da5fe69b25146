"""GPU: place recognition — k_vocab_store, k_vocab_assign / k_vocab_assign_orb, k_vocab_accumulate, k_vocab_update, k_places_hist,
k_places_score and k_places_merge behind vo_vocab_* / vo_places_* — on descriptor rows and histograms the test CHOSE
(FrontEnd.set_sift_rows / set_orb_rows, set_vocabulary, places_add_histograms: no detection anywhere), against
tests/places_reference.py, which tests/test_places_reference.py holds equal on the CPU to a loop-by-loop restatement and to what every
case is named for.  Both detectors; everything is integers, so everything is array_equal.

Held here:
  quantiser   words(slot) after set_vocabulary: K = 256 and 512, frames of 0, 1, 17 and 300 rows, duplicated words a lane, a
              16-column group and a staged chunk apart (the ORB chunk needs K = 512), a row equidistant from two words, a slot that
              held a fuller frame before;
  training    n = K, n = K + 1 (an empty cluster; ORB majority ties, SIFT means ending in .5), three slots of unequal size that use
              all their rounds, planted centres that stop after one update; iterations_run; two runs give the same bytes;
  histograms  300 identical rows (saturated at 255: sum != rows), an empty frame, ordinary frames;
  scorer      indexes of 1, 2, 17, 64, 65 and 257 chosen histograms with bytes 0 and 255; top_k 1, 3, 16 (more places than
              candidates); equal scores in one block and in two; min_gap and min_shared with an entry exactly on the bound; ids at
              both ends of int32; one query, repeated queries, all entries; a 512-word index (two LDS stages);
  lifetime    a new vocabulary closes the index, a configure call releases both, relocalize() and slam_map() unchanged by an add and
              a query;
  arguments   every VO_ERR_* the header names for these entries.
The whole file takes 1.3 s on an MI355X (measured, one run, the reference's side included); the slowest test 0.15 s."""
import numpy as np
import pytest

import places_reference as P
import relocalize_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=("sift", "orb"))
def rig(request):
    from visual_odometry_amd.frontend import FrontEnd
    det = request.param
    if det == "sift":
        fe = FrontEnd(32, 32, max_frames=5, max_pairs=3, detector="sift", kp_cap=512)
    else:
        fe = FrontEnd(64, 64, max_frames=5, max_pairs=3, nfeatures=304, nlevels=1)
    assert fe.kp_cap >= 300
    yield det, fe
    fe.ctx.close()


def _put(fe, det, slot, rows):
    (fe.set_sift_rows if det == "sift" else fe.set_orb_rows)(slot, np.ascontiguousarray(rows, np.uint8))


def _code(exc):
    return exc.value.code


# ------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("K", (256, 512))
def test_words_equal_the_reference(rig, oracle, K):
    det, fe = rig
    words = P.vocabulary_case(det, K)
    fe.set_vocabulary(words)
    assert fe.vocabulary().tobytes() == words.tobytes()
    frames = {n: P.frame_case(det, words, n) for n in P.FRAME_SIZES}
    for slot, n in enumerate((300, 17, 1, 0)):
        _put(fe, det, slot, frames[n])
    for slot, n in enumerate((300, 17, 1, 0)):
        got = fe.words(slot)
        assert got.dtype == np.int32 and np.array_equal(got, P.quantise(frames[n], words)), (det, K, n)
    # a slot that held a fuller frame: rows 17 .. 299 of slot 0 still hold the old frame, whose rows are copies of words
    _put(fe, det, 0, frames[17])
    assert np.array_equal(fe.words(0), P.quantise(frames[17], words))
    other = P.frame_case(det, words, 300, seed=1)
    _put(fe, det, 0, other)
    assert np.array_equal(fe.words(0), P.quantise(other, words))


# ------------------------------------------------------------------ training
@pytest.mark.parametrize("name", P.TRAINING_CASES)
def test_training_equals_the_reference(rig, oracle, name):
    det, fe = rig
    c = P.training_case(det, name)
    slots = [3, 0, 4][:len(c["frames"])]                       # slot-list order, not slot order
    for slot, f in zip(slots, c["frames"]):
        _put(fe, det, slot, f)
    want, want_run = P.train(c["frames"], c["K"], c["iterations"])
    run = fe.train_vocabulary(slots, K=c["K"], iterations=c["iterations"])
    got = fe.vocabulary()
    print(det, name, "iterations_run", run, "reference", want_run)
    assert run == want_run
    assert got.shape == want.shape and np.array_equal(got, want)
    assert run == {"exact": 1, "plus_one": 1, "three_slots": 2, "planted": 1}[name]
    # the trained words are stored as set words are: the quantiser on them equals the reference's
    for slot, f in zip(slots, c["frames"]):
        assert np.array_equal(fe.words(slot), P.quantise(f, want))
    again = fe.train_vocabulary(slots, K=c["K"], iterations=c["iterations"])
    assert again == run and fe.vocabulary().tobytes() == got.tobytes()
    if name == "three_slots":                                  # iterations below 1 count as 1
        assert fe.train_vocabulary(slots, K=c["K"], iterations=0) == 1
        assert np.array_equal(fe.vocabulary(), P.train(c["frames"], c["K"], 1)[0])


# ------------------------------------------------------------------ histograms
def test_entries_equal_the_reference(rig, oracle):
    det, fe = rig
    words = P.vocabulary_case(det, 256)
    frames = [np.repeat(words[11:12], 300, axis=0), np.zeros((0, P.width(det)), np.uint8), P.frame_case(det, words, 300), P.frame_case(det, words, 17)]
    fe.set_vocabulary(words)
    for slot, f in enumerate(frames):
        _put(fe, det, slot, f)
    fe.places_open(6)
    ids = np.array([7, -3, 2 ** 31 - 1, -2 ** 31], np.int32)
    assert fe.places_add([0, 1], ids[:2]) == 0
    assert fe.places_add([], []) == 2
    assert fe.places_add([2, 3], ids[2:]) == 2
    hist, s = P.entries(frames, words)
    got = fe.places_entries()
    assert got["hist"].dtype == np.uint8 and np.array_equal(got["hist"], hist)
    assert np.array_equal(got["sum"], s) and np.array_equal(got["id"], ids)
    assert got["hist"][0, 11] == 255 and got["sum"][0] == 255 and not got["hist"][1].any() and got["sum"][1] == 0
    # the scorer on entries that came from slots
    ent, sh = P.query(hist, ids, top_k=3)
    out = fe.places_query(top_k=3)
    assert np.array_equal(out["entry"], ent) and np.array_equal(out["shared"], sh)
    # a saved index comes back through places_add_histograms
    fe.places_open(4)
    assert fe.places_add_histograms(hist, ids) == 0
    back = fe.places_entries()
    assert all(np.array_equal(back[k], got[k]) for k in got)


# ------------------------------------------------------------------ scorer
@pytest.mark.parametrize("n", P.INDEX_SIZES)
def test_queries_equal_the_reference(rig, n):
    det, fe = rig
    fe.set_vocabulary(R.rand_rows(np.random.default_rng(1), 256, det))
    hist = P.histogram_case(n)
    last_ids = None
    for c in P.scorer_queries(hist):
        if last_ids is None or not np.array_equal(last_ids, c["ids"]):
            fe.places_open(n)
            half = n // 2
            assert fe.places_add_histograms(hist[:half], c["ids"][:half]) == 0      # fed in two chunks
            assert fe.places_add_histograms(hist[half:], c["ids"][half:]) == half
            last_ids = c["ids"]
            e = fe.places_entries()
            assert np.array_equal(e["hist"], hist) and np.array_equal(e["sum"], hist.astype(np.int64).sum(axis=1)) and np.array_equal(e["id"], c["ids"])
        ent, sh = P.query(hist, **c)
        out = fe.places_query(c["queries"], top_k=c["top_k"], min_gap=c["min_gap"], min_shared=c["min_shared"])
        assert out["entry"].dtype == np.int32 and np.array_equal(out["entry"], ent), (n, c["top_k"], c["min_gap"], c["min_shared"])
        assert np.array_equal(out["shared"], sh), (n, c["top_k"], c["min_gap"], c["min_shared"])
        assert np.array_equal(out["id"], np.where(ent >= 0, c["ids"][np.maximum(ent, 0)], 0))
        queries = np.arange(n) if c["queries"] is None else np.asarray(c["queries"])
        assert not (out["entry"] == queries[:, None]).any()    # an entry never meets itself
    again = fe.places_query(c["queries"], top_k=c["top_k"])
    assert np.array_equal(again["entry"], out["entry"]) and np.array_equal(again["shared"], out["shared"])


def test_a_larger_vocabulary_in_the_scorer(rig):
    """512 words: every histogram passes through LDS in two stages"""
    det, fe = rig
    fe.set_vocabulary(R.rand_rows(np.random.default_rng(2), 512, det))
    hist = P.histogram_case(65, K=512)
    fe.places_open(65)
    fe.places_add_histograms(hist, np.arange(65))
    for c in P.scorer_queries(hist)[:3]:
        ent, sh = P.query(hist, **c)
        out = fe.places_query(c["queries"], top_k=c["top_k"], min_gap=c["min_gap"], min_shared=c["min_shared"])
        assert np.array_equal(out["entry"], ent) and np.array_equal(out["shared"], sh)


# ------------------------------------------------------------------ lifetime
def test_lifetime(rig, oracle):
    from visual_odometry_amd import _lib
    det, fe = rig
    words = P.vocabulary_case(det, 256)
    fe.set_vocabulary(words)
    fe.places_open(4)
    _put(fe, det, 0, P.frame_case(det, words, 17))
    fe.places_add([0], [5])
    # a new vocabulary, set or trained, closes the index
    fe.set_vocabulary(words)
    with pytest.raises(_lib.VoError) as e:
        fe.places_entries()
    assert _code(e) == P.VO_ERR_INVALID
    fe.places_open(4)
    fe.places_add([0], [5])
    _put(fe, det, 1, P.training_case(det, "exact")["frames"][0])
    fe.train_vocabulary([1], K=256, iterations=1)
    with pytest.raises(_lib.VoError) as e:
        fe.places_query()
    assert _code(e) == P.VO_ERR_INVALID
    # a refused vocabulary changes nothing
    fe.places_open(4)
    fe.places_add([0], [5])
    before = fe.vocabulary()
    with pytest.raises(_lib.VoError) as e:
        fe.set_vocabulary(words[:255])
    assert _code(e) == P.VO_ERR_INVALID
    if det == "sift":
        loud = words.copy(); loud[3] = 255                    # |row|^2 = 128 * 255^2 > 2^20
        with pytest.raises(_lib.VoError) as e:
            fe.set_vocabulary(loud)
        assert _code(e) == P.VO_ERR_INVALID
    assert fe.vocabulary().tobytes() == before.tobytes() and len(fe.places_entries()["id"]) == 1


def test_the_other_allocations_are_left_alone(rig, oracle):
    """relocalize() results taken before an add and a query are what the same call returns afterwards; so is slam_map()."""
    det, fe = rig
    c = R.pose_case(det)
    (fe.set_sift_rows if det == "sift" else fe.set_orb_rows)(0, c["rows"], c["xy"])
    fe.stage_map(c["map_rows"], c["map_pts"])
    before = fe.relocalize([0], R.K)
    m_before = fe.map_matches(0)
    fe.train_vocabulary([0], K=256, iterations=2) if len(c["rows"]) >= 256 else fe.set_vocabulary(P.vocabulary_case(det, 256))
    fe.places_open(3)
    fe.places_add([0, 0], [1, 9])
    fe.places_query()
    m_after = fe.map_matches(0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m_before, m_after))
    rows, pts = fe.map_rows()
    assert rows.tobytes() == np.ascontiguousarray(c["map_rows"]).tobytes() and pts.tobytes() == np.ascontiguousarray(c["map_pts"]).tobytes()
    after = fe.relocalize([0], R.K)
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)
    assert len(fe.places_entries()["id"]) == 2                 # and relocalize left the index alone


def test_slam_map_and_a_configure_call(oracle):
    """slam_map() taken before an add and a query is unchanged afterwards, and a stream carried across them goes on as if they had
    not happened; a configure call releases the vocabulary and the index."""
    import ctypes as C
    import track_cases as TC
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    case = TC.cases()["tracks_births"]
    fr = TC.frames(oracle, case)
    opts = dict(ba_iterations=0, filter_threshold=1.0, max_cameras=4)
    fe = FrontEnd(64, 64, max_frames=5, max_pairs=4, nfeatures=case.nfeatures, nlevels=1)
    try:
        fe.ctx.set_poly_solver("opencv300")
        for k in range(5):
            fe.set_orb_rows(k, fr[k]["desc"], fr[k]["xy"])
        pairs = [[0, 1], [1, 2], [2, 3]]

        def stream(between):
            fe.run_pairs(pairs[:2], TC.K, fe.make_opts(want_points=True), want_points=True)
            first = fe.slam_stream(2, TC.K, total_pairs=3, **opts)
            held = fe.slam_map(0)
            between()
            assert all(held[k].tobytes() == fe.slam_map(0)[k].tobytes() for k in held)
            fe.run_pairs([[2, 3]], TC.K, fe.make_opts(want_points=True), want_points=True)
            out = fe.slam_stream(1, TC.K, resume=True, **opts)
            return first, out, fe.slam_map(0)

        def places():
            fe.set_vocabulary(P.vocabulary_case("orb", 256))
            assert len(fe.words(3)) == len(fr[3]["desc"])
            fe.places_open(5)
            fe.places_add([4, 0], [40, 0])
            fe.places_query(top_k=2)

        want = stream(lambda: None)
        got = stream(places)
        assert got[0]["status"].tolist() == [0, 0]
        for a, b in zip(want, got):
            assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
        assert len(fe.places_entries()["id"]) == 2             # and the stream left the index alone
        c = fe.ctx
        c.check(c.lib.vo_batch_configure(c.handle, fe.h, fe.w, C.addressof(fe.params), fe.max_frames, fe.max_pairs))
        for call in (fe.vocabulary, fe.places_entries, lambda: fe.words(4)):
            with pytest.raises(_lib.VoError) as e:
                call()
            assert _code(e) == P.VO_ERR_INVALID
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ arguments
def test_every_error_the_header_names(rig, oracle):
    from visual_odometry_amd import _lib
    det, fe = rig
    D = P.width(det)
    words = P.vocabulary_case(det, 256)

    def fails(code, fn, *a, **k):
        with pytest.raises((_lib.VoError, NotImplementedError)) as e:
            fn(*a, **k)
        if code == P.VO_ERR_UNSUPPORTED:
            assert e.type is NotImplementedError
        else:
            assert e.type is _lib.VoError and _code(e) == code, (fn, a, _code(e))

    _put(fe, det, 0, P.frame_case(det, words, 300))
    _put(fe, det, 1, P.frame_case(det, words, 17))
    # vocabulary
    for K in (0, 128, 255, 257, 384, 4096 + 256):
        fails(P.VO_ERR_INVALID, fe.train_vocabulary, [0], K=K)
        fails(P.VO_ERR_INVALID, fe.set_vocabulary, np.zeros((K, D), np.uint8))
    fails(P.VO_ERR_TOO_FEW, fe.train_vocabulary, [1], K=256)               # 17 rows
    fails(P.VO_ERR_TOO_FEW, fe.train_vocabulary, [0], K=512)               # 300 rows
    fails(P.VO_ERR_INVALID, fe.train_vocabulary, [], K=256)
    fails(P.VO_ERR_INVALID, fe.train_vocabulary, [5], K=256)
    fails(P.VO_ERR_INVALID, fe.train_vocabulary, [-1], K=256)
    fails(P.VO_ERR_INVALID, fe.train_vocabulary, [0] * 6, K=256)           # more slots than max_frames
    fe.set_vocabulary(words)
    fails(P.VO_ERR_INVALID, fe.words, 5)
    fails(P.VO_ERR_INVALID, fe.words, -1)
    # the index
    fails(P.VO_ERR_INVALID, fe.places_open, 0)
    fails(P.VO_ERR_INVALID, fe.places_open, 65537)
    fe.places_open(3)
    fails(P.VO_ERR_INVALID, fe.places_add, [5], [0])
    fe.places_add([0, 1], [0, 1])
    fails(P.VO_ERR_UNSUPPORTED, fe.places_add, [0, 1], [2, 3])             # one place left: nothing is added
    fails(P.VO_ERR_UNSUPPORTED, fe.places_add_histograms, np.zeros((2, 256), np.uint8), [2, 3])
    assert len(fe.places_entries()["id"]) == 2
    c = fe.ctx
    fails(P.VO_ERR_INVALID, lambda: c.check(c.lib.vo_places_entries(c.handle, 1, 2, None, None, None)))
    fails(P.VO_ERR_INVALID, lambda: c.check(c.lib.vo_places_entries(c.handle, -1, 1, None, None, None)))
    # the query
    for k in (0, 17, -1):
        fails(P.VO_ERR_INVALID, fe.places_query, top_k=k)
    fails(P.VO_ERR_INVALID, fe.places_query, [2])
    fails(P.VO_ERR_INVALID, fe.places_query, [-1])
    assert fe.places_query([]) ["entry"].shape == (0, 3)
    if det == "sift":                                          # a slot flagged for its descriptor norm
        _put(fe, det, 2, np.full((3, 128), 255, np.uint8))
        fails(P.VO_ERR_INVALID, fe.places_add, [2], [9])
        fails(P.VO_ERR_INVALID, fe.words, 2)
        fails(P.VO_ERR_INVALID, fe.train_vocabulary, [0, 2], K=256)
        _put(fe, det, 2, np.zeros((0, 128), np.uint8))


def test_before_a_vocabulary_and_before_a_configuration():
    from visual_odometry_amd import _lib
    ctx = _lib.Context(0)
    try:
        lib, h = ctx.lib, ctx.handle
        one = np.zeros(4, np.int32); words = np.zeros((256, 128), np.uint8)
        opts = _lib.PlacesOpts(3, 0, 0)
        import ctypes as C
        assert lib.vo_vocab_train(h, one.ctypes.data, 1, 256, 8, one.ctypes.data) == P.VO_ERR_NOT_CONFIGURED
        assert lib.vo_vocab_set(h, words.ctypes.data, 256) == P.VO_ERR_NOT_CONFIGURED
        assert lib.vo_vocab_words(h, 0, one.ctypes.data, 4, one.ctypes.data) == P.VO_ERR_NOT_CONFIGURED
        assert lib.vo_places_add(h, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data) == P.VO_ERR_NOT_CONFIGURED
        assert lib.vo_vocab_get(h, None, 0, one.ctypes.data) == P.VO_ERR_INVALID
        assert lib.vo_places_open(h, 4) == P.VO_ERR_INVALID                 # no vocabulary
        assert lib.vo_places_size(h, one.ctypes.data, one.ctypes.data) == P.VO_ERR_INVALID
        assert lib.vo_places_add_hist(h, words.ctypes.data, one.ctypes.data, 1, None) == P.VO_ERR_INVALID
        assert lib.vo_places_entries(h, 0, 0, None, None, None) == P.VO_ERR_INVALID
        assert lib.vo_places_query(h, one.ctypes.data, 1, C.addressof(opts), one.ctypes.data, one.ctypes.data) == P.VO_ERR_INVALID
    finally:
        ctx.close()

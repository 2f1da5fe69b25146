"""GPU: the batched Hamming matchers — k_nn_fp4 / k_nn_mfma / k_nn_pairs -> k_match_select, many pairs in one launch, the path bench.py
measures — on descriptor rows the test CHOSE (FrontEnd.set_orb_rows / vo_stage_orb_rows), against the numpy statement
tests/hamming_reference.py, which tests/test_hamming_reference.py holds equal to the oracle's C on the same cases, and every case
to what it is named for.  The kernels' claim is exactness: counts, indices and float32 distances are compared for equality, in all
four selection modes (nearest, legacy cross-check, strict mutual, knn2 + ratio) and under each of the three kernels.

Held here: uneven row counts side by side in one launch at the flagship capacity 2256 (0 .. 2256 = kp_cap rows: the remainders of
the 16-column group, the FP4 step, the wave, the B stages, the popcount tile and the 512-row block; a slot as query and as train;
a slot with itself; 35 and 40 workgroups; the pair list reversed); ties among train rows and among query rows at every level of the
kernels' reductions, all-equal sets, the ratio test exactly on its boundary; a slot that shrinks in place (the single pass's stale
column partials, stale desc rows, the operand image past the count); both sides of NN_COLS_MAX = 4096; the last admissible column
index of the FP4 and int8 accumulators (8183, 16127) and the first capacity of each silent fallback (8192, 16136); slots written
under different kernel settings; the seam itself against a real detection.

The frame is 64 x 64 with one pyramid level (the smallest tried; vo_batch_configure accepts it).  The geometry stage runs on whatever
matches come out (random points, 8 RANSAC iterations): its results are not looked at.
The whole file takes 2.3 - 3.0 s on an MI355X (measured; tests/test_gpu_match_l2i8.py on the same machine: 2.3 s), most of it the numpy
references: remainders under mfma_fp4 0.46 s (it builds the group's references), limit8184 0.33 s, every other test under 0.25 s."""
import numpy as np
import pytest

import hamming_reference as R

pytestmark = pytest.mark.gpu

H = W = 64
K = np.array([[60.0, 0, 32], [0, 60.0, 32], [0, 0, 1]])


def _mode_ids():
    from visual_odometry_amd import frontend as F
    return {"nearest": F.MATCH_NEAREST, "legacy": F.MATCH_CROSSCHECK_LEGACY, "mutual": F.MATCH_CROSSCHECK, "ratio": F.MATCH_RATIO}


def _front_end(nfeatures, max_frames, max_pairs, kernel):
    from visual_odometry_amd.frontend import FrontEnd
    fe = FrontEnd(H, W, max_frames=max_frames, max_pairs=max_pairs, nfeatures=nfeatures, nlevels=1)
    assert fe.kp_cap == R.kp_cap_for(nfeatures)
    fe.ctx.set_matcher_kernel(kernel)
    return fe


def _put(fe, slot, rows, seed=0):
    xy = np.random.default_rng(1000 + seed).uniform(1, W - 2, (len(rows), 2)).astype(np.float32)
    fe.set_orb_rows(slot, rows, xy)


def _run(fe, pairs, mode, ratio):
    opts = fe.make_opts(match_mode=_mode_ids()[mode], ratio=ratio, max_iters=8)
    res, _ = fe.run_pairs(pairs, K, opts)
    return res.copy()


def _same(fe, res, p, ref, mode, ratio, what):
    qi, ti, dd, _ = fe.pair_matches(p)
    wq, wt, wd = ref.select(mode, ratio)
    assert res["n_kp1"][p] == ref.nq and res["n_kp2"][p] == ref.nt, what
    assert res["n_match"][p] == len(wq) == len(qi), what
    assert np.array_equal(qi, wq) and np.array_equal(ti, wt), what
    assert dd.dtype == np.float32 and np.array_equal(dd, wd), what


def _launch_and_compare(fe, g, slot, launch, kernel):
    """Every mode of the group (ratio mode once per ratio) on one list of pairs: ONE run_pairs call holds them all."""
    pairs = [[slot[a], slot[b]] for a, b in launch]
    for mode in g.modes:
        for ratio in (g.ratios if mode == "ratio" else g.ratios[:1]):
            res = _run(fe, pairs, mode, ratio)
            for p, (a, b) in enumerate(launch):
                _same(fe, res, p, g.ref(a, b), mode, ratio, (g.name, kernel, a, b, mode, ratio, p))


@pytest.mark.parametrize("name, kernel", [(n, k) for n in R.GROUPS if n != "shrink" for k in R.kernels_of(n)])
def test_chosen_rows_match_the_numpy_statement(name, kernel):
    g = R.group(name)
    assert kernel in g.kernels
    if name.startswith("limit"):                            # the setter stays at mfma_fp4: the capacity alone picks the kernel
        assert R.kernel_for(kernel, g.kp_cap) == g.kernel
    slot = {k: i for i, k in enumerate(g.sets)}
    fe = _front_end(g.nfeatures, len(slot), max(len(l) for l in g.launches), kernel)
    try:
        assert fe.kp_cap == g.kp_cap
        for k, i in slot.items():
            _put(fe, i, g.sets[k], i)
        for launch in g.launches:
            _launch_and_compare(fe, g, slot, launch, kernel)
    finally:
        fe.ctx.close()


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_a_slot_that_shrinks_leaves_nothing_behind(kernel):
    """2256 rows, then 17, then none in ONE slot, as query and as train, the same pair indices every time.  The full frame's rows
    17.. are exact copies of the other slot's rows (tests/test_hamming_reference.py::test_stale_rows_would_change_the_answer): the
    FP4 single pass keeps their column partials of row blocks 1-4, ff.desc keeps the rows, the operand image is expanded anew."""
    g = R.group("shrink")
    fe = _front_end(g.nfeatures, 2, 2, kernel)
    try:
        slot = {"o2200": 0}
        _put(fe, 0, g.sets["o2200"])
        for step, launch in zip(R.SHRINK_STEPS, g.launches):
            _put(fe, 1, g.sets[step], 1)
            slot[step] = 1
            _launch_and_compare(fe, g, slot, launch, kernel)
            if step == "s0":
                res = _run(fe, [[1, 0], [0, 1]], "nearest", R.RATIO)
                assert list(res["n_match"]) == [0, 0] and res["n_kp1"][0] == 0 and res["n_kp2"][1] == 0
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ format: slots written under different kernel settings
def _oracle_or_refusal(fe, Kmat, pairs, want, what):
    """The oracle's list, or a refusal that names a slot of the pair — never a silent wrong list."""
    from visual_odometry_amd import _lib
    try:
        fe.run_pairs(pairs, Kmat, fe.make_opts(max_iters=8))
    except _lib.VoError as e:
        assert "slot" in str(e), what
        return
    for p, w in enumerate(want):
        qi, ti, dd, _ = fe.pair_matches(p)
        assert np.array_equal(qi, w[0]) and np.array_equal(ti, w[1]) and np.array_equal(dd, w[2]), (what, p)


@pytest.mark.parametrize("first, then", [("mfma_fp4", "mfma"), ("mfma", "mfma_fp4"), ("mfma_fp4", "popcount"), ("popcount", "mfma_fp4")])
def test_detecting_one_slot_after_a_kernel_switch(oracle, seq_small, first, then):
    """detect(0, 2) under one kernel, the setter, then detect(1, 1) ALONE: slot 0 still holds the first kernel's operand image.
    (tests/test_gpu_match.py::test_matcher_kernel_switch_after_detection_stays_consistent always detects both slots again.)"""
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    frames = seq_small["frames"]
    p = oracle.orb_params(nfeatures=500)
    d = [oracle.orb_detect_and_compute(frames[i], p)["desc"] for i in range(2)]
    want = [oracle.match_hamming(d[0], d[1], 2), oracle.match_hamming(d[1], d[0], 2)]
    c = _lib.Context(0)
    try:
        fe = FrontEnd(480, 640, max_frames=2, max_pairs=2, nfeatures=500, ctx=c)
        c.set_matcher_kernel(first)
        fe.upload(frames[:2]); fe.detect(0, 2)
        c.set_matcher_kernel(then)
        fe.detect(1, 1)
        _oracle_or_refusal(fe, seq_small["K"], [[0, 1], [1, 0]], want, (first, then))
        c.set_matcher_kernel(first)                         # and back, without a detection: the images stay what they are
        _oracle_or_refusal(fe, seq_small["K"], [[0, 1], [1, 0]], want, (first, then, "back"))
    finally:
        c.close()


@pytest.mark.parametrize("first, then", [(a, b) for a in R.KERNELS for b in R.KERNELS if a != b])
def test_rows_put_in_under_different_kernels(first, then):
    g = R.group("remainders")
    a, b = g.sets[513], g.sets[1025]
    fe = _front_end(g.nfeatures, 3, 3, first)
    try:
        _put(fe, 0, a); _put(fe, 2, g.sets[257], 2)
        fe.ctx.set_matcher_kernel(then)
        _put(fe, 1, b, 1)
        want = [g.ref(513, 1025).select("mutual"), g.ref(1025, 513).select("mutual"), g.ref(257, 513).select("mutual")]
        _oracle_or_refusal(fe, K, [[0, 1], [1, 0], [2, 0]], want, (first, then))
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ the seam
def test_seam_round_trip_and_argument_checks():
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    rng = np.random.default_rng(9108)
    rows = R.rand_rows(rng, 77)
    xy = rng.uniform(0, W, (77, 2)).astype(np.float32)
    fe = _front_end(8, 2, 1, "mfma_fp4")                    # kp_cap 264
    cap = fe.kp_cap
    assert cap == 264
    fe.set_orb_rows(0, rows, xy)
    f = fe.features(0)
    assert f["desc"].dtype == np.uint8 and np.array_equal(f["desc"], rows) and np.array_equal(f["xy"], xy) and not f["truncated"]
    for k in ("size", "angle", "response", "octave"):
        assert not f[k].any()
    fe.set_orb_rows(0, rows[:5])
    f = fe.features(0)
    assert np.array_equal(f["desc"], rows[:5]) and f["xy"].shape == (5, 2) and not f["xy"].any()
    fe.set_orb_rows(0, rows[:0])
    assert len(fe.features(0)["desc"]) == 0
    full = R.rand_rows(rng, cap)
    fe.set_orb_rows(1, full)                                # n == kp_cap
    f = fe.features(1)
    assert np.array_equal(f["desc"], full) and not f["truncated"]
    c = fe.ctx
    for slot, n in ((-1, 1), (2, 1), (0, cap + 1), (0, -1)):
        assert c.lib.vo_stage_orb_rows(c.handle, slot, rows.ctypes.data, n, None) == _lib.VO_ERR_INVALID
    assert c.lib.vo_stage_orb_rows(c.handle, 0, None, 1, None) == _lib.VO_ERR_INVALID
    assert c.lib.vo_stage_orb_rows(c.handle, 0, None, 0, None) == _lib.VO_OK
    assert np.array_equal(fe.features(1)["desc"], full)     # the refused calls changed nothing
    with pytest.raises(ValueError):
        fe.set_orb_rows(0, np.zeros((3, 128), np.uint8))
    bare = _lib.Context(0)
    assert bare.lib.vo_stage_orb_rows(bare.handle, 0, rows.ctypes.data, 1, None) == _lib.VO_ERR_NOT_CONFIGURED
    bare.close()
    sift = FrontEnd(32, 32, max_frames=1, max_pairs=1, detector="sift", kp_cap=256)
    assert sift.ctx.lib.vo_stage_orb_rows(sift.ctx.handle, 0, rows.ctypes.data, 1, None) == _lib.VO_ERR_NOT_CONFIGURED
    with pytest.raises(ValueError):
        sift.set_orb_rows(0, rows)
    sift.ctx.close(); c.close()


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_injected_rows_are_the_rows_the_descriptor_kernel_writes(seq_small, kernel):
    """One detected frame; its descriptors fed back into another slot through the seam: detected against injected is the identity
    pairing at distance 0, both ways round — the injected operand image is the one the detection writes."""
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    c = _lib.Context(0)
    try:
        c.set_matcher_kernel(kernel)
        fe = FrontEnd(480, 640, max_frames=2, max_pairs=2, nfeatures=500, ctx=c)
        fe.upload(seq_small["frames"][:1]); fe.detect(0, 1)
        f = fe.features(0)
        n = len(f["desc"])
        assert 300 < n <= fe.kp_cap and not f["truncated"]
        assert len(np.unique(f["desc"], axis=0)) == n
        fe.set_orb_rows(1, f["desc"], f["xy"])
        g = fe.features(1)
        assert np.array_equal(g["desc"], f["desc"]) and np.array_equal(g["xy"], f["xy"])
        fe.run_pairs([[0, 1], [1, 0]], seq_small["K"], fe.make_opts(max_iters=8))
        for p in range(2):
            qi, ti, dd, _ = fe.pair_matches(p)
            assert np.array_equal(qi, np.arange(n)) and np.array_equal(ti, np.arange(n)) and not dd.any()
    finally:
        c.close()

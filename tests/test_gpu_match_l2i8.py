"""GPU: k_nn_l2i8 + k_match_select on descriptor rows the test CHOSE (FrontEnd.set_sift_rows / vo_stage_sift_rows), against the numpy
statement tests/l2i8_reference.py — which tests/test_l2i8_reference.py holds equal to the oracle's C on the same cases, and every
case to what it is named for.  The kernel's claim is exactness: indices and float32 distances are compared for equality, in all
four selection modes (nearest, legacy cross-check, strict mutual, knn2 + ratio).

Held here: the remainders of the 16-column group, the 64 rows of a wave, the 128-row LDS stage and the 512-row workgroup with uneven
counts in one launch; the packed key on both sides of 4096 train rows (4095, 4096, 4097; packed forward with unpacked reverse;
winners in group 255 and 256; one row twice, the lower index wins); ties inside a lane, across lanes, across stages, first with
second neighbour; rows at the norm bound and the all-zero row; stale operand rows past the end of a frame; empty and one-row
frames; the norm-bound flag on the pair path; the seam itself against k_sb_descriptor's own output.

The geometry stage runs on whatever matches come out (random points of a 32 x 32 frame, 8 RANSAC iterations): its results are
not looked at.  The whole file takes 2.7 s on an MI355X (measured), 1.7 s of it the numpy references of the 4096-row pairs."""
import numpy as np
import pytest

import l2i8_reference as R
from conftest import random_image

pytestmark = pytest.mark.gpu

H = W = 32
K = np.array([[30.0, 0, 16], [0, 30.0, 16], [0, 0, 1]])


def _mode_ids():
    from visual_odometry_amd import frontend as F
    return {"nearest": F.MATCH_NEAREST, "legacy": F.MATCH_CROSSCHECK_LEGACY, "mutual": F.MATCH_CROSSCHECK, "ratio": F.MATCH_RATIO}


def _front_end(max_frames, max_pairs, kp_cap):
    from visual_odometry_amd.frontend import FrontEnd
    fe = FrontEnd(H, W, max_frames=max_frames, max_pairs=max_pairs, detector="sift", kp_cap=kp_cap)
    assert fe.kp_cap == kp_cap
    return fe


def _put(fe, slot, rows, seed=0):
    xy = np.random.default_rng(1000 + seed).uniform(1, W - 2, (len(rows), 2)).astype(np.float32)
    fe.set_sift_rows(slot, rows, xy)


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


@pytest.mark.parametrize("name", R.GROUPS)
def test_chosen_rows_match_the_numpy_statement(name):
    g = R.group(name)
    slot = {k: i for i, k in enumerate(g.sets)}
    fe = _front_end(len(slot), len(g.pairs), g.kp_cap)
    for k, i in slot.items():
        _put(fe, i, g.sets[k], i)
    pairs = [[slot[a], slot[b]] for a, b in g.pairs]
    for mode in R.MODES:
        res = _run(fe, pairs, mode, g.ratio)                # ONE launch for all the pairs of the group: uneven counts side by side
        for p, (a, b) in enumerate(g.pairs):
            _same(fe, res, p, g.ref(a, b), mode, g.ratio, (name, a, b, mode))


def test_knn2_puts_the_lowest_of_equal_columns_first():
    """Ratio mode at a ratio above 1 keeps the queries whose two neighbours tie at a distance > 0: the index shown is the knn2
    form's choice among equals (tests/test_l2i8_reference.py::test_ties_above_ratio_one_show_the_first_of_equals)."""
    g = R.group("ties")
    fe = _front_end(2, 1, g.kp_cap)
    _put(fe, 0, g.sets["q300"]); _put(fe, 1, g.sets["t280"], 1)
    res = _run(fe, [[0, 1]], "ratio", R.TIE_RATIO_ABOVE_ONE)
    _same(fe, res, 0, g.ref("q300", "t280"), "ratio", R.TIE_RATIO_ABOVE_ONE, "ties at ratio 1.5")


def test_stale_rows_past_the_end_are_never_read():
    """300 rows, then 17, then none in ONE slot: the operand image keeps the earlier frame's rows 17.., fifteen of which are exact
    copies of the queries (tests/test_l2i8_reference.py::test_stale_rows_would_change_the_answer)."""
    s = R.stale_case()
    fe = _front_end(2, 1, 512)
    _put(fe, 0, s["q"])
    for t in (s["t300"], s["t17"], s["t17"][:0]):
        _put(fe, 1, t, 1)
        ref = R.Pair(s["q"], t)
        for mode in R.MODES:
            res = _run(fe, [[0, 1]], mode, R.RATIO)
            _same(fe, res, 0, ref, mode, R.RATIO, (len(t), mode))
            if len(t) == 0:
                assert res["n_match"][0] == 0 and res["n_kp2"][0] == 0 and len(fe.pair_matches(0)[0]) == 0
    # and as the query side: no rows, no matches
    res = _run(fe, [[1, 0]], "nearest", R.RATIO)
    assert res["n_kp1"][0] == 0 and res["n_match"][0] == 0


def test_one_train_row():
    """nn_l2i8_body<true, false> with nb == 1 leaves a dead column (index >= nb) as the second neighbour; `nt < 2` in k_match_select
    keeps it from showing: ratio mode returns nothing, every other mode is the reference's."""
    g = R.group("one_train")
    fe = _front_end(2, 1, 256)
    _put(fe, 0, g.sets["q40"]); _put(fe, 1, g.sets["t1"], 1)
    res = _run(fe, [[0, 1]], "nearest", R.RATIO)
    qi, ti, dd, _ = fe.pair_matches(0)
    assert np.array_equal(qi, np.arange(40)) and (ti == 0).all()
    assert np.array_equal(dd, R.dist32(R.d2_matrix(g.sets["q40"], g.sets["t1"])[:, 0]))
    for ratio in (R.RATIO, 1.0, 1e30):                      # (whatever the ratio: a dead column's distance is never compared)
        res = _run(fe, [[0, 1]], "ratio", ratio)
        assert res["n_match"][0] == 0 and len(fe.pair_matches(0)[0]) == 0


def test_flagged_slot_is_not_matched_silently():
    from visual_odometry_amd import _lib
    rng = np.random.default_rng(8107)
    rows = R.sift_like(rng, 20)
    bad = rows.copy(); bad[7] = R.flagged_row()
    fe = _front_end(3, 2, 256)
    _put(fe, 0, rows); _put(fe, 1, bad, 1); _put(fe, 2, R.perturbed(rng, rows), 2)
    with pytest.raises(_lib.VoError) as e:
        fe.features(1)
    assert e.value.code == _lib.VO_ERR_INVALID and "norm bound" in str(e.value)
    for pairs in ([[0, 1]], [[1, 0]], [[0, 2], [2, 1]]):
        with pytest.raises(_lib.VoError) as e:
            _run(fe, pairs, "mutual", R.RATIO)
        assert e.value.code == _lib.VO_ERR_INVALID and "norm bound" in str(e.value) and "slot 1" in str(e.value)
    res = _run(fe, [[0, 2], [2, 0]], "mutual", R.RATIO)     # a pair list that avoids the slot runs clean
    _same(fe, res, 0, R.Pair(rows, fe.features(2)["desc"]), "mutual", R.RATIO, "clean")
    _put(fe, 1, rows, 1)                                    # the flag is recomputed with the slot
    assert np.array_equal(fe.features(1)["desc"], rows)
    _run(fe, [[0, 1]], "mutual", R.RATIO)


def test_seam_round_trip_and_argument_checks():
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    rng = np.random.default_rng(8108)
    rows = R.with_duplicates(rng, R.sift_like(rng, 77))
    xy = rng.uniform(0, W, (77, 2)).astype(np.float32)
    fe = _front_end(2, 1, 256)
    fe.set_sift_rows(0, rows, xy)
    f = fe.features(0)
    assert f["desc"].dtype == np.float32 and np.array_equal(f["desc"], rows) and np.array_equal(f["xy"], xy) and not f["truncated"]
    for k in ("size", "angle", "response", "octave"):
        assert not f[k].any()
    fe.set_sift_rows(0, rows[:5])
    f = fe.features(0)
    assert np.array_equal(f["desc"], rows[:5]) and not f["xy"].any()
    fe.set_sift_rows(0, rows[:0])
    assert len(fe.features(0)["desc"]) == 0
    fe.set_sift_rows(1, np.zeros((256, 128), np.uint8))      # n == kp_cap
    c = fe.ctx
    for slot, n in ((-1, 1), (2, 1), (0, 257), (0, -1)):
        assert c.lib.vo_stage_sift_rows(c.handle, slot, rows.ctypes.data, n, None) == _lib.VO_ERR_INVALID
    assert c.lib.vo_stage_sift_rows(c.handle, 0, None, 1, None) == _lib.VO_ERR_INVALID
    orb = FrontEnd(480, 640, max_frames=1, max_pairs=1)
    assert orb.ctx.lib.vo_stage_sift_rows(orb.ctx.handle, 0, rows.ctypes.data, 1, None) == _lib.VO_ERR_NOT_CONFIGURED
    with pytest.raises(ValueError):
        orb.set_sift_rows(0, rows)


def test_injected_rows_are_the_rows_the_descriptor_kernel_writes():
    """One detected frame; its descriptors fed back into another slot through the seam: detected against injected is the identity
    pairing at distance 0 — the injected operand image and norms are the ones k_sb_descriptor wrote."""
    from visual_odometry_amd.frontend import FrontEnd
    h, w = 96, 128
    fe = FrontEnd(h, w, max_frames=2, max_pairs=2, detector="sift", kp_cap=512)
    fe.upload(random_image(11, h, w)[None]); fe.detect(0, 1)
    f = fe.features(0)
    n = len(f["desc"])
    assert 40 < n <= 512 and not f["truncated"]
    rows = f["desc"].astype(np.uint8)
    assert len(np.unique(rows, axis=0)) == n
    fe.set_sift_rows(1, rows, f["xy"])
    Kc = np.array([[100.0, 0, w / 2], [0, 100.0, h / 2], [0, 0, 1]])
    res, _ = fe.run_pairs([[0, 1], [1, 0]], Kc, fe.make_opts(max_iters=8))
    for p in range(2):
        qi, ti, dd, _ = fe.pair_matches(p)
        assert np.array_equal(qi, np.arange(n)) and np.array_equal(ti, np.arange(n)) and not dd.any()

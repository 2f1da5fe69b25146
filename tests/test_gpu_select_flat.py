"""GPU parity of the flat walk of k_sel_rows and of the index map k_cv2_order reads instead of searching: a wavefront loads the
tile counts of its row of FAST tiles at once, walks the row's winners as one list, keeps the first 256 in registers between the
bitmap pass and the write pass and reads the rest a second time; in cv2 order it leaves every kept winner's place in the
candidate list at its place in the all-winner list.  The yardstick is the CPU oracle alone: every frame's regime (winners per
tile and per tile row, thresholds, capacities) is computed from the oracle's pyramid and FAST + NMS map BEFORE anything runs on
the device and asserted, then FrontEnd.features() is compared with the oracle field for field in both keypoint orders."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE, FAST_TW, FAST_TH, FOX, FOY = 31, 112, 20, 16, 31     # FAST tiles of 112 x 20 pixels from (16, 31)
HELD = 256                                                   # winners of a tile row a wavefront keeps in registers (4 per lane)
KEYS = ("xy", "octave", "response", "angle", "size", "desc")


def level_stats(oracle, img, p):
    """Per level, from the oracle's pyramid and FAST + NMS score map: listed winners inside the border, retainBest's n, the n-th
    largest score T (1 when fewer than n are listed: keep all), how many reach T, and the winners per FAST tile [rows, tiles]."""
    _, _, _, quota = oracle.level_geometry(img.shape[0], img.shape[1], p)
    out = []
    for l, lvl in enumerate(oracle.pyramid(img, p)):
        h, w = lvl.shape
        want = 2 * int(quota[l])
        if w <= 2 * EDGE or h <= 2 * EDGE:
            out.append(dict(n=0, want=want, T=256, kept=0, px=w * h, tiles=np.zeros((0, 0), int))); continue
        s = oracle.fast_score_nms(lvl, p.fast_threshold).astype(int)
        s[:EDGE] = 0; s[h - EDGE:] = 0; s[:, :EDGE] = 0; s[:, w - EDGE:] = 0
        ys, xs = np.nonzero(s)
        rows, cols = -(-(h - EDGE - FOY) // FAST_TH), -(-(w - EDGE - FOX) // FAST_TW)
        tiles = np.zeros((rows, cols), int)
        np.add.at(tiles, ((ys - FOY) // FAST_TH, (xs - FOX) // FAST_TW), 1)
        sc = np.sort(s[ys, xs])[::-1]
        T = int(sc[want - 1]) if 0 < want <= len(sc) else 1
        out.append(dict(n=len(sc), want=want, T=T, kept=int((sc >= T).sum()), px=w * h, tiles=tiles))
    return out


def capacities(s):
    """candidate lists 2 quota + max(2 quota, 1024) per level, all-winner lists px / 8 + 1024 per level."""
    return s["want"] + max(s["want"], 1024), s["px"] // 8 + 1024


def assert_within_capacities(stats, n_keypoints, nfeatures):
    for s in stats:
        cand, listed = capacities(s)
        assert s["kept"] <= cand and s["n"] <= listed, {k: v for k, v in s.items() if k != "tiles"}
    assert n_keypoints <= nfeatures + max(nfeatures // 8, 256)


_REFERENCES = {}


def oracle_both_orders(oracle, img, p):
    """The oracle's features in both keypoint orders; computed once per frame and settings, shared by the tests, never changed."""
    key = (img.shape, img.tobytes(), p.nfeatures, p.nlevels)
    if key not in _REFERENCES:
        _REFERENCES[key] = _oracle_both_orders(oracle, img, p)
    return _REFERENCES[key]


def _oracle_both_orders(oracle, img, p):
    ref = oracle.orb_detect_and_compute(img, p)
    oracle.set_keypoint_order("canonical")
    try:
        canon = oracle.orb_detect_and_compute(img, p)
    finally:
        oracle.set_keypoint_order("cv2")
    assert not ref["overflow"] and not canon["overflow"]
    return {"cv2": ref, "canonical": canon}


def assert_equals_oracle(got, want, order, tag):
    assert not got["truncated"], (tag, order)
    for k in KEYS:
        assert np.array_equal(got[k], want[order][k]), (tag, order, k)


def detect_in_both_orders(batches, nfeatures, nlevels, tag):
    """batches: lists of (frame, the oracle's features or None) detected one after the other from slot 0 by the same FrontEnd,
    each list in one launch.  None: the frame must come back flagged as truncated."""
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    h, w = batches[0][0][0].shape
    c = _lib.Context(0)
    try:
        for order in ("cv2", "canonical"):
            fe = FrontEnd(h, w, max_frames=max(len(b) for b in batches), max_pairs=1, nfeatures=nfeatures, nlevels=nlevels, ctx=c,
                          keypoint_order=order)
            for k, batch in enumerate(batches):
                fe.upload(np.stack([f for f, _ in batch]))
                fe.detect(0, len(batch))
                for i, (_, want) in enumerate(batch):
                    if want is None:
                        assert fe.features(i)["truncated"], (tag, order, k, i)
                    else:
                        assert_equals_oracle(fe.features(i), want, order, (tag, k, i))
    finally:
        c.close()


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def half_flat_frame():
    """Noise in two column bands and below row 120 of them only; the rest is flat: tile rows without a winner, and tile rows whose
    full tiles have empty ones between them."""
    img = np.full((240, 1300), 90, np.uint8)
    n = noise(9, 240, 1300)
    for x0, x1 in ((140, 350), (600, 1010)):
        img[120:, x0:x1] = n[120:, x0:x1]
    return img


def dots_frame():
    """9000 single bright pixels on a flat frame: each one that stands alone is a FAST winner with the same score, so a level
    keeps every one of them."""
    rng = np.random.default_rng(7)
    img = np.full((240, 1300), 60, np.uint8)
    img[rng.integers(0, 240, 9000), rng.integers(0, 1300, 9000)] = 255
    return img


def test_rows_far_past_the_register_cache(oracle):
    """Uniform noise, 1300 x 240: level 0 is 12 tiles wide, its tile rows list thousands of winners (the second loop that reads the
    lists again) and single tiles list more than a wave trip."""
    img, p = noise(5, 240, 1300), oracle.orb_params(nfeatures=2000, nlevels=3)
    stats = level_stats(oracle, img, p)
    t0 = stats[0]["tiles"]
    assert t0.shape[1] == 12 and t0.sum(axis=1).max() > 8 * HELD and t0.max() > 3 * 64, (t0.sum(axis=1), t0.max())
    want = oracle_both_orders(oracle, img, p)
    assert_within_capacities(stats, len(want["cv2"]["xy"]), 2000)
    detect_in_both_orders([[(img, want)]], 2000, 3, "noise")


def test_levels_one_and_two_tiles_wide(oracle):
    """Uniform noise, 170 x 120, four levels: levels of two tiles and of one tile in a row, and levels that list fewer winners than
    retainBest's n (threshold 1)."""
    img, p = noise(5, 120, 170), oracle.orb_params(nfeatures=300, nlevels=4)
    stats = level_stats(oracle, img, p)
    widths = [s["tiles"].shape[1] for s in stats]
    assert 1 in widths and 2 in widths, widths
    assert sum(0 < s["n"] < s["want"] and s["T"] == 1 for s in stats) >= 2, [(s["n"], s["want"], s["T"]) for s in stats]
    want = oracle_both_orders(oracle, img, p)
    assert_within_capacities(stats, len(want["cv2"]["xy"]), 300)
    detect_in_both_orders([[(img, want)]], 300, 4, "small noise")


def test_empty_tiles_and_empty_rows_among_dense_ones(oracle):
    """Half flat, half noise: tile rows without any winner, tile rows with empty tiles between full ones and rows past the register
    cache in one launch."""
    img, p = half_flat_frame(), oracle.orb_params(nfeatures=2000, nlevels=3)
    stats = level_stats(oracle, img, p)
    t0 = stats[0]["tiles"]
    rows = t0.sum(axis=1)
    assert (rows == 0).any() and (rows > HELD).any(), rows
    gaps = [r for r in t0 if any(r[i] == 0 and r[:i].any() and r[i + 1:].any() for i in range(len(r)))]
    assert len(gaps) >= 2, t0
    want = oracle_both_orders(oracle, img, p)
    assert_within_capacities(stats, len(want["cv2"]["xy"]), 2000)
    detect_in_both_orders([[(img, want)]], 2000, 3, "half flat")


def test_rows_that_stay_in_registers(oracle):
    """conftest.random_image at a width whose tile rows list at most 256 winners (it is several times as corner-dense as the
    benchmark's frames: 1466 in a row at 1280 pixels), up to all four entries of every lane: the lists are read once."""
    from conftest import random_image
    img, p = random_image(11, 200, 256), oracle.orb_params(nfeatures=500, nlevels=8)
    stats = level_stats(oracle, img, p)
    most = max(int(s["tiles"].sum(axis=1).max()) for s in stats if s["tiles"].size)
    assert 3 * 64 < most <= HELD, most
    want = oracle_both_orders(oracle, img, p)
    assert_within_capacities(stats, len(want["cv2"]["xy"]), 500)
    detect_in_both_orders([[(img, want)]], 500, 8, "rows in registers")


def test_flagship_frame_stays_in_registers(oracle):
    """A frame of the benchmark's synthetic sequence at its size and settings: 12 tiles in a row at level 0 and no tile row of any
    level past the 256 winners a wavefront keeps."""
    from visual_odometry_amd import synth
    img, p = synth.sequence(1, 1280, 720)["frames"][0], oracle.orb_params(nfeatures=2000, nlevels=8)
    stats = level_stats(oracle, img, p)
    assert stats[0]["tiles"].shape[1] == 12
    most = max(int(s["tiles"].sum(axis=1).max()) for s in stats)
    assert 64 < most <= HELD, most
    want = oracle_both_orders(oracle, img, p)
    assert_within_capacities(stats, len(want["cv2"]["xy"]), 2000)
    detect_in_both_orders([[(img, want)]], 2000, 8, "flagship")


@pytest.mark.filterwarnings("ignore:a frame's keypoint list hit its capacity")
def test_overflow_is_flagged_and_stays_inside_its_lists(oracle):
    """9000 bright dots: level 0 keeps more winners than its candidate list holds.  The slot is flagged, and an ordinary frame in
    the next slot of the same launch still equals the oracle: nothing was written past a list."""
    dots, img, p = dots_frame(), noise(5, 240, 1300), oracle.orb_params(nfeatures=2000, nlevels=3)
    s0 = level_stats(oracle, dots, p)[0]
    assert s0["kept"] > capacities(s0)[0] and s0["n"] <= capacities(s0)[1], (s0["kept"], s0["n"], capacities(s0))
    want = oracle_both_orders(oracle, img, p)
    detect_in_both_orders([[(dots, None), (img, want)]], 2000, 3, "overflow")


def test_second_frame_in_a_slot_ignores_the_first_ones_map(oracle):
    """Two different frames detected one after the other in the same slot: the second equals the oracle although the index map
    still holds the entries of the first."""
    a, b, p = noise(5, 240, 1300), half_flat_frame(), oracle.orb_params(nfeatures=2000, nlevels=3)
    wa, wb = oracle_both_orders(oracle, a, p), oracle_both_orders(oracle, b, p)
    assert not np.array_equal(wa["cv2"]["xy"][:100], wb["cv2"]["xy"][:100])
    detect_in_both_orders([[(a, wa)], [(b, wb)], [(a, wa)]], 2000, 3, "same slot")

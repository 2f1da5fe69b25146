"""GPU parity of the fused FAST selection: one count launch and one emit launch of k_sel_rows produce the kept candidate list
and, in cv2 keypoint order, the list of all listed winners.  The yardstick is the CPU oracle alone: the frames are chosen from
the oracle's per-level winner counts BEFORE anything runs on the device, and the regimes they are meant to hit (threshold 1:
kept list == all-winner list; many winners tied at the n-th largest score; detections at a slot offset) are asserted from
those counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, NFEATURES, NLEVELS, EDGE = 480, 640, 1000, 8, 31
KEYS = ("xy", "octave", "response", "angle", "size", "desc")


def low_texture_frame():
    """60 flat bright squares on a flat background: a few hundred FAST winners in the whole pyramid."""
    rng = np.random.default_rng(3)
    img = np.full((H, W), 90, np.uint8)
    for _ in range(60):
        s = int(rng.integers(6, 30)); y = int(rng.integers(0, H - s)); x = int(rng.integers(0, W - s))
        img[y:y + s, x:x + s] = int(rng.integers(130, 256))
    return img


def tie_frame():
    """A lattice of identical 12 x 12 squares, pitch 32: the corners of a level all score the same."""
    img = np.full((H, W), 60, np.uint8)
    for y in range(40, H - 47, 32):
        for x in range(40, W - 47, 32):
            img[y:y + 12, x:x + 12] = 200
    return img


def level_stats(oracle, img, p):
    """Per level, from the oracle's pyramid and FAST + NMS score map: listed winners inside the border, retainBest's n, the n-th
    largest score T (1 when fewer than n are listed: keep all), how many reach T and how many equal it."""
    _, _, _, quota = oracle.level_geometry(img.shape[0], img.shape[1], p)
    out = []
    for l, lvl in enumerate(oracle.pyramid(img, p)):
        h, w = lvl.shape
        want = 2 * int(quota[l])
        if w <= 2 * EDGE or h <= 2 * EDGE:
            out.append(dict(n=0, want=want, T=256, kept=0, ties=0, px=w * h)); continue
        s = oracle.fast_score_nms(lvl, p.fast_threshold)[EDGE:h - EDGE, EDGE:w - EDGE]
        sc = np.sort(s[s > 0].astype(int))[::-1]
        T = int(sc[want - 1]) if 0 < want <= len(sc) else 1
        out.append(dict(n=len(sc), want=want, T=T, kept=int((sc >= T).sum()), ties=int((sc == T).sum()), px=w * h))
    return out


def assert_within_capacities(stats, n_keypoints):
    """candidate lists 2 quota + max(2 quota, 1024) per level, all-winner lists px / 8 + 1024 per level,
    keypoint lists nfeatures + max(nfeatures / 8, 256)."""
    for s in stats:
        assert s["kept"] <= s["want"] + max(s["want"], 1024), s
        assert s["n"] <= s["px"] // 8 + 1024, s
    assert n_keypoints <= NFEATURES + max(NFEATURES // 8, 256)


def oracle_both_orders(oracle, img, p):
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
    if order == "canonical":                      # the oracle's cv2-order SET, sorted by (octave, y, x), is this list
        ref = want["cv2"]
        idx = np.lexsort((ref["xy"][:, 0], ref["xy"][:, 1], ref["octave"]))
        assert np.array_equal(got["xy"], ref["xy"][idx]) and np.array_equal(got["desc"], ref["desc"][idx]), (tag, order)


def detect_in_both_orders(oracle, frames, wants, first_slots, tag):
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    F, c = len(frames), _lib.Context(0)
    try:
        for order in ("cv2", "canonical"):
            fe = FrontEnd(H, W, max_frames=max(first_slots) + F, max_pairs=1, nfeatures=NFEATURES, nlevels=NLEVELS, ctx=c,
                          keypoint_order=order)
            for s in first_slots:
                fe.upload(np.stack(frames), first_slot=s)
                fe.detect(s, F)
                for i in range(F):
                    assert_equals_oracle(fe.features(s + i), wants[i], order, (tag, s, i))
    finally:
        c.close()


def test_kept_list_equals_all_winner_list(oracle):
    """Low texture: the levels list fewer winners than retainBest's n, the threshold is 1 and both lists hold the same entries."""
    img, p = low_texture_frame(), oracle.orb_params(nfeatures=NFEATURES, nlevels=NLEVELS)
    stats = level_stats(oracle, img, p)
    assert sum(0 < s["n"] < s["want"] and s["T"] == 1 and s["kept"] == s["n"] for s in stats) >= 2, stats
    want = oracle_both_orders(oracle, img, p)
    assert_within_capacities(stats, len(want["cv2"]["xy"]))
    assert len(want["cv2"]["xy"]) > 100
    detect_in_both_orders(oracle, [img], [want], [0], "low texture")


def test_heavy_ties_at_the_nth_largest_score(oracle):
    """Identical corners: hundreds of winners share the n-th largest score of a level (retainBest keeps every one of them), and the
    other levels have smaller tie groups at theirs."""
    img, p = tie_frame(), oracle.orb_params(nfeatures=NFEATURES, nlevels=NLEVELS)
    stats = level_stats(oracle, img, p)
    assert max(s["ties"] for s in stats if s["n"] > s["want"]) >= 200, stats
    assert sum(s["n"] > s["want"] and s["ties"] >= 10 and s["kept"] > s["want"] for s in stats) >= 3, stats
    want = oracle_both_orders(oracle, img, p)
    assert_within_capacities(stats, len(want["cv2"]["xy"]))
    detect_in_both_orders(oracle, [img], [want], [0], "ties")


def test_detection_at_a_slot_offset(oracle):
    """The same three frames at slots [0, 3) and at slots [2, 5): every per-slot offset into the selection's arrays (thresholds,
    tile-row counts of both lists, all-winner lists, flags) is exercised, and both runs equal the oracle."""
    from conftest import random_image
    frames = [low_texture_frame(), tie_frame(), random_image(11, H, W)]
    p = oracle.orb_params(nfeatures=NFEATURES, nlevels=NLEVELS)
    wants = [oracle_both_orders(oracle, f, p) for f in frames]
    for f, w in zip(frames, wants):
        assert_within_capacities(level_stats(oracle, f, p), len(w["cv2"]["xy"]))
    detect_in_both_orders(oracle, frames, wants, [0, 2], "slot offset")

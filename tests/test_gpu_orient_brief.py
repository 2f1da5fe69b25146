"""GPU parity of k_brief, which computes a keypoint's orientation (ICAngles + fastAtan2) and its steered BRIEF descriptor in one
pass: the raw 31 x 31 patch and the blurred 37-row window are fetched together as aligned 16-byte chunks, the moments meet in the
first wavefront of the workgroup, and the descriptor is gathered from LDS.  The yardstick is the CPU oracle alone; `angle`, `desc`,
`xy`, `size` are compared for equality.  Every frame is chosen from the oracle's output BEFORE anything runs on the device, and
what a frame is meant to reach is asserted on that output:

- pyramids whose top level is 64 - 80 pixels on its smaller side (68 and 72 here), every level holding keypoints, some of them exactly 31 pixels from
  each of the four borders of their level (the chunk and row clamps of both windows);
- keypoint counts of 1 and of 15 modulo 16 (one keypoint past / one short of a workgroup's share, whether a wavefront takes two
  keypoints or four) next to a frame with none, in one launch, in both keypoint orders;
- a slot that is detected dense, then sparse, then empty;
- the three operand images of the matcher;
- angles in all eight octants: the four quadrants times both branches of fastAtan2.

All frames are 150 x 420 at five levels or 243 x 331 at eight; the oracle needs 25 - 40 ms per frame."""
import numpy as np
import pytest

from conftest import random_image

pytestmark = pytest.mark.gpu

H, W, NLEVELS, NFEATURES, EDGE = 150, 420, 5, 300, 31
KEYS = ("angle", "desc", "xy", "size", "octave", "response")
KMAT = np.array([[300.0, 0, W / 2], [0, 300.0, H / 2], [0, 0, 1]])
KERNELS = ("mfma_fp4", "mfma", "popcount")


def squares_frame(seed, n, h=H, w=W):
    """n flat bright squares on a flat background: fewer corners than nfeatures, so the count is the frame's own."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 90, np.uint8)
    for _ in range(n):
        s = int(rng.integers(6, 30)); y = int(rng.integers(0, h - s)); x = int(rng.integers(0, w - s))
        img[y:y + s, x:x + s] = int(rng.integers(130, 256))
    return img


def both_orders(oracle, img, p):
    ref = oracle.orb_detect_and_compute(img, p)
    oracle.set_keypoint_order("canonical")
    try:
        canon = oracle.orb_detect_and_compute(img, p)
    finally:
        oracle.set_keypoint_order("cv2")
    assert not ref["overflow"] and not canon["overflow"]
    return {"cv2": ref, "canonical": canon}


@pytest.fixture(scope="module")
def frames(oracle):
    """name -> (image, the oracle's features in both orders); computed once, never changed."""
    p = oracle.orb_params(nfeatures=NFEATURES, nlevels=NLEVELS)
    imgs = {"one_past": squares_frame(4, 30), "one_short": squares_frame(0, 20), "flat": np.full((H, W), 128, np.uint8),
            "dense": random_image(0, H, W), "sparse": squares_frame(2, 12)}
    out = {k: (v, both_orders(oracle, v, p)) for k, v in imgs.items()}
    n = {k: len(v[1]["cv2"]["xy"]) for k, v in out.items()}
    assert n["one_past"] % 16 == 1 and n["one_past"] > 16, n
    assert n["one_short"] % 16 == 15 and n["one_short"] > 16, n
    assert n["flat"] == 0 and n["dense"] == NFEATURES and 16 < n["sparse"] < n["dense"] // 2, n
    return out


def front_end(h, w, slots, pairs, nfeatures, nlevels, order="cv2", kernel=None):
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    c = _lib.Context(0)
    if kernel:
        c.set_matcher_kernel(kernel)
    return FrontEnd(h, w, max_frames=slots, max_pairs=pairs, nfeatures=nfeatures, nlevels=nlevels, ctx=c, keypoint_order=order)


def assert_features(got, want, tag):
    assert not got["truncated"], tag
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (tag, k)


def assert_matches(oracle, fe, pairs, desc, tag):
    """pair_matches of every pair against the oracle's cross-checked list on the oracle's descriptors."""
    res, _ = fe.run_pairs(pairs, KMAT, fe.make_opts(max_iters=8))
    n_match = res["n_match"].copy()
    for i, (a, b) in enumerate(pairs):
        wq, wt, wd = oracle.match_hamming(desc[a], desc[b], 2)
        qi, ti, dd, _ = fe.pair_matches(i)
        assert n_match[i] == len(wq), (tag, i)
        assert np.array_equal(qi, wq) and np.array_equal(ti, wt) and np.array_equal(dd, wd), (tag, i)


# ------------------------------------------------------------------ window clamps
@pytest.mark.parametrize("h, w, nlevels", [(243, 331, 8), (150, 420, 5)])
def test_small_top_levels_and_keypoints_on_the_border_band(oracle, h, w, nlevels):
    p = oracle.orb_params(nfeatures=500, nlevels=nlevels)
    img = random_image(0, h, w)
    ref = oracle.orb_detect_and_compute(img, p)
    lw, lh, ls, _ = oracle.level_geometry(h, w, p)
    assert 64 <= min(lw[-1], lh[-1]) <= 80 and max(lw[-1], lh[-1]) > 2 * EDGE, (lw, lh)
    o = ref["octave"]
    assert set(o.tolist()) == set(range(nlevels))
    x = np.rint(ref["xy"][:, 0] / ls[o]).astype(int); y = np.rint(ref["xy"][:, 1] / ls[o]).astype(int)
    assert x.min() >= EDGE and y.min() >= EDGE and (x <= lw[o] - 1 - EDGE).all() and (y <= lh[o] - 1 - EDGE).all()
    assert (x == EDGE).any() and (y == EDGE).any() and (x == lw[o] - 1 - EDGE).any() and (y == lh[o] - 1 - EDGE).any()
    top = o == nlevels - 1
    assert top.sum() >= 10
    fe = front_end(h, w, 1, 1, 500, nlevels)
    try:
        fe.upload(img[None]); fe.detect(0, 1)
        assert_features(fe.features(0), ref, (h, w))
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ partial workgroups, one launch
@pytest.mark.parametrize("order", ["cv2", "canonical"])
def test_counts_around_a_workgroups_share_and_an_empty_frame(frames, order):
    names = ("one_past", "one_short", "flat")
    fe = front_end(H, W, 3, 1, NFEATURES, NLEVELS, order)
    try:
        fe.upload(np.stack([frames[k][0] for k in names])); fe.detect(0, 3)
        for s, k in enumerate(names):
            assert_features(fe.features(s), frames[k][1][order], (order, k))
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ stale state
def test_a_slot_detected_dense_then_sparse_then_empty(oracle, frames):
    """Slot 1 shrinks in place; slot 0 keeps one frame.  After every detection the slot's features are the oracle's and the match
    lists of (1, 0) and (0, 1) are the oracle's on the oracle's descriptors: kp_angle, desc and the operand image past the new
    count are not read."""
    fe = front_end(H, W, 2, 2, NFEATURES, NLEVELS)
    try:
        fe.upload(frames["one_short"][0][None], first_slot=0); fe.detect(0, 1)
        d0 = frames["one_short"][1]["cv2"]["desc"]
        for k in ("dense", "sparse", "flat"):
            fe.upload(frames[k][0][None], first_slot=1); fe.detect(1, 1)
            want = frames[k][1]["cv2"]
            assert_features(fe.features(1), want, k)
            assert_features(fe.features(0), frames["one_short"][1]["cv2"], (k, "slot 0"))
            assert_matches(oracle, fe, [[1, 0], [0, 1]], {0: d0, 1: want["desc"]}, k)
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ every operand image
@pytest.mark.parametrize("kernel", KERNELS)
def test_three_slots_under_every_matcher_kernel(oracle, frames, kernel):
    names = ("one_past", "one_short", "flat")
    fe = front_end(H, W, 3, 4, NFEATURES, NLEVELS, kernel=kernel)
    try:
        fe.upload(np.stack([frames[k][0] for k in names])); fe.detect(0, 3)
        desc = {}
        for s, k in enumerate(names):
            assert_features(fe.features(s), frames[k][1]["cv2"], (kernel, k))
            desc[s] = frames[k][1]["cv2"]["desc"]
        assert_matches(oracle, fe, [[0, 1], [1, 0], [0, 2], [2, 1]], desc, kernel)
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ fastAtan2
def test_angles_in_every_octant(frames):
    """Quadrants decide the two reflections of fastAtan2, the octant inside a quadrant its |x| >= |y| branch."""
    img, want = frames["dense"]
    octants = np.bincount((want["cv2"]["angle"] // 45).astype(int), minlength=8)
    assert len(octants) == 8 and octants.min() >= 10, octants
    fe = front_end(H, W, 1, 1, NFEATURES, NLEVELS)
    try:
        fe.upload(img[None]); fe.detect(0, 1)
        assert_features(fe.features(0), want["cv2"], "octants")
    finally:
        fe.ctx.close()

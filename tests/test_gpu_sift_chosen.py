"""The SIFT kernels of sift_batch.hip on scenes CHOSEN for the branches the whole-detector tests never reach
(tests/sift_cases.py; tests/test_sift_cases_reference.py proves from the oracle's path census that each scene reaches its
branch): k_sb_extrema<3 / 8 / 9 / 10>, the run-time sweep at 3, 5, 57 and 63 taps and the refusal at 69, k_sb_descriptor's second
chunk of window rows and clipped radii, k_sb_orient's windows wider than a wavefront, the clamped last bucket of k_sb_bucket /
k_sb_rank, strip and segment seams of the extrema search, every exit of the refinement, cut windows, multiple peaks.

Every case goes through both doors — SiftDetector.detect_arrays (vo_sift_detect_and_compute) and FrontEnd(detector="sift")
(vo_frames_detect) — and position, size, angle, response, packed octave and descriptors equal
oracle.sift_detect_and_compute's byte for byte."""
import itertools

import numpy as np
import pytest

import sift_cases as S
from conftest import random_image

pytestmark = pytest.mark.gpu

KEYS = ("xy", "size", "angle", "response", "octave", "desc")
SUPPORTED = [c.name for c in S.CASES if not c.unsupported]


def _same_features(got, want, tag):
    assert not got["truncated"], tag
    assert len(got["xy"]) == want["n_found"] == len(want["xy"]), tag
    assert got["desc"].dtype == np.float32
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (tag, k)


@pytest.mark.parametrize("name", SUPPORTED)
def test_per_image_call_on_chosen_scene(oracle, ctx, name):
    from visual_odometry_amd.detector import SiftDetector
    c = S.BY_NAME[name]
    want = S.expected(oracle, c)
    assert want["n_found"] >= 1
    _same_features(SiftDetector(ctx=ctx, **c.params).detect_arrays(c.img), want, name)


def _slot_orders(n):
    """Two orders of n different frames, one after the other (2 n slots), in which no frame has the same set of neighbours twice."""
    first = list(range(n))
    for second in itertools.permutations(range(n)):
        slots = first + list(second)
        nb = lambda i: {slots[j] for j in (i - 1, i + 1) if 0 <= j < 2 * n}
        if all(nb(slots.index(f)) != nb(n + list(second).index(f)) for f in range(n)):
            return slots
    raise AssertionError(n)


def _batch(oracle, names):
    """(frames, expected results, parameters): the batch's cases, then random_image frames up to three different frames."""
    cases = [S.BY_NAME[n] for n in names]
    assert len({c.batch_key for c in cases}) == 1
    h, w = cases[0].img.shape
    prm = cases[0].params
    frames = [c.img for c in cases]
    wants = [S.expected(oracle, c) for c in cases]
    while len(frames) < 3:
        frames.append(random_image(900 + len(frames), h, w))
        wants.append(oracle.sift_detect_and_compute(frames[-1], **S.oracle_kw(prm)))
    return frames, wants, prm


@pytest.mark.parametrize("names", S.BATCHES, ids="+".join)
def test_batched_path_on_chosen_scenes(oracle, names):
    from visual_odometry_amd import frontend as F
    frames, wants, prm = _batch(oracle, names)
    h, w = frames[0].shape
    n = len(frames)
    slots = _slot_orders(n)
    fe = F.FrontEnd(h, w, max_frames=2 * n, max_pairs=1, detector="sift", kp_cap=S.KP_CAP.get(names[0], 4096), **prm)
    assert max(x["n_found"] for x in wants) < fe.kp_cap
    # one call: every frame sits in two slots, with other neighbours
    fe.upload(np.stack([frames[i] for i in slots]))
    fe.detect(0, 2 * n)
    for s, i in enumerate(slots):
        _same_features(fe.features(s), wants[i], (names, "one call", s))
    # the frames moved on by one slot, detected in two calls
    moved = slots[1:] + slots[:1]
    fe.upload(np.stack([frames[i] for i in moved]))
    fe.detect(0, 2)
    fe.detect(2, 2 * n - 2)
    for s, i in enumerate(moved):
        _same_features(fe.features(s), wants[i], (names, "two calls", s))
    if names in S.PAIRED:
        # one pair through the matcher: k_nn_l2i8 reads the operand image and the norms k_sb_descriptor wrote beside the rows
        a, b = moved.index(0), moved.index(1)                   # the chosen scene against the batch's second frame
        res, _ = fe.run_pairs([[a, b]], np.array([[300.0, 0, w / 2], [0, 300.0, h / 2], [0, 0, 1]]), fe.make_opts(match_mode=F.MATCH_CROSSCHECK))
        qi, ti, dd, _mask = fe.pair_matches(0)
        oq, ot, od = oracle.match_l2(wants[moved[a]]["desc"], wants[moved[b]]["desc"], 2)
        assert len(oq) >= 1 and res["n_match"][0] == len(oq)
        assert res["n_kp1"][0] == wants[moved[a]]["n_found"] and res["n_kp2"][0] == wants[moved[b]]["n_found"]
        assert np.array_equal(qi, oq) and np.array_equal(ti, ot) and np.array_equal(dd, od)


def test_blur_wider_than_63_taps_is_refused_and_the_context_goes_on(oracle, ctx):
    """nOctaveLayers 1 with sigma 1.2 needs a 69-tap blur, one step above what k_sb_sweep holds: both doors answer
    VO_ERR_UNSUPPORTED, and the context they refused on then runs cv2's default parameters as if nothing had happened."""
    from visual_odometry_amd import frontend as F
    from visual_odometry_amd.detector import SiftDetector
    c = S.BY_NAME["too_wide"]
    assert c.unsupported and max(S.census(oracle, c)["taps"]) == 69
    h, w = c.img.shape
    with pytest.raises(NotImplementedError, match="wider than 63 taps"):
        SiftDetector(ctx=ctx, **c.params).detect_arrays(c.img)
    with pytest.raises(NotImplementedError, match="wider than 63 taps"):
        F.FrontEnd(h, w, max_frames=3, max_pairs=1, detector="sift", ctx=ctx, **c.params)
    want = oracle.sift_detect_and_compute(c.img)
    _same_features(SiftDetector(ctx=ctx).detect_arrays(c.img), want, "per image, after the refusal")
    fe = F.FrontEnd(h, w, max_frames=3, max_pairs=1, detector="sift", ctx=ctx, kp_cap=4096)
    frames = [c.img, random_image(901, h, w), random_image(902, h, w)]
    fe.upload(np.stack(frames))
    fe.detect(0, 3)
    _same_features(fe.features(0), want, "batched, after the refusal")
    for s in (1, 2):
        _same_features(fe.features(s), oracle.sift_detect_and_compute(frames[s]), ("batched, after the refusal", s))

"""GPU parity of the whole per-pair path (batched, device resident) and of the drop-in ImagePair classes
against the CPU oracle's restatement of src/visual_slam.py:294-298."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _same_root_finder_rule(kernel_dk_rule):
    """Every test of this module compares the product's DEFAULT mode with the oracle bit for bit, so the oracle runs the
    kernel's Durand-Kerner exit rule; tests/test_gpu_faithful.py covers OpenCV's fixed 300 sweeps on both sides."""
    yield


def _check_pair(res, X, ref):
    assert res["status"] == 0 and ref["rc"] == 0
    assert (res["n_kp1"], res["n_kp2"], res["n_match"], res["n_inl"], res["n_good"]) == \
           (ref["n_kp1"], ref["n_kp2"], ref["n_match"], ref["n_inl"], ref["n_good"])
    got_rt = np.hstack([res["R"].reshape(3, 3), res["t"].reshape(3, 1)])
    assert np.linalg.norm(got_rt - np.hstack([ref["R"], ref["t"]])) < 1e-4
    n = ref["n_inl"]
    Xg, Xr = X[:, :n], ref["X"][:, :n]
    norm_r = np.linalg.norm(Xr[:3], axis=0)
    rel = np.linalg.norm(Xg[:3] - Xr[:3], axis=0) / norm_r
    # DLT points with (almost) no parallax are arbitrarily ill conditioned: a 1e-12 change of [R|t] moves them by
    # more than 1e-3 relative (the reference itself drops far points, visual_slam.py:177-178). The 1e-3 bound is
    # asserted on the points within 10x the median distance, the homogeneous direction on all of them.
    near = norm_r <= 10.0 * np.median(norm_r)
    assert near.sum() > 0.9 * n
    assert rel[near].max() < 1e-3, (rel.max(), norm_r[np.argmax(rel)])
    hg, hr = Xg / np.linalg.norm(Xg, axis=0), Xr / np.linalg.norm(Xr, axis=0)
    assert (1.0 - np.abs((hg * hr).sum(axis=0))).max() < 1e-9
    assert np.allclose(X[3, :n], 1.0)


@pytest.mark.parametrize("match_mode", [0, 1, 2])
def test_batched_pairs_match_oracle(oracle, seq_small, match_mode):
    from visual_odometry_amd.frontend import FrontEnd
    frames, K = seq_small["frames"], seq_small["K"]
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=4, nfeatures=500)
    fe.upload(frames)
    fe.detect(0, 4)
    pairs = [[0, 1], [1, 2], [2, 3], [0, 3]]
    opts = fe.make_opts(match_mode=match_mode, ratio=0.8, want_points=True)
    res, X = fe.run_pairs(pairs, K, opts)
    p = oracle.orb_params(nfeatures=500)
    for i, (a, b) in enumerate(pairs):
        ref = oracle.pair(frames[a], frames[b], p, K, match_mode=match_mode, ratio=0.8)
        _check_pair(res[i], X[i], ref)
        qi, ti, d, m = fe.pair_matches(i)
        d1 = oracle.orb_detect_and_compute(frames[a], p)["desc"]; d2 = oracle.orb_detect_and_compute(frames[b], p)["desc"]
        rq, rt, rd = oracle.match_hamming(d1, d2, 2 if match_mode == 0 else 1) if match_mode != 1 else oracle.knn2_ratio_hamming(d1, d2, 0.8)
        assert np.array_equal(qi, rq) and np.array_equal(ti, rt) and np.array_equal(d, rd)   # bit-exact match pairs


def test_batch_is_independent_of_batching(seq_small):
    """The same pair gives identical results alone and inside a batch (no cross-pair state)."""
    from visual_odometry_amd.frontend import FrontEnd
    frames, K = seq_small["frames"], seq_small["K"]
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=3, nfeatures=500)
    fe.upload(frames); fe.detect(0, 4)
    a, _ = fe.run_pairs([[0, 1], [1, 2], [2, 3]], K)
    a = a.copy()                       # run_pairs returns views of reused page-locked buffers
    b, _ = fe.run_pairs([[1, 2]], K)
    assert a[1].tobytes() == b[0].tobytes()


def test_dropin_image_pair_flow(oracle, seq_small, capsys):
    """FrameGenerator + ImagePair driven exactly as visual_slam.py:294-298 drives them."""
    from visual_odometry_amd import FrameGenerator, ImagePair, ORB_create, BFMatcher
    from visual_odometry_amd.matcher import NORM_HAMMING
    frames, K = seq_small["frames"], seq_small["K"]
    gen = FrameGenerator(ORB_create(nfeatures=500))
    bf = BFMatcher(NORM_HAMMING, crossCheck=True)
    f1, f2 = gen.make_frame(frames[0]), gen.make_frame(frames[1])
    assert (f1.id, f2.id) == (0, 1) and f1.features[3].feature_id == (0, 3)
    ip = ImagePair(f1, f2, bf, K)
    ip.match_features()
    ess = ip.determine_essential_matrix(ip.filtered_matches)
    ip.estimate_camera_movement(ess)
    ip.reconstruct_3d_points(ess)
    out = capsys.readouterr().out
    assert "relative movement in image pair" in out and "Reconstructed points" in out
    ref = oracle.pair(frames[0], frames[1], oracle.orb_params(nfeatures=500), K)
    assert len(ip.raw_matches) == ref["n_match"] and len(ess) == ref["n_inl"]
    assert ip.t.shape == (3, 1) and ip.R.shape == (3, 3) and ip.relative_pose.shape == (4, 4)
    assert np.linalg.norm(np.hstack([ip.R, ip.t]) - np.hstack([ref["R"], ref["t"]])) < 1e-4
    X = ip.points3d_reconstr
    assert X.shape == (4, len(ess)) and np.allclose(X[3], 1.0)
    rel = np.linalg.norm(X[:3] - ref["X"][:3], axis=0) / np.linalg.norm(ref["X"][:3], axis=0)
    assert rel.max() < 1e-3
    m3 = ip.matches_with_3d_information[0]
    assert m3.point == (X[0, 0], X[1, 0], X[2, 0]) and m3.featureid1[0] == 0 and m3.featureid2[0] == 1
    # second entry, as add_information_to_map re-enters (visual_slam.py:165-172): explicit projection matrices
    again = ip.determine_essential_matrix(ip.filtered_matches)
    assert len(again) == len(ess)                       # fixed RANSAC seed: same inliers on the same data
    ip.reconstruct_3d_points(again, np.eye(4)[:3], ip.relative_pose[:3])
    assert ip.points3d_reconstr.shape == (4, len(ess))
    vis = ip.visualize_matches(ess[:20])
    assert vis.shape[1] == 2 * frames[0].shape[1]


def test_too_few_matches_raises(ctx):
    from visual_odometry_amd import Frame, ImagePair, BFMatcher, Feature, KeyPoint
    from visual_odometry_amd.matcher import NORM_HAMMING

    def mk(i, n):
        f = Frame(np.zeros((64, 64), np.uint8)); f.id = i
        f.keypoints = tuple(KeyPoint(10 + k, 10 + 2 * k) for k in range(n))
        f.descriptors = np.random.default_rng(i).integers(0, 256, (n, 32), dtype=np.uint8)
        f.features = [Feature(kp, d, (i, k)) for k, (kp, d) in enumerate(zip(f.keypoints, f.descriptors))]
        return f
    ip = ImagePair(mk(0, 3), mk(1, 3), BFMatcher(NORM_HAMMING, crossCheck=True), np.eye(3))
    ip.match_features()
    with pytest.raises(ValueError):
        ip.determine_essential_matrix(ip.filtered_matches)


def test_bgr_frames_and_config3_shape(oracle):
    """BGR upload (gray conversion on the device) and the 4-level / 4000-feature configuration on a 1080p frame."""
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    seq = synth.sequence(2, 1920, 1080, cache_dir="/tmp")
    gray, K = seq["frames"], seq["K"]
    rng = np.random.default_rng(5)
    bgr = np.clip(gray[..., None].astype(np.int16) + rng.integers(-6, 7, gray.shape + (3,)), 0, 255).astype(np.uint8)
    fe = FrontEnd(1080, 1920, max_frames=2, max_pairs=1, nfeatures=4000, nlevels=4)
    fe.upload(bgr)
    fe.detect(0, 2)
    p = oracle.orb_params(nfeatures=4000, nlevels=4)
    for s in range(2):
        ref = oracle.orb_detect_and_compute(bgr[s], p)
        got = fe.features(s)
        assert len(ref["xy"]) > 3500 and not got["truncated"]
        assert np.array_equal(got["xy"], ref["xy"]) and np.array_equal(got["desc"], ref["desc"])
        assert np.array_equal(got["angle"], ref["angle"]) and np.array_equal(got["response"], ref["response"])
    res, X = fe.run_pairs([[0, 1]], K, want_points=True)
    ref = oracle.pair(oracle.gray(bgr[0]), oracle.gray(bgr[1]), p, K)
    _check_pair(res[0], X[0], ref)


def test_kitti_like_shape(oracle):
    """1241 x 376 (KITTI gray): widths that are not multiples of the tile sizes."""
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    seq = synth.sequence(3, 1241, 376, cache_dir="/tmp")
    fe = FrontEnd(376, 1241, max_frames=3, max_pairs=2, nfeatures=2000)
    fe.upload(seq["frames"]); fe.detect(0, 3)
    res, X = fe.run_pairs([[0, 1], [1, 2]], seq["K"], want_points=True)
    p = oracle.orb_params(nfeatures=2000)
    for i in range(2):
        _check_pair(res[i], X[i], oracle.pair(seq["frames"][i], seq["frames"][i + 1], p, seq["K"]))


def test_two_image_driver_and_image_and_keypoints(oracle, seq_small, tmp_path):
    """ImageAndKeypoints + TriangulatePointsFromTwoImages (the reference's main_triangulate.py flow), from files."""
    from PIL import Image
    from visual_odometry_amd import ImageAndKeypoints, TriangulatePointsFromTwoImages
    frames, K = seq_small["frames"], seq_small["K"]
    names = []
    for i in range(2):
        names.append(str(tmp_path / f"f{i}.png"))
        Image.fromarray(np.stack([frames[i]] * 3, axis=2)).save(names[-1])
    iak = ImageAndKeypoints("ORB")
    iak.set_image(np.stack([frames[0]] * 3, axis=2))
    iak.detect_keypoints()
    assert len(iak.keypoints) == len(iak.kp_colors) == len(iak.descriptors) > 100
    assert iak.kp_colors[0].shape == (3,)
    pair = TriangulatePointsFromTwoImages(camera_matrix=K).run(names[0], names[1])
    ref = oracle.pair(frames[0], frames[1], oracle.orb_params(nfeatures=500), K)       # gray of an r=g=b image is itself
    assert len(pair.raw_matches) == ref["n_match"]
    assert np.linalg.norm(np.hstack([pair.R, pair.t]) - np.hstack([ref["R"], ref["t"]])) < 1e-4
    assert pair.points3d_reconstr.shape == (4, ref["n_inl"])


def test_long_sequence_every_pair_identical_to_oracle(oracle):
    """23 consecutive pairs of a KITTI-shaped sequence (wide, short frames: many badly conditioned samples, weak
    cheirality).  The five-point solver runs the same IEEE operations in the same order on both sides, so the
    RANSAC decisions, inlier sets and [R|t] must agree exactly — this caught a premature RANSAC exit once."""
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    n = 24
    seq = synth.sequence(n, 1241, 376, cache_dir="/tmp")
    fe = FrontEnd(376, 1241, n, n - 1, nfeatures=2000)
    fe.upload(seq["frames"]); fe.detect(0, n)
    res, _ = fe.run_pairs([[i, i + 1] for i in range(n - 1)], seq["K"])
    p = oracle.orb_params(nfeatures=2000)
    for k in range(n - 1):
        ref = oracle.pair(seq["frames"][k], seq["frames"][k + 1], p, seq["K"], want_points=False)
        g = res[k]
        assert (g["n_match"], g["n_inl"], g["n_good"]) == (ref["n_match"], ref["n_inl"], ref["n_good"]), k
        d = np.linalg.norm(np.hstack([g["R"].reshape(3, 3), g["t"].reshape(3, 1)]) - np.hstack([ref["R"], ref["t"]]))
        assert d < 1e-9, (k, d)


def test_overlapped_contexts_are_deterministic():
    """Two contexts alternating chunks (asynchronous detect + pairs, chained detections) must reproduce the
    synchronous single-context results bit for bit, chunk after chunk: catches kernels that lean on timing
    (a missing wait on an LDS-DMA in the MFMA matcher once showed up exactly here)."""
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    C = 48
    seq = synth.sequence(9, 1280, 720, cache_dir="/tmp")
    order = [(i % 16 if i % 16 < 9 else 16 - i % 16) for i in range(C + 1)]
    frames = seq["frames"][order]
    pairs = np.stack([np.arange(C), np.arange(C) + 1], 1).astype(np.int32)
    fes = [FrontEnd(720, 1280, max_frames=C + 1, max_pairs=C, nfeatures=2000) for _ in range(2)]
    for f in fes:
        f.upload(frames)
    opts = fes[0].make_opts(want_points=True)

    def key(r):
        return np.concatenate([r[k].astype(np.float64).ravel()
                               for k in ("status", "n_kp1", "n_match", "n_inl", "n_good", "ransac_iters", "R", "t", "E")])

    fes[0].detect(0, C + 1)
    ref = key(fes[0].run_pairs(pairs, seq["K"], opts)[0])
    inflight = [None, None]
    for it in range(10):
        k = it % 2
        if inflight[k] is not None:
            fes[k].wait()
            assert np.array_equal(key(inflight[k]), ref), f"chunk {it - 2} differs from the synchronous run"
        fes[k].detect(0, C + 1, wait=False, after=fes[1 - k])
        inflight[k] = fes[k].run_pairs(pairs, seq["K"], opts, wait=False)[0]
    for k in range(2):
        fes[k].wait()
        assert np.array_equal(key(inflight[k]), ref)


def test_reconfigure_recycles_memory_safely(oracle, seq_small):
    """vo_batch_configure frees and reallocates every device buffer.  The MFMA matcher multiplies the unwritten rows
    of the last 16-row group of the expanded descriptors (it masks them with a bias), so those rows must never hold
    arbitrary recycled bytes: configure small -> large (fill the heap with image noise) -> small again on ONE context
    and compare the match lists with the oracle."""
    from conftest import random_image
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    frames, K = seq_small["frames"], seq_small["K"]
    c = _lib.Context(0)
    p = oracle.orb_params(nfeatures=500)
    d = [oracle.orb_detect_and_compute(frames[i], p)["desc"] for i in range(3)]
    want = [oracle.match_hamming(d[i], d[i + 1], 2) for i in range(2)]
    for round_ in range(3):
        fe = FrontEnd(480, 640, max_frames=3, max_pairs=2, nfeatures=500, ctx=c)
        fe.upload(frames[:3]); fe.detect(0, 3)
        fe.run_pairs([[0, 1], [1, 2]], K)
        for i in range(2):
            qi, ti, dd, _ = fe.pair_matches(i)
            assert np.array_equal(qi, want[i][0]) and np.array_equal(ti, want[i][1]) and np.array_equal(dd, want[i][2]), (round_, i)
        big = FrontEnd(1080, 1920, max_frames=6, max_pairs=2, nfeatures=4000, nlevels=4, ctx=c)
        noise = np.stack([random_image(40 + round_ * 7 + k, 1080, 1920) | 0x80 for k in range(6)])
        big.upload(noise); big.detect(0, 6)
    c.close()


def test_library_gather_equals_local_records(seq_small):
    """vo_pairs_gather: the [R|t] + counts records packed on the device (k_pack_records) and all-gathered by the
    library itself (ncclAllGather from librccl.so on the context's stream).  Without a communicator it returns the
    local records; with a world-size-1 RCCL communicator the same bytes must come back through the collective.  Both
    equal sharding.pack_records of the structured results (the host-side statement of the record layout).  The launchers'
    small all-gather of host doubles (vo_comm_allgather_f64) returns its input through the same communicator."""
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    from visual_odometry_amd.sharding import pack_records
    frames, K = seq_small["frames"], seq_small["K"]
    c = _lib.Context(0)
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=3, nfeatures=500, ctx=c)
    fe.upload(frames[:4]); fe.detect(0, 4)
    res = fe.run_pairs([[0, 1], [1, 2], [2, 3]], K)[0]
    want = pack_records(res)
    local = fe.gather_records(3).copy()
    assert local.shape == (1, 3, _lib.VO_RECORD_DOUBLES) and np.array_equal(local[0], want)
    c.comm_init(c.comm_unique_id(), 0, 1)
    try:
        got = fe.gather_records(3, world=1).copy()
        assert np.array_equal(got[0], want)
        part = fe.gather_records(2, world=1).copy()                    # a shorter prefix of the same run
        assert np.array_equal(part[0], want[:2])
        for n in (1, 4096):                                            # one value (the barrier) up to the largest n
            v = np.random.default_rng(n).standard_normal(n)
            got = c.allgather(v, 1)
            assert got.shape == (1, n) and np.array_equal(got[0], v)
        with pytest.raises(_lib.VoError):
            c.allgather(np.zeros(4097), 1)
    finally:
        c.comm_destroy()
    c.close()

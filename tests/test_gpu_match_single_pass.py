"""GPU parity of the single-pass cross-check: with the FP4 matrix-core matcher, BFMatcher(crossCheck=True) takes both
nearest-neighbour directions from one sweep of each pair's distance matrix (the reverse direction from column maxima).
Checked against the XOR + popcount and int8 matrix-core kernels, which still run the two directions separately, and
against the CPU oracle: uneven sizes, one-row and empty sides, all-equal descriptors, and a keypoint capacity above
the single pass's LDS limit (two-sweep fallback)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _descs(seed, n, dup_from=None, flip_bits=0):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if dup_from is not None:
        m = min(n, len(dup_from))
        d[:m] = dup_from[rng.permutation(len(dup_from))[:m]]
        for i in range(m):
            for b in rng.integers(0, 256, rng.integers(0, flip_bits + 1)):
                d[i, b // 8] ^= 1 << (b % 8)
    return d


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# (nq, nt): counts off the 16-column groups, the 128-row B stages and the 512-row workgroups, one-row sides, nq != nt
SIZES = [(1, 1), (1, 300), (300, 1), (15, 17), (17, 900), (513, 31), (1000, 15), (511, 513), (1025, 1537),
         (2000, 2000), (2256, 2255), (3001, 2999)]


@pytest.mark.parametrize("kernel", ["mfma_fp4", "mfma", "popcount"])
def test_cross_check_kernels_agree(oracle, kernel):
    from visual_odometry_amd import _lib
    from visual_odometry_amd.matcher import HammingMatcher
    c = _lib.Context(0)
    try:
        c.set_matcher_kernel(kernel)
        for nq, nt in SIZES:
            t = _descs(nq + 31, nt)
            q = _descs(nt + 77, nq, dup_from=t, flip_bits=40)
            for mode in (0, 1, 2):
                m = HammingMatcher(crossCheck=mode > 0, legacy_crosscheck=mode == 1, ctx=c)
                assert _same(m.match_arrays(q, t), oracle.match_hamming(q, t, mode)), (kernel, nq, nt, mode)
                # the other direction of the same pair (frame 2 -> frame 1)
                assert _same(m.match_arrays(t, q), oracle.match_hamming(t, q, mode)), (kernel, nt, nq, mode)
    finally:
        c.close()


def test_single_pass_ties_go_to_the_lowest_index(oracle):
    from visual_odometry_amd import _lib
    from visual_odometry_amd.matcher import HammingMatcher
    c = _lib.Context(0)
    try:
        c.set_matcher_kernel("mfma_fp4")
        m = HammingMatcher(crossCheck=True, ctx=c)
        z = np.zeros((600, 32), np.uint8)
        o = np.full((530, 32), 255, np.uint8)
        for q, t in ((z, z), (z, o), (o, z), (z[:1], o[:1]), (o[:520], o[:17])):   # every distance equal: all ties
            assert _same(m.match_arrays(q, t), oracle.match_hamming(q, t, 2))
        rng = np.random.default_rng(5)
        base = rng.integers(0, 256, (8, 32), dtype=np.uint8)
        q, t = base[rng.integers(0, 8, 1300)], base[rng.integers(0, 8, 700)]   # duplicates spread over row blocks and stages
        assert _same(m.match_arrays(q, t), oracle.match_hamming(q, t, 2))
        assert _same(m.match_arrays(t, q), oracle.match_hamming(t, q, 2))
    finally:
        c.close()


def test_capacity_above_the_single_pass_limit(oracle):
    """4000 rows give a keypoint capacity above the single pass's LDS column array but below the FP4 limit: the two-sweep
    launch runs, with the same results."""
    from visual_odometry_amd import _lib
    from visual_odometry_amd.matcher import HammingMatcher
    c = _lib.Context(0)
    try:
        c.set_matcher_kernel("mfma_fp4")
        m = HammingMatcher(crossCheck=True, ctx=c)
        for nq, nt in ((4000, 3990), (700, 4100)):
            t = _descs(nq, nt)
            q = _descs(nt, nq, dup_from=t, flip_bits=40)
            assert _same(m.match_arrays(q, t), oracle.match_hamming(q, t, 2)), (nq, nt)
        # the same context now matches small sets at that capacity
        t = _descs(3, 900)
        q = _descs(4, 1100, dup_from=t, flip_bits=40)
        assert _same(m.match_arrays(q, t), oracle.match_hamming(q, t, 2))
    finally:
        c.close()


def test_pairs_with_an_empty_frame(oracle, seq_small):
    """Batched pairs where one frame has no keypoints (either side), next to a normal pair."""
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    c = _lib.Context(0)
    try:
        frames, K = seq_small["frames"], seq_small["K"]
        blank = np.zeros_like(frames[0])
        fe = FrontEnd(480, 640, max_frames=3, max_pairs=3, nfeatures=500, ctx=c)
        fe.upload([frames[0], frames[1], blank]); fe.detect(0, 3)
        res = fe.run_pairs([[0, 1], [0, 2], [2, 1]], K)[0]
        r = oracle.pair(frames[0], frames[1], oracle.orb_params(nfeatures=500), K, want_points=False)
        assert (int(res["n_match"][0]), int(res["n_inl"][0])) == (r["n_match"], r["n_inl"])
        assert int(res["n_kp2"][1]) == 0 and int(res["n_match"][1]) == 0
        assert int(res["n_kp1"][2]) == 0 and int(res["n_match"][2]) == 0
    finally:
        c.close()

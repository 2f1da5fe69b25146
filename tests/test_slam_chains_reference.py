"""No GPU: what tests/test_gpu_slam_chains.py builds on.  The sequences it cuts from synth.sequence(7, 640, 480, step=4.0) /
1000 features / max_cameras = 4 are not trivial for the free-running checker (tests/slam_reference.py on oracle features):
A = frames 0..6 localises its 6 pairs and evicts a camera at pairs 3, 4, 5; B = frames 2..6 localises its 4 pairs and evicts at
its pair 3; C = frames 0, 1, 2 localises both pairs.  And the pure helpers of FrontEnd.slam_chains: sequence lengths -> seq_off,
flat outputs -> one dict per sequence."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
SEQUENCES = dict(A=[0, 1, 2, 3, 4, 5, 6], B=[2, 3, 4, 5, 6], C=[0, 1, 2])


@pytest.fixture(scope="module")
def free_runs(oracle):
    from visual_odometry_amd import synth
    oracle.set_dk_early_exit(True)
    try:
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        p = oracle.orb_params(nfeatures=NFEAT)
        feats = [oracle.orb_detect_and_compute(f, p) for f in seq["frames"]]
        out = {}
        for name, frames in SEQUENCES.items():
            own = [feats[f] for f in frames]                                  # frames numbered along the sequence's own chain
            pin = S.pair_inputs_from_oracle(oracle, own, [[k, k + 1] for k in range(len(frames) - 1)], seq["K"])
            out[name] = S.run(oracle, pin, seq["K"], dict(max_cameras=MAX_CAMERAS))
        return out
    finally:
        oracle.set_dk_early_exit(False)


def test_sequence_a_localises_six_pairs_and_evicts_three_times(free_runs):
    res = free_runs["A"]
    assert [r["status"] for r in res] == [0] * 6
    assert [r["n_corr"] for r in res[1:]] == [203, 202, 181, 213, 246]
    assert [r["evicted"] is not None for r in res] == [False, False, False, True, True, True]


def test_sequence_b_starts_elsewhere_and_evicts_at_its_last_pair(free_runs):
    res = free_runs["B"]
    assert [r["status"] for r in res] == [0] * 4
    assert [r["n_corr"] for r in res[1:]] == [181, 213, 132]
    assert [r["evicted"] is not None for r in res] == [False, False, False, True]
    assert res[-1]["state"]["cam_frame"] == [1, 2, 3, 4]                      # indices along B's own chain


def test_sequence_c_localises_both_pairs(free_runs):
    res = free_runs["C"]
    assert [r["status"] for r in res] == [0, 0] and res[1]["n_corr"] > 50
    assert [r["evicted"] for r in res] == [None, None]


def test_sequence_offsets():
    from visual_odometry_amd.frontend import sequence_offsets
    off = sequence_offsets([3, 2, 6, 4], 15)
    assert off.dtype == np.int32 and off.tolist() == [0, 3, 5, 11, 15]
    assert sequence_offsets((7,), 7).tolist() == [0, 7]
    assert sequence_offsets(np.array([1, 1], np.int64), 2).tolist() == [0, 1, 2]
    for bad, n in (([], 0), ([], 3), ([3, 0], 3), ([4, -1], 3), ([2, 1], 4), ([2, 3], 4), ([1], 0)):
        with pytest.raises(ValueError):
            sequence_offsets(bad, n)


def test_split_sequences():
    from visual_odometry_amd.frontend import sequence_offsets, split_sequences
    lengths = [3, 2, 6, 4]
    off = sequence_offsets(lengths, 15)
    B, n_seq = 15, len(lengths)
    flat = dict(poses_pnp=np.arange((B + n_seq) * 12, dtype=np.float64).reshape(B + n_seq, 12), poses=-np.arange((B + n_seq) * 12, dtype=np.float64).reshape(B + n_seq, 12),
                chi2=np.arange(2 * B, dtype=np.float64).reshape(B, 2), status=np.arange(B, dtype=np.int32), n_cam=100 + np.arange(B, dtype=np.int32))
    out = split_sequences(flat, off)
    assert len(out) == n_seq and all(set(d) == set(flat) for d in out)
    row = 0
    for s, (d, n) in enumerate(zip(out, lengths)):
        assert d["poses_pnp"].shape == d["poses"].shape == (n + 1, 3, 4) and d["chi2"].shape == (n, 2) and d["status"].shape == (n,)
        assert d["status"].tolist() == list(range(off[s], off[s + 1])) and d["n_cam"].tolist() == [100 + v for v in range(off[s], off[s + 1])]
        assert d["chi2"][0, 0] == 2 * off[s] and d["chi2"][-1, 1] == 2 * off[s + 1] - 1
        assert d["poses_pnp"][0, 0, 0] == 12 * row and d["poses"][-1, 2, 3] == -(12 * (row + n + 1) - 1)    # rows seq_off[s] + s .. seq_off[s + 1] + s
        row += n + 1
    assert row == B + n_seq
    flat["status"][:] = -1                                                    # the per-sequence arrays are copies
    assert out[0]["status"].tolist() == [0, 1, 2]

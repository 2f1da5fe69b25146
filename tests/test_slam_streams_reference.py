"""No GPU: the two pure helpers of FrontEnd.slam_streams.  stream_slice takes one sequence's part out of the dict a multi-stream call
returns, join_streams joins every sequence's flight; both must undo exactly the layout vo_slam_streams writes (per-pair rows
seq_off[s] .. seq_off[s + 1] - 1, pose rows seq_off[s] + s .. seq_off[s + 1] + s, an idle sequence one pose row and no pair).

The calls are built from the CPU walker of tests/slam_stream_restart_reference.py on the flights the GPU test uses, so the segment
tables, statuses, counts, list sizes and carried cameras are real ones — L loses two frames and restarts, and one of its calls is
lost from end to end; the pose rows carry marks that say which flight, call and frame they belong to (join_stream's choice of the
LATEST report of a frame is what is at stake there, not the arithmetic).  The yardstick is join_stream of the flight walked alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_restart_reference as RR  # noqa: E402
import slam_stream_restart_reference as R  # noqa: E402

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
CHAINS = dict(L=[0, 1, 2, 3, None, 2, 3, 4, 5, 6], A=[0, 1, 2, 3, 4, 5, 6])
SPLITS = dict(L=(4, 1, 4), A=(2, 4))
PAIR_KEYS = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")
SEG_KEYS = ("segment", "cause", "seg_poses_pnp", "seg_poses")


def _mark(flight, call, frame, kind):
    return np.full((3, 4), 1000.0 * (1 + "LA".index(flight)) + 100.0 * call + frame + 0.25 * kind)


def _calls(flight, res, carries, split):
    """the dicts slam_stream_restart would return for the walk, call by call: the walker's tables, marked pose rows"""
    calls, at = [], 0
    for c, n in enumerate(split):
        rows = res[at:at + n]
        d = dict(status=np.array([r["status"] for r in rows], np.int32), n_corr=np.array([r["n_corr"] for r in rows], np.int32),
                 n_inl=np.array([r["n_inl"] for r in rows], np.int32), segment=np.array([r["segment"] for r in rows], np.int32),
                 cause=np.array([r["cause"] for r in rows], np.int32),
                 n_pts=np.array([len(r["state"]["points"]) for r in rows], np.int32), n_obs=np.array([len(r["state"]["obs_cam"]) for r in rows], np.int32),
                 n_cam=np.array([len(r["state"]["cam_frame"]) for r in rows], np.int32),
                 ba_iterations=np.arange(at, at + n, dtype=np.int32), ba_trials=np.arange(at, at + n, dtype=np.int32) * 2,
                 chi2=np.stack([np.array([at + j, at + j + 0.5]) for j in range(n)]))
        # a frame no pair localised has all-zero rows, as on the device
        ok = [True] + [r["status"] == 0 for r in rows]
        if c > 0:
            ok[0] = bool(calls[-1]["poses_pnp"][-1].any())
        d["poses_pnp"] = np.stack([_mark(flight, 0, at + j, 0) * ok[j] for j in range(n + 1)])   # the same mark in every call: row 0 is the call before's last
        d["poses"] = np.stack([_mark(flight, c, at + j, 1) * ok[j] for j in range(n + 1)])
        starts = [j for j in range(n) if rows[j]["segment"] >= 0 and (at + j == 0 or res[at + j - 1]["segment"] != rows[j]["segment"])]
        d["seg_poses_pnp"] = np.stack([_mark(flight, c, at + j, 2) * (j in starts) for j in range(n)])
        d["seg_poses"] = np.stack([_mark(flight, c, at + j, 3) * (j in starts) for j in range(n)])
        cams = carries[c - 1]["cameras"] if c > 0 else []
        cams = [f for f in cams if f != at]                                 # the anchor has row 0, never a carried row
        d["carried_frame"] = np.array(cams, np.int32)
        d["carried_poses"] = np.stack([_mark(flight, c, f, 1) for f in cams]) if cams else np.zeros((0, 3, 4))
        calls.append(d)
        at += n
    return calls


@pytest.fixture(scope="module")
def walked(oracle):
    from visual_odometry_amd import synth
    oracle.set_dk_early_exit(True)
    try:
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        p = oracle.orb_params(nfeatures=NFEAT)
        feats = [oracle.orb_detect_and_compute(f, p) for f in seq["frames"]]
        blank = oracle.orb_detect_and_compute(np.full_like(seq["frames"][0], 127), p)
        out = {}
        for name, frames in CHAINS.items():
            pins = RR.pair_inputs_from_oracle(oracle, [blank if f is None else feats[f] for f in frames], seq["K"])
            res, _, carries = R.run_chunked(oracle, pins, seq["K"], SPLITS[name], {"max_cameras": MAX_CAMERAS})
            out[name] = _calls(name, res, carries, SPLITS[name])
    finally:
        oracle.set_dk_early_exit(False)
    return out


def _pack(parts):
    """what slam_streams returns for one call: parts[s] is sequence s's own call dict, or (None, anchor rows) if it is idle"""
    lengths = [0 if d is None else len(d["status"]) for d, _ in parts]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    B, n_seq = int(off[-1]), len(parts)
    out = dict(seq_off=off, poses_pnp=np.zeros((B + n_seq, 3, 4)), poses=np.zeros((B + n_seq, 3, 4)), chi2=np.zeros((B, 2)),
               seg_poses_pnp=np.zeros((B, 3, 4)), seg_poses=np.zeros((B, 3, 4)), n_carried=np.zeros(n_seq, np.int32), carried_frame=[], carried_poses=[])
    out.update({k: np.zeros(B, np.int32) for k in PAIR_KEYS + ("segment", "cause") if k != "chi2"})
    for s, (d, anchor) in enumerate(parts):
        a, b = int(off[s]), int(off[s + 1])
        if d is None:
            out["poses_pnp"][a + s], out["poses"][a + s] = anchor
            out["carried_frame"].append(np.zeros(0, np.int32)); out["carried_poses"].append(np.zeros((0, 3, 4)))
            continue
        for k in PAIR_KEYS + SEG_KEYS:
            out[k][a:b] = d[k]
        out["poses_pnp"][a + s:b + s + 1] = d["poses_pnp"]; out["poses"][a + s:b + s + 1] = d["poses"]
        out["n_carried"][s] = len(d["carried_frame"])
        out["carried_frame"].append(d["carried_frame"].copy()); out["carried_poses"].append(d["carried_poses"].copy())
    return out


def _schedule(walked, order):
    """L 4+1+4 beside A 2+0+4: A is idle in the call in which L is lost from end to end"""
    per_call = dict(L=[0, 1, 2], A=[0, None, 1])
    outs = []
    for c in range(3):
        parts = []
        for name in order:
            k = per_call[name][c]
            if k is None:
                last = walked[name][per_call[name][c - 1]]
                parts.append((None, (last["poses_pnp"][-1], last["poses"][-1])))
            else:
                parts.append((walked[name][k], None))
        outs.append(_pack(parts))
    return outs


def _same_dict(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), (what, k)


@pytest.mark.parametrize("order", [("L", "A"), ("A", "L")], ids=["L,A", "A,L"])
def test_slices_and_joins_undo_the_layout(walked, order):
    from visual_odometry_amd.frontend import join_stream, join_streams, stream_slice
    assert walked["L"][1]["segment"].tolist() == [-1] and not walked["L"][1]["poses"].any()      # the all-lost call
    assert walked["L"][2]["segment"].tolist() == [1, 1, 1, 1] and walked["L"][2]["carried_frame"].tolist() == [0, 1, 2, 3]
    outs = _schedule(walked, order)
    assert [o["seq_off"].tolist() for o in outs] == ([[0, 4, 6], [0, 1, 1], [0, 4, 8]] if order[0] == "L" else [[0, 2, 6], [0, 0, 1], [0, 4, 8]])
    per_call = dict(L=[0, 1, 2], A=[0, None, 1])
    for s, name in enumerate(order):
        for c, o in enumerate(outs):
            sl, k = stream_slice(o, s), per_call[name][c]
            if k is None:                                                    # idle: no pair, the anchor's row, nothing carried
                assert len(sl["status"]) == 0 and sl["chi2"].shape == (0, 2) and sl["seg_poses"].shape == (0, 3, 4)
                assert sl["poses_pnp"].shape == (1, 3, 4) and np.array_equal(sl["poses"][0], walked[name][0]["poses"][-1])
                assert len(sl["carried_frame"]) == 0 and sl["carried_poses"].shape == (0, 3, 4)
            else:
                _same_dict(walked[name][k], sl, (order, name, c))
        sl = stream_slice(outs[0], s)
        sl["poses"][:] = -1
        assert not (stream_slice(outs[0], s)["poses"] == -1).any()                                # copies
    joined = join_streams(outs)
    assert len(joined) == 2
    for s, name in enumerate(order):
        _same_dict(join_stream(walked[name]), joined[s], (order, name))
    L = joined[order.index("L")]
    assert L["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1] and len(L["poses"]) == 10 and len(joined[order.index("A")]["poses"]) == 7


def test_the_helpers_refuse_what_is_not_a_stream(walked):
    from visual_odometry_amd.frontend import join_streams, stream_slice
    outs = _schedule(walked, ("L", "A"))
    with pytest.raises(ValueError):
        stream_slice(outs[0], 2)
    with pytest.raises(ValueError):
        join_streams([])
    with pytest.raises(ValueError):
        join_streams([outs[0], _pack([(walked["L"][1], None)])])                                  # another number of sequences
    with pytest.raises(ValueError):
        join_streams([outs[1]])                                                                  # a sequence that never advanced has no flight

"""No GPU: the append and stage rules of a stream's descriptor store (tests/stream_rows_reference.py) on the chunked walk of
tests/slam_stream_reference.py, sequence A of tests/test_gpu_slam_stream.py (7 frames, 1000 features, max_cameras = 4: pairs 3, 4
and 5 evict a camera).  The rules on hand-made maps, and the premises tests/test_gpu_stream_rows.py rests on: on every split it
uses, a point that already has a row is moved by a later eviction's compaction (a store that kept a row per LIST INDEX would then
hand out another point's descriptor), and the overflow capacity drops a point that is still in the stream's last map."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
import stream_rows_reference as SR  # noqa: E402

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
OPTS = dict(max_cameras=MAX_CAMERAS)


def test_rows_are_handed_out_in_map_order_per_call_and_keyed_by_feature():
    st = SR.Store(-1, total_pairs=3, kp_cap=10)
    assert st.capacity == 40
    st.append([(0, 5), (0, 2), (1, 7)], frame0=0)
    assert st.rows == [(0, 5), (0, 2), (1, 7)] and st.row_of == {(0, 5): 0, (0, 2): 1, (1, 7): 2}
    # the next call: (0, 5) was removed, the list was compacted, two points were born; (1, 3) lies before frame0 and has no row:
    # it was not in the end map of its own call (it cannot happen on the device; the rule leaves it without a row)
    st.append([(0, 2), (1, 7), (1, 3), (2, 9), (3, 0)], frame0=2)
    assert st.rows == [(0, 5), (0, 2), (1, 7), (2, 9), (3, 0)]           # row 0 stays: a hole
    assert st.info() == dict(capacity=40, stored=5, dropped=0)
    st.append([(0, 2), (2, 9), (3, 0)], frame0=3)                        # (3, 0) has its row: nothing is appended twice
    assert st.stored == 5
    keep, rows, without = st.stage([(1, 7), (0, 2), (1, 3), (3, 0)])
    assert keep.tolist() == [0, 1, 3] and rows.tolist() == [2, 1, 4] and without == 1


def test_drops_at_capacity_are_for_good():
    st = SR.Store(2, total_pairs=3, kp_cap=10)
    st.append([(0, 1), (0, 2), (1, 3), (1, 4)], frame0=0)
    assert st.info() == dict(capacity=2, stored=2, dropped=2) and st.rows == [(0, 1), (0, 2)]
    st.append([(1, 3), (1, 4), (2, 5)], frame0=2)                        # (1, 3) and (1, 4) are not tried again, (2, 5) is dropped
    assert st.info() == dict(capacity=2, stored=2, dropped=3)
    keep, rows, without = st.stage([(0, 2), (1, 3), (2, 5)])
    assert keep.tolist() == [0] and rows.tolist() == [1] and without == 2
    assert SR.Store(0, 3, 10).capacity == 0


def test_the_window_is_by_owning_frame_half_open():
    st = SR.Store(-1, total_pairs=5, kp_cap=10)
    feats = [(0, 1), (2, 1), (2, 3), (4, 0), (5, 9)]
    st.append(feats, frame0=0)
    assert st.stage(feats, 0, 2)[0].tolist() == [0]
    assert st.stage(feats, 2, 5)[0].tolist() == [1, 2, 3]
    assert st.stage(feats, 5, -1)[0].tolist() == [4] and st.stage(feats, 5, None)[0].tolist() == [4]
    assert st.stage(feats, 3, 3)[0].tolist() == [] and st.stage(feats, 3, 3)[2] == 0
    assert st.stage(feats)[0].tolist() == [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def walk(oracle):
    """-> (pair inputs, K, the free-running walk of sequence A with the map of every stage of every pair)"""
    from visual_odometry_amd import synth
    oracle.set_dk_early_exit(True)
    try:
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        p = oracle.orb_params(nfeatures=NFEAT)
        feats = [oracle.orb_detect_and_compute(f, p) for f in seq["frames"]]
        pin = S.pair_inputs_from_oracle(oracle, feats, [[k, k + 1] for k in range(N - 1)], seq["K"])
        s, free = S.empty_state(), []
        for pr in pin:
            r = S.step(oracle, s, pr, seq["K"], OPTS, stages=True)
            assert r["status"] == 0
            free.append(r); s = r["state"]
        yield pin, seq["K"], free, NFEAT                                  # (a frame holds at most nfeatures keypoints)
    finally:
        oracle.set_dk_early_exit(False)


@pytest.mark.parametrize("split", SR.SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_on_sequence_a_a_point_with_a_row_is_moved_by_a_later_eviction(oracle, walk, split):
    pin, K, free, kp_cap = walk
    assert [r["evicted"] is not None for r in free] == [False, False, False, True, True, True]
    maps = SR.chunk_maps(oracle, pin, K, split, OPTS)
    # the chunked walk's maps are the free-running walk's at the same pairs (what the stream contract says of the device)
    for m, nxt in zip(maps, maps[1:] + [None]):
        end = (nxt["frame0"] if nxt is not None else N - 1) - 1
        want = free[end]["stage"][4]
        assert [tuple(int(v) for v in f) for f in want["pt_feature"]] == m["pt_feature"] and np.array_equal(want["points"], m["points"])
    evicting = [p for p, r in enumerate(free) if r["evicted"] is not None]
    stage3 = {p: free[p]["stage"][3]["pt_feature"] for p in evicting}
    stage4 = {p: free[p]["stage"][4]["pt_feature"] for p in evicting}
    moved = SR.moved_with_a_row(maps, stage3, stage4)
    print("split", split, "map sizes", [len(m["pt_feature"]) for m in maps], "points with a row moved by a later eviction:", moved)
    assert moved >= 1
    # capacity -1: nothing is dropped, every point of every end map has a row, and rows are in map order within each call
    st, infos = SR.run_store(maps, -1, N - 1, kp_cap)
    assert all(i["dropped"] == 0 for i in infos) and [i["stored"] for i in infos] == sorted(i["stored"] for i in infos)
    for m in maps:
        assert all(f in st.row_of for f in m["pt_feature"])
    at = 0
    for m, i in zip(maps, infos):
        new = [f for f in m["pt_feature"] if f[0] >= m["frame0"] and st.row_of[f] >= at]
        assert [st.row_of[f] for f in new] == list(range(at, i["stored"]))
        at = i["stored"]
    assert len(set(st.rows)) == len(st.rows)
    # holes: rows whose point is gone from the last map
    holes = [f for f in st.rows if f not in set(maps[-1]["pt_feature"])]
    print("rows", st.stored, "holes at the end", len(holes))
    assert len(holes) >= 1
    keep, rows, without = st.stage(maps[-1]["pt_feature"])
    assert without == 0 and keep.tolist() == list(range(len(maps[-1]["pt_feature"])))


def test_the_overflow_capacity_drops_a_point_that_survives(oracle, walk):
    pin, K, free, kp_cap = walk
    maps = SR.chunk_maps(oracle, pin, K, SR.OVERFLOW_SPLIT, OPTS)
    st, infos = SR.run_store(maps, SR.OVERFLOW_CAPACITY, N - 1, kp_cap)
    print("map sizes", [len(m["pt_feature"]) for m in maps], "infos", infos)
    # nothing is dropped in the first call, the store fills INSIDE the second (rows and drops both grow there, so the last free row
    # is handed out in the middle of the new points, with rows of an earlier call below it), and the third finds it full
    assert infos[0]["dropped"] == 0 and 0 < infos[0]["stored"] < SR.OVERFLOW_CAPACITY
    assert infos[1]["stored"] == SR.OVERFLOW_CAPACITY and infos[1]["dropped"] >= 1
    assert infos[2]["stored"] == SR.OVERFLOW_CAPACITY and infos[2]["dropped"] > infos[1]["dropped"]
    keep, rows, without = st.stage(maps[-1]["pt_feature"])
    print("last map", len(maps[-1]["pt_feature"]), "staged", len(keep), "without a row", without)
    assert without >= 1 and len(keep) >= 1 and len(keep) + without == len(maps[-1]["pt_feature"])
    full, _ = SR.run_store(maps, -1, N - 1, kp_cap)
    assert st.rows == full.rows[:SR.OVERFLOW_CAPACITY]                   # the first rows in map order: which are dropped follows from the lists alone

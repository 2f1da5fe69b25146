"""The checker of a stream's descriptor store (vo_set_stream_rows, vo_map_from_stream; docs/kernels/k_stream_rows.md): the append
and stage rules in plain Python over the maps a stream holds at the end of its calls.

  append, at the end of a call whose first frame is frame0 of the stream: every point of the end map, IN MAP ORDER, whose owning
      feature (frame, keypoint) has frame >= frame0 and no row yet takes the next free row; with the store full it is counted as
      dropped and never gets one (its frame is before the next call's frame0).  A point born and removed inside one call is not in
      the end map and gets no row; a row whose point is removed later stays where it is — a hole.
  stage, of a window [first, end): the points of the live map with first <= frame < end that have a row, in map order; the others
      of the window are counted as without a row.

A store row is identified here by the feature whose descriptor it holds: row r of the device's store must be the descriptor of
frame rows[r][0], keypoint rows[r][1], as it was detected.  chunk_maps() produces the per-call maps from the chunked walk of
tests/slam_stream_reference.py (carry() and frame_id() imported, not edited); the GPU test feeds the device's own slam_map() lists
through the same Store."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
import slam_stream_reference as R  # noqa: E402

SPLITS = [(3, 3), (1, 5), (5, 1), (2, 2, 2)]
# The overflow case of tests/test_gpu_stream_rows.py, on sequence A: with this many rows the first call of the split drops nothing,
# the store fills inside the second call's append and the third call finds it full (tests/test_stream_rows_reference.py pins it,
# and that a dropped point is still in the stream's last map).
OVERFLOW_SPLIT, OVERFLOW_CAPACITY = (2, 2, 2), 1000


class Store:
    def __init__(self, capacity, total_pairs, kp_cap):
        self.capacity = (total_pairs + 1) * kp_cap if capacity < 0 else int(capacity)
        self.rows, self.row_of, self.dropped = [], {}, 0      # rows[r] = (frame, keypoint) of the descriptor in row r

    @property
    def stored(self):
        return len(self.rows)

    def info(self):
        return dict(capacity=self.capacity, stored=self.stored, dropped=self.dropped)

    def append(self, pt_feature, frame0):
        """pt_feature: the end map's owning features [(frame along the stream, keypoint)], in map order"""
        for f, k in ((int(a), int(b)) for a, b in pt_feature):
            if f < frame0 or (f, k) in self.row_of:
                continue
            if self.stored < self.capacity:
                self.row_of[(f, k)] = self.stored
                self.rows.append((f, k))
            else:
                self.dropped += 1

    def stage(self, pt_feature, first=0, end=None):
        """-> (indices into the map of the points staged, their store rows, points of the window without a row)"""
        keep, rows, without = [], [], 0
        for i, (f, k) in enumerate((int(a), int(b)) for a, b in pt_feature):
            if f < first or (end is not None and end >= 0 and f >= end):
                continue
            if (f, k) in self.row_of:
                keep.append(i); rows.append(self.row_of[(f, k)])
            else:
                without += 1
        return np.array(keep, np.int64), np.array(rows, np.int64), without


def chunk_maps(O, pair_inputs, K, split, opts=None):
    """R.run_chunked's walk, keeping the map at the end of every chunk: [dict(frame0, pt_feature [(stream frame, keypoint)],
    points [n, 3])].  Every pair must localise."""
    assert sum(split) == len(pair_inputs)
    feat_of, stream_of, ids = {}, {}, {}
    s, maps, at = S.empty_state(), [], 0
    for c, n in enumerate(split):
        if c > 0:
            s = R.carry(s, ids[at], R.GHOST0 + c, feat_of, stream_of)
        for j in range(n + 1):
            if at + j not in ids:
                ids[at + j] = R.frame_id(c, j); stream_of[ids[at + j]] = at + j
        for j in range(n):
            pr = dict(pair_inputs[at + j]); pr["frame1"] = ids[at + j]; pr["frame2"] = ids[at + j + 1]
            r = S.step(O, s, pr, K, opts)
            assert r["status"] == 0, (c, j, r["status"])
            s = r["state"]
        lists = S.to_lists(s)
        feats = [feat_of[fid] if fid in feat_of else (stream_of[fid[0]], fid[1]) for fid in lists["pt_feature"]]
        maps.append(dict(frame0=at, pt_feature=feats, points=np.array(lists["points"], np.float64).reshape(-1, 3)))
        at += n
    return maps


def run_store(maps, capacity, total_pairs, kp_cap):
    """The store after every call of a stream whose end maps are `maps` -> (Store, [info() after each call])"""
    st, infos = Store(capacity, total_pairs, kp_cap), []
    for m in maps:
        st.append(m["pt_feature"], m["frame0"])
        infos.append(st.info())
    return st, infos


def moved_with_a_row(maps, stage3, stage4):
    """Points that had a row at the end of an earlier call and that the camera limit of a later call's pair moves to another index.
    stage3 / stage4: {pair: pt_feature list before / after that pair's limit_number_of_camera_in_map}, for the pairs that evict;
    pairs and frames count along the stream.  A point has a row at pair p if it was in the end map of a call that ended before p
    (capacity -1)."""
    moved = 0
    for p in sorted(stage3):
        have = set()
        for m, nxt in zip(maps, maps[1:] + [None]):
            end_pair = (nxt["frame0"] if nxt is not None else 10 ** 9)
            if end_pair <= p:                                           # the call ended before pair p (its pairs are frame0 .. end_pair - 1)
                have |= {(int(a), int(b)) for a, b in m["pt_feature"]}
        before = {(int(a), int(b)): i for i, (a, b) in enumerate(stage3[p])}
        after = {(int(a), int(b)): i for i, (a, b) in enumerate(stage4[p])}
        moved += sum(1 for f in have if f in before and f in after and before[f] != after[f])
    return moved

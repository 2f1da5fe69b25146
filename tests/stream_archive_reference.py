"""The checker of a stream's archive of evicted points (vo_set_stream_archive, vo_map_from_stream_archive;
docs/kernels/k_stream_archive.md): the removal, row-source, capacity and staging rules in plain Python, beside
tests/stream_rows_reference.Store.

  removal, on the map as it stands before a pair's limit_number_of_camera_in_map ("stage 3": obs_cam, obs_pt, pt_feature, points)
      when that limit evicts camera 0: observations are counted per point among cameras != 0; a point left with exactly one goes, a
      point with none stays (remove_camera_from_map's defaultdict quirk, src/map.py:208-216).  The removed points, IN MAP ORDER,
      are the eviction's entries; evictions follow one another in pair order.
  entry: feature = pt_feature (frame along the stream, keypoint), xyz = the point as stage 3 holds it, evicted_at = the pair along
      the stream, and a copy of the descriptor row — from the slots when the point was born in this call (feature frame >= the
      call's frame0), otherwise from the store (Store.row_of as the call BEFORE left it: the store appends at the end of a call),
      otherwise none (has_row False).
  capacity: an entry past the capacity is counted as dropped, for good; the entries kept are the first in that order.
  stage, of a window [first, end): the entries with first <= feature frame < end that have a row, in archive order; those without
      are counted.  With live, behind the points Store.stage() gives for the live map.

A row is identified here by the feature whose descriptor it holds, as in stream_rows_reference."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rows_reference as SR  # noqa: E402

SPLITS = [(6,), (3, 3), (1, 5), (5, 1), (2, 2, 2)]
# sequence A (7 frames, 640x480, 1000 features, max_cameras = 4) on the CPU walk: points removed by the limits of pairs 3, 4, 5
EVICTED_A = {3: 201, 4: 224, 5: 224}
# the capacity case of tests/test_gpu_stream_archive.py: smaller than the first eviction plus half the second
SMALL_CAPACITY = EVICTED_A[3] + EVICTED_A[4] // 2 - 1
# The store-overflow cases, split (2, 2, 2) on sequence A: entries the row-source rule leaves without a row (CPU walk, pinned by
# tests/test_stream_archive_reference.py).  With stream_rows_reference's 1000 rows the store fills inside the SECOND call, with
# points owned by frame 3 and later — none of which is evicted by pair 5 — so every entry still finds its row.  With 500 rows it
# fills inside the first call, whose end map holds 610 points: points owned by frames 0 .. 2 are dropped before they are evicted.
STORE_OVERFLOW_WITHOUT_ROW = {SR.OVERFLOW_CAPACITY: 0, 500: 232}


def removed_points(obs_cam, obs_pt, npt):
    """indices, ascending, of the points the eviction of camera 0 removes"""
    count = np.zeros(int(npt), np.int64)
    for c, p in zip(np.asarray(obs_cam).tolist(), np.asarray(obs_pt).tolist()):
        if c != 0:
            count[p] += 1
    return np.flatnonzero(count == 1)


class Archive:
    def __init__(self, capacity, total_pairs, kp_cap):
        self.capacity = (total_pairs + 1) * kp_cap if capacity < 0 else int(capacity)
        self.feature, self.xyz, self.evicted_at, self.has_row, self.dropped = [], [], [], [], 0

    @property
    def stored(self):
        return len(self.feature)

    def info(self):
        return dict(capacity=self.capacity, stored=self.stored, dropped=self.dropped)

    def evict(self, m, frame0, pair, store=None):
        """m: the map before the limit of stream pair `pair`, which evicts camera 0 (cam_frame, obs_cam, obs_pt, pt_feature, points;
        frames count along the stream); frame0: first frame of the call the pair belongs to; store: the Store as the call before
        left it (None: no earlier call).  -> the indices removed"""
        gone = removed_points(m["obs_cam"], m["obs_pt"], len(m["points"]))
        for q in gone.tolist():
            f, k = int(m["pt_feature"][q][0]), int(m["pt_feature"][q][1])
            if self.stored >= self.capacity:
                self.dropped += 1
                continue
            self.feature.append((f, k)); self.xyz.append(np.array(m["points"][q], np.float64)); self.evicted_at.append(int(pair))
            self.has_row.append(f >= frame0 or (store is not None and (f, k) in store.row_of))
        return gone

    def arrays(self):
        return dict(feature=np.array(self.feature, np.int32).reshape(-1, 2), xyz=np.array(self.xyz, np.float64).reshape(-1, 3),
                    evicted_at=np.array(self.evicted_at, np.int32), has_row=np.array(self.has_row, bool))

    def stage(self, first=0, end=None):
        """-> (indices of the entries staged, entries of the window without a row)"""
        keep, without = [], 0
        for i, (f, _) in enumerate(self.feature):
            if f < first or (end is not None and end >= 0 and f >= end):
                continue
            if self.has_row[i]:
                keep.append(i)
            else:
                without += 1
        return np.array(keep, np.int64), without


def stage(store, archive, pt_feature, points, first=0, end=None, live=True):
    """What vo_map_from_stream_archive stages -> dict(feature [(frame, keypoint)] whose rows are staged, in order; points [n, 3];
    n, n_archived, without_row)"""
    feats, pts, without = [], [], 0
    if live:
        keep, _, without = store.stage(pt_feature, first, end)
        feats += [(int(pt_feature[i][0]), int(pt_feature[i][1])) for i in keep.tolist()]
        pts += [np.array(points[i], np.float64) for i in keep.tolist()]
    akeep, awithout = archive.stage(first, end)
    feats += [archive.feature[i] for i in akeep.tolist()]
    pts += [archive.xyz[i] for i in akeep.tolist()]
    return dict(feature=feats, points=np.array(pts, np.float64).reshape(-1, 3), n=len(feats), n_archived=len(akeep), without_row=without + awithout)


def run_split(split, stage3, end_maps, capacity, total_pairs, kp_cap, store_capacity=-1):
    """The store and the archive along a stream chunked by `split`.  stage3: {stream pair: the map before that pair's limit} for
    the pairs that evict; end_maps: [dict(frame0, pt_feature)] the map at the end of every call.
    -> (Store, Archive, [archive info after each call])"""
    store, arc, infos, at = SR.Store(store_capacity, total_pairs, kp_cap), Archive(capacity, total_pairs, kp_cap), [], 0
    for c, n in enumerate(split):
        for p in range(at, at + n):
            if p in stage3:
                arc.evict(stage3[p], at, p, store if c > 0 else None)
        store.append(end_maps[c]["pt_feature"], at)
        infos.append(arc.info())
        at += n
    return store, arc, infos


def store_referencing_without_row(split, stage3, end_maps, total_pairs, kp_cap):
    """Entries an archive that only REFERENCED the store (no copy at eviction, no slots) would leave without a row: the point must
    have a store row when it is removed — it was in the end map of an earlier call."""
    store, without, at = SR.Store(-1, total_pairs, kp_cap), 0, 0
    for c, n in enumerate(split):
        for p in range(at, at + n):
            if p in stage3:
                m = stage3[p]
                for q in removed_points(m["obs_cam"], m["obs_pt"], len(m["points"])).tolist():
                    without += (int(m["pt_feature"][q][0]), int(m["pt_feature"][q][1])) not in store.row_of
        store.append(end_maps[c]["pt_feature"], at)
        at += n
    return without

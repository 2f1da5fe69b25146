"""No GPU: the rules of a stream's archive of evicted points (tests/stream_archive_reference.py) on hand-made maps and on the CPU
walk of sequence A of tests/test_gpu_slam_stream.py (7 frames, 640x480, 1000 features, max_cameras = 4: pairs 3, 4 and 5 evict a
camera), and the premises tests/test_gpu_stream_archive.py rests on: the removal rule applied to the map before a limit gives the
map after it; the evictions are large enough to cross a 256-point round of the limit's scan and reach the "one observation left
after the filter" branch; every entry finds a row on every split; an archive that only referenced the store would not.

The chunked walk's maps are the free-running walk's at the same pairs (tests/test_stream_rows_reference.py pins that on every
split), so the maps at the end of a call are taken from the free-running walk here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
import stream_rows_reference as SR  # noqa: E402
import stream_archive_reference as AR  # noqa: E402

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
OPTS = dict(max_cameras=MAX_CAMERAS)


def _map(pt_feature, obs):
    """a hand-made map: obs = [(camera, point)]"""
    return dict(pt_feature=pt_feature, points=[[float(i), 0.5 * i, -1.0 * i] for i in range(len(pt_feature))],
                obs_cam=[c for c, _ in obs], obs_pt=[p for _, p in obs])


def test_a_point_left_with_one_observation_goes_and_a_point_with_none_stays():
    # point 0: cameras 0 and 1 -> one left: goes.  point 1: cameras 1 and 2: stays.  point 2: camera 0 only -> none left: STAYS (the
    # defaultdict quirk).  point 3: no observation at all: stays.  point 4: one observation, in camera 2, which is not evicted: goes.
    m = _map([(0, 7), (1, 3), (0, 9), (1, 1), (2, 2)], [(0, 0), (1, 0), (1, 1), (2, 1), (0, 2), (2, 4)])
    assert AR.removed_points(m["obs_cam"], m["obs_pt"], 5).tolist() == [0, 4]
    arc = AR.Archive(-1, total_pairs=5, kp_cap=10)
    assert arc.capacity == 60
    store = SR.Store(-1, 5, 10)
    store.append([(0, 7)], 0)                                             # the call before left a row for (0, 7) only
    assert arc.evict(m, frame0=2, pair=4, store=store).tolist() == [0, 4]
    a = arc.arrays()
    assert a["feature"].tolist() == [[0, 7], [2, 2]] and a["evicted_at"].tolist() == [4, 4] and a["has_row"].tolist() == [True, True]
    assert a["xyz"].tolist() == [[0.0, 0.0, 0.0], [4.0, 2.0, -4.0]]
    # the row source: (1, 3) lies before frame0 and the store never had it -> no row; (3, 0) was born in this call -> the slots
    m2 = _map([(1, 3), (3, 0)], [(1, 0), (2, 1)])
    arc.evict(m2, frame0=3, pair=5, store=store)
    assert arc.arrays()["has_row"].tolist() == [True, True, False, True] and arc.arrays()["evicted_at"].tolist() == [4, 4, 5, 5]
    assert arc.info() == dict(capacity=60, stored=4, dropped=0)
    keep, without = arc.stage()
    assert keep.tolist() == [0, 1, 3] and without == 1


def test_drops_at_capacity_are_for_good_and_keep_the_first_entries():
    m = _map([(0, 1), (0, 2), (0, 3)], [(1, 0), (1, 1), (1, 2)])
    arc = AR.Archive(2, 5, 10)
    arc.evict(m, 0, 1)
    assert arc.info() == dict(capacity=2, stored=2, dropped=1) and arc.feature == [(0, 1), (0, 2)]
    arc.evict(_map([(1, 4)], [(1, 0)]), 0, 2)
    assert arc.info() == dict(capacity=2, stored=2, dropped=2) and arc.feature == [(0, 1), (0, 2)]
    assert AR.Archive(0, 5, 10).capacity == 0


def test_windows_are_half_open_and_the_archived_points_follow_the_live_ones():
    arc = AR.Archive(-1, 6, 10)
    arc.evict(_map([(0, 1), (2, 1), (2, 3), (4, 0), (5, 9)], [(1, q) for q in range(5)]), 0, 5)
    assert arc.stage(0, 2)[0].tolist() == [0] and arc.stage(2, 5)[0].tolist() == [1, 2, 3]
    assert arc.stage(5, -1)[0].tolist() == [4] and arc.stage(5, None)[0].tolist() == [4]
    assert arc.stage(3, 3)[0].tolist() == [] and arc.stage()[0].tolist() == [0, 1, 2, 3, 4]
    store = SR.Store(-1, 6, 10)
    live = [(2, 3), (3, 3), (6, 0)]                                       # (2, 3) again: a removed point's feature may own a new point
    store.append(live[:2], 0)                                             # (6, 0) has no row
    pts = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]]
    got = AR.stage(store, arc, live, pts, 2, -1, live=True)
    assert got["feature"] == [(2, 3), (3, 3), (2, 1), (2, 3), (4, 0), (5, 9)] and got["n"] == 6 and got["n_archived"] == 4 and got["without_row"] == 1
    assert got["points"][:2].tolist() == pts[:2] and got["points"][3].tolist() == [2.0, 1.0, -2.0]
    alone = AR.stage(store, arc, live, pts, 2, -1, live=False)
    assert alone["feature"] == [(2, 1), (2, 3), (4, 0), (5, 9)] and alone["n_archived"] == alone["n"] == 4 and alone["without_row"] == 0


@pytest.fixture(scope="module")
def walk(oracle):
    """-> (the free-running walk of sequence A with the map of every stage of every pair, kp_cap)"""
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
        yield free, NFEAT
    finally:
        oracle.set_dk_early_exit(False)


def _stage3(free):
    return {p: r["stage"][3] for p, r in enumerate(free) if r["evicted"] is not None}


def _end_maps(free, split):
    maps, at = [], 0
    for n in split:
        m = free[at + n - 1]["stage"][4]
        maps.append(dict(frame0=at, pt_feature=[(int(a), int(b)) for a, b in m["pt_feature"]], points=m["points"]))
        at += n
    return maps


def test_on_sequence_a_the_rule_gives_the_map_after_the_limit(walk):
    free, kp_cap = walk
    stage3 = _stage3(free)
    assert sorted(stage3) == [3, 4, 5]
    arc = AR.Archive(-1, N - 1, kp_cap)
    for p in sorted(stage3):
        m3, m4 = stage3[p], free[p]["stage"][4]
        gone = arc.evict(m3, 0, p)
        keep = np.setdiff1d(np.arange(len(m3["points"])), gone)
        assert np.array_equal(m3["pt_feature"][keep], m4["pt_feature"]) and m3["points"][keep].tobytes() == m4["points"].tobytes(), p
        assert len(gone) == free[p]["evicted"]["points_removed"] == AR.EVICTED_A[p], (p, len(gone))
        rounds = sorted(set((gone // 256).tolist()))
        print("pair", p, "map points", len(m3["points"]), "removed", len(gone), "scan rounds with a removed point", rounds)
        assert len(m3["points"]) > 3 * 256 and len(rounds) >= 2           # the removed ranks cross a round of the limit's scan
    a = arc.arrays()
    owners = {f: int((a["feature"][:, 0] == f).sum()) for f in range(N)}
    print("entries", arc.stored, "owned by frame", owners)
    assert arc.stored == 649 and owners == {0: 329, 1: 186, 2: 134, 3: 0, 4: 0, 5: 0, 6: 0}
    # frame-1 points go already at pair 3, where frame 0's camera is evicted: they had two observations, lost one to the filter
    # or have one in the evicted camera, and are left with one
    assert int(((a["evicted_at"] == 3) & (a["feature"][:, 0] == 1)).sum()) >= 1
    # no deduplication is needed on this sequence — which the contract does not promise in general
    assert len(set(arc.feature)) == 649
    assert not set(arc.feature) & {(int(x), int(y)) for x, y in free[-1]["stage"][4]["pt_feature"]}
    assert AR.SMALL_CAPACITY < AR.EVICTED_A[3] + AR.EVICTED_A[4] // 2 and AR.SMALL_CAPACITY > AR.EVICTED_A[3]


@pytest.mark.parametrize("split", AR.SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_on_sequence_a_every_entry_finds_a_row_on_every_split(walk, split):
    free, kp_cap = walk
    stage3, maps = _stage3(free), _end_maps(free, split)
    store, arc, infos = AR.run_split(split, stage3, maps, -1, N - 1, kp_cap)
    assert arc.stored == 649 and arc.dropped == 0 and all(arc.has_row)
    assert infos[-1] == dict(capacity=N * kp_cap, stored=649, dropped=0)
    assert [i["stored"] for i in infos] == sorted(i["stored"] for i in infos)
    whole = AR.run_split((6,), stage3, _end_maps(free, (6,)), -1, N - 1, kp_cap)[1]
    assert arc.feature == whole.feature and arc.evicted_at == whole.evicted_at          # the entries do not depend on the split
    lazy = AR.store_referencing_without_row(split, stage3, maps, N - 1, kp_cap)
    print("split", split, "entries a store-referencing archive would leave without a row:", lazy, "of", arc.stored)
    want = {(6,): 649, (1, 5): 320, (5, 1): 425}
    if split in want:
        assert lazy == want[split]
    # staging: the archived points of frames 0 .. 2 follow the live map's, and a window of the whole flight stages them all
    last = maps[-1]
    got = AR.stage(store, arc, last["pt_feature"], last["points"], 0, None, live=True)
    assert got["n"] == len(last["pt_feature"]) + 649 and got["n_archived"] == 649 and got["without_row"] == 0
    assert AR.stage(store, arc, last["pt_feature"], last["points"], 1, 2, live=False)["n"] == 186


@pytest.mark.parametrize("store_capacity", sorted(AR.STORE_OVERFLOW_WITHOUT_ROW))
def test_the_store_overflow_cases(walk, store_capacity):
    """(2, 2, 2) with a store that overflows.  At the existing tests' 1000 rows the store fills inside the second call and the points
    it drops are owned by frames the flight does not evict from before it ends: the rule leaves NO entry without a row there.  At
    500 rows — fewer than the 610 points of the first call's end map — it drops points of frames 0 .. 2, and entries lose their rows."""
    free, kp_cap = walk
    split = SR.OVERFLOW_SPLIT
    stage3, maps = _stage3(free), _end_maps(free, split)
    store, arc, infos = AR.run_split(split, stage3, maps, -1, N - 1, kp_cap, store_capacity=store_capacity)
    a = arc.arrays()
    without = int((~a["has_row"]).sum())
    print("store", store.info(), "entries without a row", without, "of", arc.stored, "by pair", [int(((~a["has_row"]) & (a["evicted_at"] == p)).sum()) for p in (3, 4, 5)])
    assert store.stored == store_capacity and store.dropped > 0
    assert arc.stored == 649 and without == AR.STORE_OVERFLOW_WITHOUT_ROW[store_capacity]
    keep, w = arc.stage()
    assert len(keep) + w == 649 and w == without
    if store_capacity == 500:
        assert len(maps[0]["pt_feature"]) == 610 and without > 0
        # an entry of a frame-2 point removed in the call it was born in has its row from the slots, whatever the store dropped
        assert bool(a["has_row"][(a["evicted_at"] == 3) & (a["feature"][:, 0] == 2)].all())

"""GPU: vo_slam_stream (FrontEnd.slam_stream) — the resident map carried from one call to the next — against vo_slam_chain on
the whole flight.  All comparisons are exact: the same device functions run on the same lists in the same order, and a tolerance
would hide the one thing these tests look for, a key that went to the wrong place at a carry.

Sequence A of tests/test_gpu_slam_chains.py: synth.sequence(7, 640, 480, step=4.0) / 1000 features / max_cameras = 4, 6 pairs
(tests/test_slam_chains_reference.py pins on the CPU that every pair localises and that pairs 3, 4 and 5 evict a camera).  The
yardstick (`whole`) is slam_chain on the 6 pairs with all 7 frames resident.  The stream runs on a FrontEnd with FEWER SLOTS THAN
FRAMES: 4, or one more than the pairs of the longest chunk where that is more (a chunk of 5 pairs needs its 6 frames resident for
its one vo_pairs_run); every chunk's new frames go into the slots the chunk before freed, the anchor slot is kept."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
import slam_stream_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
PER_PAIR = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")
SPLITS = [(3, 3), (1, 5), (5, 1), (4, 2), (2, 2, 2)]
DEAD_ROOT_NORM = 8.0


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _copy(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


class Run:
    def __init__(self):
        from visual_odometry_amd import synth
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        self.K, self.frames = seq["K"], seq["frames"]
        self.blank = np.full_like(self.frames[0], 127)
        self.fes, self.whole_cache, self.stream_cache = {}, {}, {}

    def fe(self, slots):
        from visual_odometry_amd.frontend import FrontEnd
        if slots not in self.fes:
            self.fes[slots] = dict(fe=FrontEnd(H, W, max_frames=slots, max_pairs=N - 1, nfeatures=NFEAT), resident=None)
        return self.fes[slots]

    def frame(self, f, blank):
        return self.blank if f == blank else self.frames[f]

    def pair_results(self, fe, pairs):
        """run_pairs(want_points) of these pairs; what the chain reads of every pair, copied"""
        res, X = fe.run_pairs(pairs, self.K, want_points=True)
        n = len(pairs)
        got = []
        for p in range(n):
            qi, ti, d, mask = fe.pair_matches(p)
            n_inl = int((mask > 0).sum())
            got.append(dict(res=res[p].copy(), q=qi, t=ti, d=d, mask=mask, X=X[p][:, :n_inl].copy() if res[p]["status"] == 0 else None))
        return got

    def whole_resident(self, blank=None):
        """the 7-slot FrontEnd with all frames resident and the run of the 6 pairs as the latest run_pairs"""
        h = self.fe(N); fe = h["fe"]
        if h["resident"] != ("whole", blank):
            fe.upload(np.stack([self.frame(f, blank) for f in range(N)])); fe.detect(0, N)
            h["pairs"] = self.pair_results(fe, [[k, k + 1] for k in range(N - 1)])
            h["resident"] = ("whole", blank)
        return h

    def whole(self, snapshot=None, blank=None, **opts):
        """slam_chain on all 6 pairs, 7 slots -> dict(out, map, snap, pairs)"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (snapshot, blank, tuple(sorted(opts.items())))
        if key not in self.whole_cache:
            h = self.whole_resident(blank); fe = h["fe"]
            out = fe.slam_chain(N - 1, self.K, snapshot=snapshot, **opts)
            self.whole_cache[key] = dict(out=_copy(out), map=fe.slam_map(0), snap=fe.slam_map(1) if snapshot is not None else None, pairs=h["pairs"])
        return self.whole_cache[key]

    def stream(self, split, snapshot=None, blank=None, cached=True, **opts):
        """slam_stream over the chunks of `split` with real slot reuse.  snapshot = (chunk, pair, stage).
        -> list of dict(out, map, snap, pairs, frame0, slots) per call"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (tuple(split), snapshot, blank, tuple(sorted(opts.items())))
        if cached and key in self.stream_cache:
            return self.stream_cache[key]
        n_slots = max(4, max(split) + 1)
        assert n_slots < N or len(split) == 1                          # fewer slots than frames: slots are reused
        h = self.fe(n_slots); fe = h["fe"]; h["resident"] = None
        free, slot_of, calls, at = list(range(n_slots)), {}, [], 0
        for c, n in enumerate(split):
            for f in range(at + (c > 0), at + n + 1):                   # the anchor (frame `at` of a later chunk) stays where it is
                slot_of[f] = free.pop(0)
                fe.upload(self.frame(f, blank)[None], first_slot=slot_of[f]); fe.detect(slot_of[f], 1)
            pairs = [[slot_of[at + j], slot_of[at + j + 1]] for j in range(n)]
            got = self.pair_results(fe, pairs)
            snap = (snapshot[1], snapshot[2]) if snapshot is not None and snapshot[0] == c else None
            out = fe.slam_stream(n, self.K, resume=c > 0, total_pairs=sum(split), snapshot=snap, **opts)
            calls.append(dict(out=_copy(out), map=fe.slam_map(0), snap=fe.slam_map(1) if snap is not None else None, pairs=got, frame0=at,
                              slots=[slot_of[at + j] for j in range(n + 1)]))
            for f in range(at, at + n):                                 # every frame but the chunk's last gives its slot back
                free.append(slot_of.pop(f))
            free.sort()
            at += n
        if cached:
            self.stream_cache[key] = calls
        return calls


@pytest.fixture(scope="module")
def run():
    return Run()


def _premise(whole, calls):
    """A pair's vo_pairs_run result does not depend on the slots its frames are in, on how its frames were uploaded and detected, or
    on the other pairs of the run: every chunk's pair results are the whole run's."""
    for c in calls:
        for j, got in enumerate(c["pairs"]):
            want = whole["pairs"][c["frame0"] + j]
            assert got["res"]["status"] == want["res"]["status"], (c["frame0"], j)
            for k in ("q", "t", "d", "mask"):
                assert np.array_equal(got[k], want[k]), (c["frame0"], j, k)
            if want["res"]["status"] == 0:
                for k in want["res"].dtype.names:
                    if k != "reserved":
                        assert np.asarray(got["res"][k]).tobytes() == np.asarray(want["res"][k]).tobytes(), (c["frame0"], j, k)
                assert got["X"].tobytes() == want["X"].tobytes(), (c["frame0"], j)


def _latest_poses(calls, n_frames):
    """per stream frame the latest report of `poses`, from a call's own rows or its carried rows"""
    out = np.zeros((n_frames, 3, 4))
    for c in calls:
        o = c["out"]
        for f, T in zip(o["carried_frame"], o["carried_poses"]):
            out[int(f)] = T
        for j, T in enumerate(o["poses"]):
            out[c["frame0"] + j] = T
    return out


def _check_split(whole, calls):
    want, outs = whole["out"], [c["out"] for c in calls]
    for k in PER_PAIR:
        got = np.concatenate([o[k] for o in outs])
        assert got.shape == want[k].shape and got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    pnp = np.concatenate([outs[0]["poses_pnp"]] + [o["poses_pnp"][1:] for o in outs[1:]])
    assert pnp.shape == want["poses_pnp"].shape and np.array_equal(pnp, want["poses_pnp"])
    for a, b in zip(outs[:-1], outs[1:]):
        assert np.array_equal(b["poses_pnp"][0], a["poses_pnp"][-1])    # the anchor as it entered the map
    assert len(outs[0]["carried_frame"]) == 0 and outs[0]["carried_poses"].shape == (0, 3, 4)
    for prev, c in zip(calls[:-1], calls[1:]):                          # the carried cameras: the map at the carry without the anchor, in order
        before, o = prev["map"]["cam_frame"], c["out"]
        assert o["carried_frame"].dtype == np.int32 and o["carried_frame"].tolist() == before.tolist()[:-1] and before[-1] == c["frame0"]
    assert np.array_equal(_latest_poses(calls, len(want["poses"])), want["poses"])
    _same(whole["map"], calls[-1]["map"], S.MAP_KEYS, "final map")


def test_a_stream_of_one_call_is_slam_chain(run):
    whole = run.whole()
    calls = run.stream((6,))
    _premise(whole, calls)
    _same(whole["out"], calls[0]["out"], PER_PAIR + ("poses_pnp", "poses"))
    assert set(calls[0]["out"]) == set(whole["out"]) | {"carried_frame", "carried_poses"}
    _same(whole["map"], calls[0]["map"], S.MAP_KEYS, "final map")
    assert whole["out"]["status"].tolist() == [0] * 6 and whole["out"]["n_cam"].tolist() == [2, 3, 4, 4, 4, 4]
    for stage in (1, 2, 3, 4):
        w = run.whole(snapshot=(4, stage))
        s = run.stream((6,), snapshot=(0, 4, stage))
        _same(w["snap"], s[0]["snap"], S.MAP_KEYS, ("snapshot", stage))
        _same(w["map"], s[0]["map"], S.MAP_KEYS, ("final map", stage))
        _same(whole["out"], s[0]["out"], PER_PAIR + ("poses_pnp", "poses"))
    assert len(run.whole(snapshot=(4, 2))["snap"]["cam_frame"]) == 5     # pair 4 evicts: the stages differ


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_a_split_flight_is_the_whole_flight(run, split):
    whole = run.whole()
    calls = run.stream(split)
    _premise(whole, calls)
    _check_split(whole, calls)
    assert whole["map"]["cam_frame"].tolist() == [3, 4, 5, 6] and whole["out"]["n_cam"].tolist() == [2, 3, 4, 4, 4, 4]
    used = [s for c in calls for s in c["slots"][1:]] + calls[0]["slots"][:1]
    assert len(used) == N and len(set(used)) < N                       # some slot held two frames of the flight


def test_a_carried_camera_that_is_still_free_moves(run):
    whole = run.whole(free_cameras=3)
    calls = run.stream((3, 3), free_cameras=3)
    _premise(whole, calls)
    _check_split(whole, calls)
    first, second = calls[0]["out"], calls[1]["out"]
    assert second["carried_frame"].tolist() == [0, 1, 2]
    # frame 2 is one of the last three cameras at pair 3: the bundle adjustment of the second call moves it
    assert np.array_equal(second["carried_poses"][2], whole["out"]["poses"][2])
    assert not np.array_equal(second["carried_poses"][2], first["poses"][2])
    assert np.array_equal(second["carried_poses"][0], first["poses"][0])           # frame 0 is fixed, and evicted at pair 3


def test_a_dead_root_becomes_a_ghost(run):
    """max_point_norm = 8.0 (default 50): chosen with tests/slam_reference.py on the CPU, where it skips 1 inlier of pair 1 and 20
    of pair 2 at src/visual_slam.py:177 and every pair still localises.  At the carry of the 3 + 3 split 20 anchor keypoints then
    have a track root that owns no map point (dead roots), and the second chunk adds points under such tracks (both counts are
    recomputed here from the whole run's snapshots and matches and must be >= 1; on an MI355X they are 20 and 13).  Were a
    dead-rooted anchor keypoint left as its own root, the first of those points would be found by the pairs after it
    (tests/test_slam_stream_reference.py pins that on the CPU)."""
    opts = dict(max_point_norm=DEAD_ROOT_NORM)
    whole = run.whole(**opts)
    assert whole["out"]["status"].tolist() == [0] * 6
    snaps = [run.whole(snapshot=(p, 1), **opts)["snap"] for p in range(N - 1)]
    matches = [(pr["q"][pr["mask"] > 0], pr["t"][pr["mask"] > 0]) for pr in whole["pairs"]]
    dead, added = R.dead_root_counts(snaps, matches, carry_pair=2)
    print("dead-rooted anchor keypoints at the carry:", dead, " points added under them afterwards:", added)
    assert dead >= 1 and added >= 1, (dead, added)
    calls = run.stream((3, 3), **opts)
    _premise(whole, calls)
    _check_split(whole, calls)
    assert not np.array_equal(whole["out"]["n_pts"], run.whole()["out"]["n_pts"])   # the bound does skip something


def test_a_snapshot_in_a_resumed_call(run):
    plain = run.stream((3, 3))
    for stage in (1, 2, 3, 4):
        want = run.whole(snapshot=(4, stage))["snap"]
        calls = run.stream((3, 3), snapshot=(1, 1, stage))
        _same(want, calls[1]["snap"], S.MAP_KEYS, stage)
        for a, b in zip(plain, calls):                                  # the snapshot does not alter any output
            _same(a["out"], b["out"], PER_PAIR + ("poses_pnp", "poses", "carried_frame", "carried_poses"), stage)
            _same(a["map"], b["map"], S.MAP_KEYS, stage)
    assert len(run.whole(snapshot=(4, 2))["snap"]["cam_frame"]) == 5 and len(run.whole(snapshot=(4, 4))["snap"]["cam_frame"]) == 4


def test_a_lost_stream_ends_and_cannot_be_continued(run):
    from visual_odometry_amd import _lib
    whole = run.whole(blank=5)
    calls = run.stream((3, 3), blank=5, cached=False)
    _premise(whole, calls)
    _check_split(whole, calls)
    failed = int(whole["pairs"][4]["res"]["status"])
    assert failed != 0 and whole["out"]["status"].tolist() == [0, 0, 0, 0, failed, _lib.VO_ERR_NOT_CONFIGURED]
    assert calls[1]["out"]["status"].tolist() == [0, failed, _lib.VO_ERR_NOT_CONFIGURED] and np.all(calls[1]["out"]["poses"][2:] == 0)
    fe = run.fe(4)["fe"]                                                # the stream FrontEnd of the 3 + 3 split, its last call lost
    anchor = calls[1]["slots"][-1]
    other = [s for s in range(4) if s != anchor][0]
    fe.upload(run.frames[0][None], first_slot=other); fe.detect(other, 1)
    fe.run_pairs([[anchor, other]], run.K, want_points=True)
    with pytest.raises(_lib.VoError) as e:
        fe.slam_stream(1, run.K, resume=True, max_cameras=MAX_CAMERAS)
    assert e.value.code == _lib.VO_ERR_INVALID


def test_refusals():
    from visual_odometry_amd import _lib, synth
    from visual_odometry_amd.frontend import FrontEnd, MATCH_RATIO
    seq = synth.sequence(4, 640, 480, cache_dir="/tmp")
    K, frames = seq["K"], seq["frames"]
    c = _lib.Context(0)
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=3, nfeatures=500, ctx=c)
    fe.upload(frames); fe.detect(0, 4)

    def start(total=3):
        fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
        out = fe.slam_stream(2, K, total_pairs=total)
        assert out["status"].tolist() == [0, 0] and len(out["carried_frame"]) == 0
        fe.run_pairs([[2, 3]], K, want_points=True)                     # the anchor is slot 2

    def refused(code=_lib.VO_ERR_INVALID, n=1, **kw):
        with pytest.raises(_lib.VoError) as e:
            fe.slam_stream(n, kw.pop("K", K), resume=True, **kw)
        assert e.value.code == code, (e.value.code, code, kw)
        with pytest.raises(_lib.VoError):
            fe.slam_map(0)                                              # a refused call leaves no map to read

    fe.run_pairs([[0, 1]], K, want_points=True)
    refused()                                                           # there is no stream
    start(); good = fe.slam_stream(1, K, resume=True)                   # what a good resume gives ...
    assert good["status"].tolist() == [0] and good["carried_frame"].tolist() == [0, 1]
    start(); refused(free_cameras=3); refused(max_point_norm=49.0); refused(seed=5); refused(K=K * 1.0001)   # a changed option, a changed K
    again = fe.slam_stream(1, K, resume=True, snapshot=(0, 1))          # ... a refused resume leaves the stream as it was; the snapshot may differ
    for k in good:
        assert np.array_equal(good[k], again[k]), k
    start(); fe.run_pairs([[1, 3]], K, want_points=True); refused()     # pair 0 does not start at the anchor
    start(); fe.run_pairs([[2, 3], [3, 2]], K, want_points=True); refused(n=2)   # a later pair uses the anchor slot: not a chain of distinct frames
    start(); fe.upload(frames[2][None], first_slot=2); fe.detect(2, 1)  # the same frame again, but the host cannot know that
    fe.run_pairs([[2, 3]], K, want_points=True); refused()
    start(); fe.detect(1, 2); fe.run_pairs([[2, 3]], K, want_points=True); refused()      # a detection that covers the anchor slot
    start(total=2); refused()                                           # 2 + 1 pairs pass total_pairs = 2
    fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
    with pytest.raises(_lib.VoError) as e:
        fe.slam_stream(2, K, total_pairs=1)                             # ... and so does the first call alone
    assert e.value.code == _lib.VO_ERR_INVALID
    start(); fe.run_pairs([[2, 3]], K, opts=fe.make_opts(match_mode=MATCH_RATIO, want_points=True)); refused(_lib.VO_ERR_UNSUPPORTED)
    start(); fe.run_pairs([[2, 3]], K, want_points=True)
    assert fe.slam_chain(1, K)["status"].tolist() == [0]                # slam_chain drops the stream
    refused()
    start(); fe.run_pairs([[2, 3]], K, want_points=True)
    assert fe.slam_chains([1], K)[0]["status"].tolist() == [0]          # ... and so does slam_chains
    refused()
    start()
    fe2 = FrontEnd(480, 640, max_frames=4, max_pairs=3, nfeatures=500, ctx=c)   # a configure call on the same context
    fe2.upload(frames); fe2.detect(0, 4); fe2.run_pairs([[2, 3]], K, want_points=True)
    with pytest.raises(_lib.VoError):
        fe2.slam_stream(1, K, resume=True)
    fe2.run_pairs([[0, 1], [1, 2], [2, 3]], K, want_points=True)        # after all that a fresh stream works, and equals slam_chain
    a = fe2.slam_stream(3, K); ma = fe2.slam_map(0)
    b = fe2.slam_chain(3, K); mb = fe2.slam_map(0)
    _same(a, b, PER_PAIR + ("poses_pnp", "poses")); _same(ma, mb, S.MAP_KEYS)
    c.close()


def test_call_equals_call(run):
    a = run.stream((2, 2, 2), cached=False)
    b = run.stream((2, 2, 2), cached=False)
    for x, y in zip(a, b):
        _same(x["out"], y["out"], PER_PAIR + ("poses_pnp", "poses", "carried_frame", "carried_poses"))
        _same(x["map"], y["map"], S.MAP_KEYS)


def test_switches_off_is_localize_chain(run):
    off = dict(ba_iterations=0, filter_threshold=0.0, max_cameras=N)
    whole = run.whole()
    lc = run.whole_resident()["fe"].localize_chain(N - 1, run.K)
    assert lc["status"].tolist() == [0] * 6
    calls = run.stream((2, 2, 2), **off)
    _premise(whole, calls)
    outs = [c["out"] for c in calls]
    pnp = np.concatenate([outs[0]["poses_pnp"]] + [o["poses_pnp"][1:] for o in outs[1:]])
    assert np.array_equal(pnp, lc["poses"]) and np.array_equal(_latest_poses(calls, N), lc["poses"])
    for k in ("n_corr", "n_inl", "status"):
        assert np.array_equal(np.concatenate([o[k] for o in outs]), lc[k]), k
    assert np.array_equal(np.concatenate([o["n_pts"] for o in outs]), lc["n_map"])
    assert np.concatenate([o["n_cam"] for o in outs]).tolist() == list(range(2, N + 1))
    assert not np.concatenate([o["chi2"] for o in outs]).any()
    assert calls[2]["out"]["carried_frame"].tolist() == [0, 1, 2, 3]

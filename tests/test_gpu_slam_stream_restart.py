"""GPU: vo_slam_stream_restart (FrontEnd.slam_stream_restart) — the stream whose map restarts after a lost frame — against
vo_slam_chains_restart with S = 1 (FrontEnd.slam_chain(restart=True)) on the whole flight with every frame resident.  All
comparisons are exact (array_equal on bytes): a tolerance would hide a key or a state word that went to the wrong place at a carry.

The flights of tests/test_gpu_slam_restart.py, cut from synth.sequence(7, 640, 480, step=4.0) / 1000 features / max_cameras = 4
(tests/test_slam_restart_reference.py pins their segment tables on the CPU oracle, tests/test_slam_stream_restart_reference.py
that walking them in chunks changes nothing):
  L  frames 0, 1, 2, 3, blank (127), 2, 3, 4, 5, 6   9 pairs: 0-2 segment 0, 3 and 4 fail on their own, 5-8 segment 1 (evicts at pair 8)
  A  frames 0..6                                     6 pairs, never fails with default options; reproj_err = 1e-9: every pair >= 1
                                                     starts a segment (VO_ERR_NO_MODEL); max_point_norm = 1e-6, max_cameras = 3: the
                                                     map runs dry and pair 3 restarts with VO_ERR_TOO_FEW
The stream runs on a FrontEnd with max(4, longest chunk + 1) slots — fewer than the flight's frames unless the flight is one
chunk — and reuses slots for real: every chunk's new frames go into the slots the chunk before freed, the anchor slot is kept.
The premise, asserted first in every case: a pair's vo_pairs_run result does not depend on the slots of its frames or on the other
pairs of the run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
PER_PAIR = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")
SHARED = PER_PAIR + ("poses_pnp", "poses", "carried_frame", "carried_poses")
SEG_KEYS = ("segment", "cause", "seg_poses_pnp", "seg_poses")
FLIGHTS = dict(L=[0, 1, 2, 3, None, 2, 3, 4, 5, 6], A=[0, 1, 2, 3, 4, 5, 6])          # None: a blank frame (127)
L_SPLITS = [(9,), (3, 6), (4, 5), (5, 4), (6, 3), (2, 2, 2, 3), (4, 1, 4)]
NO_MODEL = dict(reproj_err=1e-9)
TOO_FEW = dict(max_point_norm=1e-6, max_cameras=3)


def _ids(splits):
    return ["+".join(map(str, s)) for s in splits]


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _copy(d):
    return {k: (v if isinstance(v, list) else np.array(v, copy=True)) for k, v in d.items()}


class Run:
    """FrontEnds by slot count, built once; the yardstick (slam_chain(restart=True), every frame resident) and the stream runs,
    cached by flight, split, snapshot and options."""

    def __init__(self):
        from visual_odometry_amd import synth
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        self.K, self.frames = seq["K"], seq["frames"]
        self.blank = np.full_like(self.frames[0], 127)
        self.fes, self.whole_cache, self.stream_cache = {}, {}, {}

    def fe(self, slots):
        from visual_odometry_amd.frontend import FrontEnd
        if slots not in self.fes:
            self.fes[slots] = dict(fe=FrontEnd(H, W, max_frames=slots, max_pairs=slots - 1, nfeatures=NFEAT), resident=None)
        return self.fes[slots]

    def frame(self, flight, f):
        k = FLIGHTS[flight][f]
        return self.blank if k is None else self.frames[k]

    def pair_results(self, fe, pairs):
        """run_pairs(want_points) of these pairs; what the chain reads of every pair, copied"""
        res, X = fe.run_pairs(pairs, self.K, want_points=True)
        got = []
        for p in range(len(pairs)):
            qi, ti, d, mask = fe.pair_matches(p)
            n_inl = int((mask > 0).sum())
            got.append(dict(res=res[p].copy(), q=qi, t=ti, d=d, mask=mask, X=X[p][:, :n_inl].copy() if res[p]["status"] == 0 else None))
        return got

    def whole(self, flight, snapshot=None, **opts):
        """the yardstick: slam_chain(restart=True) on all pairs of the flight, all frames resident -> dict(out, map, snap, pairs)"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (flight, snapshot, tuple(sorted(opts.items())))
        if key not in self.whole_cache:
            n = len(FLIGHTS[flight])
            h = self.fe(n); fe = h["fe"]
            if h["resident"] != ("whole", flight):
                fe.upload(np.stack([self.frame(flight, f) for f in range(n)])); fe.detect(0, n)
                h["pairs"] = self.pair_results(fe, [[k, k + 1] for k in range(n - 1)])
                h["resident"] = ("whole", flight)
            out = fe.slam_chain(n - 1, self.K, snapshot=snapshot, restart=True, **opts)
            self.whole_cache[key] = dict(out=_copy(out), map=fe.slam_map(0), snap=fe.slam_map(1) if snapshot is not None else None, pairs=h["pairs"])
        return self.whole_cache[key]

    def stream(self, flight, split, snapshot=None, cached=True, restart=True, **opts):
        """slam_stream_restart (restart=False: slam_stream) over the chunks of `split` with real slot reuse.
        snapshot = (chunk, pair, stage).  -> list of dict(out, map, snap, pairs, frame0, slots) per call"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (flight, tuple(split), snapshot, restart, tuple(sorted(opts.items())))
        if cached and key in self.stream_cache:
            return self.stream_cache[key]
        n_frames = len(FLIGHTS[flight])
        assert sum(split) == n_frames - 1
        n_slots = max(4, max(split) + 1)
        assert n_slots < n_frames or len(split) == 1                   # fewer slots than frames: slots are reused
        h = self.fe(n_slots); fe = h["fe"]; h["resident"] = None
        free, slot_of, calls, at = list(range(n_slots)), {}, [], 0
        for c, n in enumerate(split):
            for f in range(at + (c > 0), at + n + 1):                   # the anchor (frame `at` of a later chunk) stays where it is
                slot_of[f] = free.pop(0)
                fe.upload(self.frame(flight, f)[None], first_slot=slot_of[f]); fe.detect(slot_of[f], 1)
            pairs = [[slot_of[at + j], slot_of[at + j + 1]] for j in range(n)]
            got = self.pair_results(fe, pairs)
            snap = (snapshot[1], snapshot[2]) if snapshot is not None and snapshot[0] == c else None
            call = fe.slam_stream_restart if restart else fe.slam_stream
            out = call(n, self.K, resume=c > 0, total_pairs=sum(split), snapshot=snap, **opts)
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
    """every chunk's pair results are the whole run's"""
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


def _join_is_whole(whole, calls, what=""):
    """join_stream of the calls equals the yardstick in every key.  The yardstick's dict holds seg_poses_pnp / seg_poses as the
    first rows of `segments`; outside the pairs that start a segment both are zeros by contract."""
    from visual_odometry_amd.frontend import join_stream, split_segments
    want = whole["out"]
    got = join_stream([c["out"] for c in calls])
    assert set(got) == (set(want) - {"segments"}) | {"seg_poses_pnp", "seg_poses"}, what
    _same(want, got, PER_PAIR + ("poses_pnp", "poses", "segment", "cause"), what)
    segs = split_segments(got["segment"], got["poses_pnp"], got["poses"], got["seg_poses_pnp"], got["seg_poses"])
    assert [(s["first_pair"], s["n_pairs"]) for s in segs] == [(s["first_pair"], s["n_pairs"]) for s in want["segments"]], what
    for a, b in zip(segs, want["segments"]):
        _same(a, b, ("poses_pnp", "poses"), (what, a["first_pair"]))
    starts = {s["first_pair"] for s in segs}
    for p in range(len(got["segment"])):
        if p not in starts:
            assert not got["seg_poses_pnp"][p].any() and not got["seg_poses"][p].any(), (what, p)
    # a resumed call's row 0 is the row the call before ended with, in both arrays
    for a, b in zip(calls[:-1], calls[1:]):
        assert np.array_equal(b["out"]["poses_pnp"][0], a["out"]["poses_pnp"][-1]), what
    return got


def _maps_are_the_yardsticks(run, flight, whole, calls, **opts):
    """after every call vo_slam_map(0) is the yardstick's snapshot at that call's last pair, stage 4; the last one is its final map"""
    for c in calls:
        last = c["frame0"] + len(c["pairs"]) - 1
        _same(run.whole(flight, snapshot=(last, 4), **opts)["snap"], c["map"], S.MAP_KEYS, ("map after pair", last))
    _same(whole["map"], calls[-1]["map"], S.MAP_KEYS, "final map")


def _carried_is_the_map_at_the_carry(calls):
    """the carried cameras: the map at the carry in order, without the anchor if it is a camera of the map"""
    assert len(calls[0]["out"]["carried_frame"]) == 0 and calls[0]["out"]["carried_poses"].shape == (0, 3, 4)
    for prev, c in zip(calls[:-1], calls[1:]):
        before = prev["map"]["cam_frame"].tolist()
        want = before[:-1] if before and before[-1] == c["frame0"] else before
        assert c["out"]["carried_frame"].dtype == np.int32 and c["out"]["carried_frame"].tolist() == want


@pytest.mark.parametrize("split", [(3, 3), (2, 2, 2)], ids=_ids([(3, 3), (2, 2, 2)]))
def test_a_flight_that_never_fails_is_slam_stream(run, split):
    whole = run.whole("A")
    on, off = run.stream("A", split), run.stream("A", split, restart=False)
    _premise(whole, on); _premise(whole, off)
    for a, b in zip(on, off):
        _same(a["out"], b["out"], SHARED, "shared outputs")
        assert set(a["out"]) == set(b["out"]) | set(SEG_KEYS)
        _same(a["map"], b["map"], S.MAP_KEYS, "map after the call")
        assert not a["out"]["segment"].any() and not a["out"]["cause"].any() and a["out"]["status"].tolist() == [0] * len(a["pairs"])
    _join_is_whole(whole, on)
    _maps_are_the_yardsticks(run, "A", whole, on)


@pytest.mark.parametrize("split", L_SPLITS, ids=_ids(L_SPLITS))
def test_a_lost_stretch_in_a_stream(run, split):
    whole = run.whole("L")
    calls = run.stream("L", split)
    _premise(whole, calls)
    failed = [int(whole["pairs"][p]["res"]["status"]) for p in (3, 4)]
    assert failed[0] != 0 and failed[1] != 0
    assert whole["out"]["status"].tolist() == [0, 0, 0, failed[0], failed[1], 0, 0, 0, 0]
    assert whole["out"]["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1] and whole["out"]["cause"].tolist() == [0, 0, 0, 0, 0, failed[0], 0, 0, 0]
    assert whole["out"]["n_cam"].tolist() == [2, 3, 4, 4, 4, 2, 3, 4, 4]                  # segment 1 evicts at its last pair
    got = _join_is_whole(whole, calls, split)
    assert got["seg_poses"][0].any() and got["seg_poses"][5].any() and got["seg_poses_pnp"][5].any()
    _maps_are_the_yardsticks(run, "L", whole, calls)
    _carried_is_the_map_at_the_carry(calls)
    for c in calls:                                                     # while lost: segment 0's map, in stream indices
        if c["frame0"] + len(c["pairs"]) in (4, 5):
            assert c["map"]["cam_frame"].tolist() == [0, 1, 2, 3] and c["out"]["segment"][-1] == -1
    assert whole["map"]["cam_frame"].tolist() == [6, 7, 8, 9] and whole["map"]["pt_feature"][:, 0].min() >= 5
    if len(split) > 1:
        used = [s for c in calls for s in c["slots"][1:]] + calls[0]["slots"][:1]
        assert len(used) == 10 and len(set(used)) < 10                  # some slot held two frames of the flight
    if split == (4, 1, 4):                                              # call 1 is the failing pair 4 alone: the whole call is lost
        o = calls[1]["out"]
        assert len(o["carried_frame"]) == 4 and o["carried_frame"].tolist() == [0, 1, 2, 3]
        _same(dict(p=o["carried_poses"]), dict(p=calls[0]["map"]["cam_pose"]), ("p",), "segment 0's four cameras")
        assert not o["poses"].any() and not o["poses_pnp"].any() and o["segment"].tolist() == [-1] and o["status"].tolist() == [failed[1]]
        assert calls[2]["out"]["carried_frame"].tolist() == [0, 1, 2, 3] and calls[2]["out"]["cause"].tolist() == [failed[0], 0, 0, 0]
    if split == (6, 3):                                                 # segment 1's first camera (frame 5) is a carried camera of call 1
        assert calls[1]["out"]["carried_frame"].tolist() == [5] and not calls[1]["out"]["seg_poses"].any()
        assert np.array_equal(calls[1]["out"]["carried_poses"][0], got["seg_poses"][5])
    if split == (5, 4):                                                 # pair 0 of call 1 starts segment 1 on the anchor
        o = calls[1]["out"]
        assert o["segment"].tolist() == [1, 1, 1, 1] and o["cause"][0] == failed[0] and o["seg_poses"][0].any() and not o["poses"][0].any()
        assert o["carried_frame"].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("split", [(3, 3), (1, 5), (2, 2, 2)], ids=_ids([(3, 3), (1, 5), (2, 2, 2)]))
def test_a_restart_at_every_pair_in_a_stream(run, split):
    """rule 2 at pair 0 of every resumed call: the restart happens in the same step, on a carried map that is not empty"""
    from visual_odometry_amd import _lib
    whole = run.whole("A", **NO_MODEL)
    calls = run.stream("A", split, **NO_MODEL)
    _premise(whole, calls)
    got = _join_is_whole(whole, calls, split)
    assert got["segment"].tolist() == [0, 1, 2, 3, 4, 5] and got["cause"].tolist() == [0] + [_lib.VO_ERR_NO_MODEL] * 5
    assert got["status"].tolist() == [0] * 6
    _maps_are_the_yardsticks(run, "A", whole, calls, **NO_MODEL)
    _carried_is_the_map_at_the_carry(calls)
    for prev, c in zip(calls[:-1], calls[1:]):
        assert len(prev["map"]["points"]) > 0 and len(c["out"]["carried_frame"]) == 1 and c["out"]["segment"][0] == c["frame0"]


@pytest.mark.parametrize("split", [(3, 3), (4, 2)], ids=_ids([(3, 3), (4, 2)]))
def test_a_map_that_runs_dry_in_a_stream(run, split):
    from visual_odometry_amd import _lib
    whole = run.whole("A", **TOO_FEW)
    calls = run.stream("A", split, **TOO_FEW)
    _premise(whole, calls)
    got = _join_is_whole(whole, calls, split)
    assert got["segment"].tolist() == [0, 0, 0, 1, 1, 1] and got["cause"].tolist() == [0, 0, 0, _lib.VO_ERR_TOO_FEW, 0, 0]
    _maps_are_the_yardsticks(run, "A", whole, calls, **TOO_FEW)
    _carried_is_the_map_at_the_carry(calls)
    if split == (3, 3):                                                 # pair 0 of the resumed call; its carried map has cameras but no points
        assert len(calls[0]["map"]["cam_frame"]) == 3 and len(calls[0]["map"]["points"]) == 0 and calls[1]["out"]["segment"].tolist() == [1, 1, 1]
    else:                                                               # call 0's last pair; segment 1's first camera is then a carried one
        assert calls[0]["out"]["segment"].tolist() == [0, 0, 0, 1] and calls[1]["out"]["carried_frame"].tolist() == [3]


def test_snapshots_in_a_resumed_call(run):
    plain = run.stream("L", (5, 4))
    for pair, stages in ((0, (1, 2, 3, 4)), (3, (4,))):                 # the restart pair (stream pair 5); the eviction (stream pair 8)
        for stage in stages:
            want = run.whole("L", snapshot=(5 + pair, stage))["snap"]
            calls = run.stream("L", (5, 4), snapshot=(1, pair, stage))
            _same(want, calls[1]["snap"], S.MAP_KEYS, (pair, stage))
            for a, b in zip(plain, calls):                              # the snapshot does not alter any output
                _same(a["out"], b["out"], SHARED + SEG_KEYS, (pair, stage))
                _same(a["map"], b["map"], S.MAP_KEYS, (pair, stage))
    assert len(run.whole("L", snapshot=(5, 1))["snap"]["cam_frame"]) == 2 and run.whole("L", snapshot=(5, 1))["snap"]["cam_frame"].tolist() == [5, 6]


def test_call_equals_call(run):
    a = run.stream("L", (4, 5), cached=False)
    b = run.stream("L", (4, 5), cached=False)
    for x, y in zip(a, b):
        _same(x["out"], y["out"], SHARED + SEG_KEYS)
        _same(x["map"], y["map"], S.MAP_KEYS)


def test_switches_off(run):
    off = dict(ba_iterations=0, filter_threshold=0.0, max_cameras=10)
    whole = run.whole("L", **off)
    calls = run.stream("L", (4, 5), **off)
    _premise(whole, calls)
    got = _join_is_whole(whole, calls, "switches off")
    assert got["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1] and not got["chi2"].any()
    assert got["n_cam"].tolist() == [2, 3, 4, 4, 4, 2, 3, 4, 5]
    _same(whole["map"], calls[-1]["map"], S.MAP_KEYS, "final map")


def test_refusals():
    from visual_odometry_amd import _lib, synth
    from visual_odometry_amd.frontend import FrontEnd, MATCH_RATIO
    seq = synth.sequence(4, 640, 480, cache_dir="/tmp")
    K, frames = seq["K"], seq["frames"]
    blank = np.full_like(frames[0], 127)
    c = _lib.Context(0)
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=3, nfeatures=500, ctx=c)
    fe.upload(frames); fe.detect(0, 4)
    entry = {True: fe.slam_stream_restart, False: fe.slam_stream}

    def start(restart=True, total=3):
        fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
        out = entry[restart](2, K, total_pairs=total)
        assert out["status"].tolist() == [0, 0] and len(out["carried_frame"]) == 0
        fe.run_pairs([[2, 3]], K, want_points=True)                     # the anchor is slot 2

    def refused(restart=True, code=_lib.VO_ERR_INVALID, n=1, **kw):
        with pytest.raises(_lib.VoError) as e:
            entry[restart](n, kw.pop("K", K), resume=True, **kw)
        assert e.value.code == code, (e.value.code, code, kw)
        with pytest.raises(_lib.VoError):
            fe.slam_map(0)                                              # a refused call leaves no map to read

    fe.run_pairs([[0, 1]], K, want_points=True)
    refused()                                                           # there is no stream at all
    good = {}
    for restart in (True, False):                                       # what a good resume gives ...
        start(restart); good[restart] = entry[restart](1, K, resume=True)
        assert good[restart]["status"].tolist() == [0] and good[restart]["carried_frame"].tolist() == [0, 1]
    assert good[True]["segment"].tolist() == [0] and good[True]["cause"].tolist() == [0]
    _same(good[True], good[False], SHARED)
    for restart in (True, False):                                       # ... the other entry point is refused and leaves the stream as it was
        start(restart); refused(not restart)
        again = entry[restart](1, K, resume=True)
        _same(good[restart], again, tuple(good[restart]))
    start(); refused(free_cameras=3); refused(K=K * 1.0001)             # a changed option, a changed K
    _same(good[True], fe.slam_stream_restart(1, K, resume=True, snapshot=(0, 1)), tuple(good[True]))
    start(); fe.run_pairs([[1, 3]], K, want_points=True); refused()     # pair 0 does not start at the anchor
    start(); fe.upload(frames[2][None], first_slot=2); fe.detect(2, 1)  # the anchor slot re-uploaded
    fe.run_pairs([[2, 3]], K, want_points=True); refused()
    start(total=2); refused()                                           # 2 + 1 pairs pass total_pairs = 2
    start(); fe.run_pairs([[2, 3]], K, opts=fe.make_opts(match_mode=MATCH_RATIO, want_points=True)); refused(code=_lib.VO_ERR_UNSUPPORTED)
    fe.run_pairs([[2, 3]], K, want_points=True)                         # the run with ratio matches left the stream continuable
    _same(good[True], fe.slam_stream_restart(1, K, resume=True), tuple(good[True]))
    # a call that ended lost: vo_slam_stream still refuses to go on, vo_slam_stream_restart goes on
    fe.upload(blank[None], first_slot=2); fe.detect(2, 1)
    for restart in (False, True):
        fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
        out = entry[restart](2, K, total_pairs=3)
        assert out["status"][0] == 0 and out["status"][1] != 0
        fe.run_pairs([[2, 3]], K, want_points=True)
        if not restart:
            refused(False); refused(True)                               # lost, and the other entry point
        else:
            nxt = fe.slam_stream_restart(1, K, resume=True)             # blank -> frame 3 fails too: the stream stays lost, and continuable
            assert nxt["status"][0] != 0 and nxt["segment"].tolist() == [-1] and nxt["carried_frame"].tolist() == [0, 1]
            assert fe.slam_map(0)["cam_frame"].tolist() == [0, 1]
            fe.upload(frames[:2], first_slot=0); fe.detect(0, 2)        # slots 0 and 1 are free: frames 0 and 1 again, after frame 3
            fe.run_pairs([[3, 0], [0, 1]], K, want_points=True)
            with pytest.raises(_lib.VoError):
                fe.slam_stream_restart(2, K, resume=True)               # 2 + 1 + 2 pairs pass total_pairs = 3
    c.close()

"""GPU: vo_slam_streams (FrontEnd.slam_streams) — several restart streams carried from call to call in one call each — against
vo_slam_chains_restart with S = 1 (FrontEnd.slam_chain(restart=True)) on every whole flight with all its frames resident, and
against vo_slam_stream_restart on the same chunking.  All comparisons are exact (array_equal, shape and dtype): a tolerance would
hide a key, a state word or a row of a shared table that went to the wrong sequence.

The flights of tests/test_gpu_slam_stream_restart.py, cut from synth.sequence(7, 640, 480, step=4.0) / 1000 features /
max_cameras = 4:
  L   frames 0, 1, 2, 3, blank (127), 2, 3, 4, 5, 6   9 pairs: 0-2 segment 0, 3 and 4 fail on their own, 5-8 segment 1 (evicts at pair 8)
  L6  L's first 7 frames                               6 pairs
  A   frames 0..6                                      6 pairs, never fails with default options (evicts from pair 3 on)
  X, Y  frames 0..3 and 3..6                           3 pairs each (the refusals)
The streams run on a FrontEnd with fewer slots than the flights have frames in total, handed out from ONE free list shared by the
sequences: a frame takes a slot the other sequence gave back whenever there is one, and every case asserts that this happened.
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
FLIGHTS = dict(L=[0, 1, 2, 3, None, 2, 3, 4, 5, 6], L6=[0, 1, 2, 3, None, 2, 3], A=[0, 1, 2, 3, 4, 5, 6], X=[0, 1, 2, 3], Y=[3, 4, 5, 6])
NO_MODEL = dict(reproj_err=1e-9)
TOO_FEW = dict(max_point_norm=1e-6, max_cameras=3)


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _copy(d):
    return {k: (v if k == "segments" else [np.array(x, copy=True) for x in v] if isinstance(v, list) else np.array(v, copy=True)) for k, v in d.items()}


class Run:
    """FrontEnds by slot count, built once; the yardstick (slam_chain(restart=True), every frame resident), the single streams and
    the multi-streams, cached by flights, splits, snapshot and options."""

    def __init__(self):
        from visual_odometry_amd import synth
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        self.K, self.frames = seq["K"], seq["frames"]
        self.blank = np.full_like(self.frames[0], 127)
        self.fes, self.whole_cache, self.single_cache, self.streams_cache = {}, {}, {}, {}

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

    def resident(self, flight):
        """the FrontEnd that holds every frame of the flight, its pairs run"""
        n = len(FLIGHTS[flight])
        h = self.fe(n); fe = h["fe"]
        if h["resident"] != ("whole", flight):
            fe.upload(np.stack([self.frame(flight, f) for f in range(n)])); fe.detect(0, n)
            h["pairs"] = self.pair_results(fe, [[k, k + 1] for k in range(n - 1)])
            h["resident"] = ("whole", flight)
        return h

    def whole(self, flight, snapshot=None, **opts):
        """the yardstick: slam_chain(restart=True) on all pairs of the flight, all frames resident -> dict(out, map, snap, pairs)"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (flight, snapshot, tuple(sorted(opts.items())))
        if key not in self.whole_cache:
            h = self.resident(flight); fe = h["fe"]
            out = fe.slam_chain(len(FLIGHTS[flight]) - 1, self.K, snapshot=snapshot, restart=True, **opts)
            self.whole_cache[key] = dict(out=_copy(out), map=fe.slam_map(0), snap=fe.slam_map(1) if snapshot is not None else None, pairs=h["pairs"])
        return self.whole_cache[key]

    def single(self, flight, split, **opts):
        """slam_stream_restart over the chunks of `split` with slot reuse -> list of dict(out, map) per call"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (flight, tuple(split), tuple(sorted(opts.items())))
        if key not in self.single_cache:
            n_slots = max(4, max(split) + 1)
            h = self.fe(n_slots); fe = h["fe"]; h["resident"] = None
            free, slot_of, calls, at = list(range(n_slots)), {}, [], 0
            for c, n in enumerate(split):
                for f in range(at + (c > 0), at + n + 1):
                    slot_of[f] = free.pop(0)
                    fe.upload(self.frame(flight, f)[None], first_slot=slot_of[f]); fe.detect(slot_of[f], 1)
                fe.run_pairs([[slot_of[at + j], slot_of[at + j + 1]] for j in range(n)], self.K, want_points=True)
                out = fe.slam_stream_restart(n, self.K, resume=c > 0, total_pairs=sum(split), **opts)
                calls.append(dict(out=_copy(out), map=fe.slam_map(0)))
                for f in range(at, at + n):
                    free.append(slot_of.pop(f))
                free.sort()
                at += n
            self.single_cache[key] = calls
        return self.single_cache[key]

    def streams(self, order, splits, snapshot=None, cached=True, **opts):
        """slam_streams over the calls of `splits` (one tuple of pairs-per-call for every flight of `order`, 0 = idle in that call)
        on one slot pool.  snapshot = (call, seq, pair, stage).
        -> list of dict(out, maps [S], map0, snap, pairs [S] lists, frame0 [S], handoffs [(slot, from, to)]) per call"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (tuple(order), tuple(map(tuple, splits)), snapshot, tuple(sorted(opts.items())))
        if cached and key in self.streams_cache:
            return self.streams_cache[key]
        n_seq, n_calls = len(order), len(splits[0])
        assert all(len(sp) == n_calls and sum(sp) == len(FLIGHTS[f]) - 1 and sp[0] > 0 for f, sp in zip(order, splits))
        need = [sum(sp[c] + (c == 0) for sp in splits) + (n_seq if c else 0) for c in range(n_calls)]
        n_slots = max(need)
        assert n_slots < sum(len(FLIGHTS[f]) for f in order) or n_calls == 1            # fewer slots than frames: slots are reused
        h = self.fe(n_slots); fe = h["fe"]; h["resident"] = None
        free, last_owner, slot_of, at, calls = list(range(n_slots)), {}, [dict() for _ in order], [0] * n_seq, []
        for c in range(n_calls):
            lengths = [sp[c] for sp in splits]
            pairs, handoffs = [], []
            for s, n in enumerate(lengths):
                for f in range(at[s] + (at[s] > 0), at[s] + n + 1 if n else 0):      # the anchor stays where it is
                    slot = next((x for x in free if last_owner.get(x, s) != s), free[0])   # a slot the other sequence gave back, if any
                    free.remove(slot)
                    if last_owner.get(slot, s) != s:
                        handoffs.append((slot, last_owner[slot], s))
                    last_owner[slot] = s; slot_of[s][f] = slot
                    fe.upload(self.frame(order[s], f)[None], first_slot=slot); fe.detect(slot, 1)
                pairs += [[slot_of[s][at[s] + j], slot_of[s][at[s] + j + 1]] for j in range(n)]
            got = self.pair_results(fe, pairs)
            snap = snapshot[1:] if snapshot is not None and snapshot[0] == c else None
            out = fe.slam_streams(lengths, self.K, resume=c > 0, total_pairs=[sum(sp) for sp in splits], snapshot=snap, **opts)
            off = np.concatenate([[0], np.cumsum(lengths)])
            calls.append(dict(out=_copy(out), maps=[fe._slam_chains_map(s, 0) for s in range(n_seq)], map0=fe.slam_map(0),
                              snap=fe.slam_map(1, seq=snap[0]) if snap is not None else None,
                              pairs=[got[off[s]:off[s + 1]] for s in range(n_seq)], frame0=list(at), handoffs=handoffs))
            for s, n in enumerate(lengths):
                for f in range(at[s], at[s] + n):                           # every frame but the sequence's last gives its slot back
                    free.append(slot_of[s].pop(f))
                at[s] += n
            free.sort()
        if cached:
            self.streams_cache[key] = calls
        return calls


@pytest.fixture(scope="module")
def run():
    return Run()


def _premise(run, order, calls, **opts):
    """every call's pair results are the whole runs' of their flights"""
    for c in calls:
        for s, flight in enumerate(order):
            whole = run.whole(flight, **opts)
            for j, got in enumerate(c["pairs"][s]):
                want = whole["pairs"][c["frame0"][s] + j]
                assert got["res"]["status"] == want["res"]["status"], (flight, c["frame0"][s], j)
                for k in ("q", "t", "d", "mask"):
                    assert np.array_equal(got[k], want[k]), (flight, c["frame0"][s], j, k)
                if want["res"]["status"] == 0:
                    for k in want["res"].dtype.names:
                        if k != "reserved":
                            assert np.asarray(got["res"][k]).tobytes() == np.asarray(want["res"][k]).tobytes(), (flight, j, k)
                    assert got["X"].tobytes() == want["X"].tobytes(), (flight, c["frame0"][s], j)


def _join_is_whole(whole, got, what=""):
    """a joined flight equals the yardstick in every key (its seg_poses rows are the first rows of `segments`)"""
    from visual_odometry_amd.frontend import split_segments
    want = whole["out"]
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


def _flights_are_the_yardsticks(run, order, calls, **opts):
    """for every sequence: join_streams equals the yardstick; the map after every call is the yardstick's snapshot at the
    sequence's last pair so far, stage 4 (after an idle call: unchanged); the carried rows are the map at the carry; an idle
    sequence owns its anchor's pose row and reports nothing else"""
    from visual_odometry_amd.frontend import join_streams, stream_slice
    joined = join_streams([c["out"] for c in calls])
    assert len(joined) == len(order)
    for s, flight in enumerate(order):
        what = (order, flight)
        _join_is_whole(run.whole(flight, **opts), joined[s], what)
        prev = None
        for c in calls:
            sl = stream_slice(c["out"], s)
            n = len(sl["status"])
            assert n == len(c["pairs"][s]) and c["out"]["n_carried"][s] == len(sl["carried_frame"])
            done = c["frame0"][s] + n
            _same(run.whole(flight, snapshot=(done - 1, 4), **opts)["snap"], c["maps"][s], S.MAP_KEYS, (what, "map after pair", done - 1))
            if prev is not None:
                assert np.array_equal(sl["poses_pnp"][0], prev["sl"]["poses_pnp"][-1]), what
                if n == 0:                                                  # idle: one row in each pose array, unchanged; nothing carried
                    assert sl["poses_pnp"].shape == (1, 3, 4) and np.array_equal(sl["poses"][0], prev["sl"]["poses"][-1]), what
                    assert len(sl["carried_frame"]) == 0 and sl["carried_poses"].shape == (0, 3, 4), what
                    _same(prev["map"], c["maps"][s], S.MAP_KEYS, (what, "idle map"))
                else:
                    before = prev["map"]["cam_frame"].tolist()
                    want = before[:-1] if before and before[-1] == c["frame0"][s] else before
                    assert sl["carried_frame"].dtype == np.int32 and sl["carried_frame"].tolist() == want, what
            else:
                assert len(sl["carried_frame"]) == 0
            prev = dict(sl=sl, map=c["maps"][s])
        _same(run.whole(flight, **opts)["map"], calls[-1]["maps"][s], S.MAP_KEYS, (what, "final map"))
    for c in calls:                                                         # vo_slam_map reports sequence 0
        _same(c["map0"], c["maps"][0], S.MAP_KEYS, "vo_slam_map")
    return joined


def _slots_changed_hands(calls):
    """a slot one sequence freed was taken next by another"""
    moves = [(c, h) for c, call in enumerate(calls) for h in call["handoffs"]]
    assert moves, "no slot changed hands"
    return moves


def test_one_sequence_is_slam_stream_restart(run):
    from visual_odometry_amd.frontend import stream_slice
    multi, single = run.streams(("L",), ((4, 5),)), run.single("L", (4, 5))
    _premise(run, ("L",), multi)
    for c, (a, b) in enumerate(zip(multi, single)):
        sl = stream_slice(a["out"], 0)
        assert set(sl) == set(b["out"])
        _same(sl, b["out"], tuple(b["out"]), ("call", c))
        _same(a["maps"][0], b["map"], S.MAP_KEYS, ("map after call", c))
        _same(a["map0"], b["map"], S.MAP_KEYS, ("vo_slam_map after call", c))
    _flights_are_the_yardsticks(run, ("L",), multi)


def test_two_flights_on_one_slot_pool(run):
    from visual_odometry_amd.frontend import stream_slice
    la = run.streams(("L", "A"), ((3, 3, 3), (2, 2, 2)))
    _premise(run, ("L", "A"), la)
    joined = _flights_are_the_yardsticks(run, ("L", "A"), la)
    assert joined[0]["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1] and joined[1]["segment"].tolist() == [0] * 6
    assert joined[0]["n_cam"].tolist() == [2, 3, 4, 4, 4, 2, 3, 4, 4] and joined[1]["n_cam"].tolist() == [2, 3, 4, 4, 4, 4]
    moves = _slots_changed_hands(la)
    assert {(h[1], h[2]) for _, h in moves} == {(0, 1), (1, 0)}              # in both directions
    # listed the other way round, on other slots: every sequence's bytes are the same
    al = run.streams(("A", "L"), ((2, 2, 2), (3, 3, 3)))
    _premise(run, ("A", "L"), al)
    _flights_are_the_yardsticks(run, ("A", "L"), al)
    _slots_changed_hands(al)
    for c, (x, y) in enumerate(zip(la, al)):
        for s in (0, 1):
            a, b = stream_slice(x["out"], s), stream_slice(y["out"], 1 - s)
            _same(a, b, SHARED + SEG_KEYS, ("call", c, "sequence", s))
            _same(x["maps"][s], y["maps"][1 - s], S.MAP_KEYS, ("map after call", c, "sequence", s))


def test_a_sequence_that_ends_early_is_idle(run):
    order = ("L", "A")
    calls = run.streams(order, ((4, 5), (6, 0)))
    _premise(run, order, calls)
    _flights_are_the_yardsticks(run, order, calls)
    _same(calls[0]["maps"][1], calls[1]["maps"][1], S.MAP_KEYS, "A's map after the idle call")
    assert calls[1]["out"]["seq_off"].tolist() == [0, 5, 5] and calls[1]["out"]["n_carried"].tolist()[1] == 0
    assert any(h[1] == 1 and h[2] == 0 for h in calls[1]["handoffs"])        # L went on in slots A gave back


def test_a_sequence_idle_in_the_middle_goes_on(run):
    order = ("A", "L")
    calls = run.streams(order, ((2, 0, 4), (3, 3, 3)))
    _premise(run, order, calls)
    _flights_are_the_yardsticks(run, order, calls)
    assert calls[1]["out"]["seq_off"].tolist() == [0, 0, 3]
    assert any(h[1] == 0 and h[2] == 1 for h in calls[1]["handoffs"])        # during the idle call L uses a slot the idle A gave back
    assert any(h[1] == 1 and h[2] == 0 for h in calls[2]["handoffs"])        # and A goes on in slots L had in between


@pytest.mark.parametrize("opts", [NO_MODEL, TOO_FEW], ids=["no_model", "too_few"])
def test_restarts_in_the_same_step_on_carried_maps(run, opts):
    from visual_odometry_amd import _lib
    order = ("L6", "A")
    calls = run.streams(order, ((3, 3), (3, 3)), **opts)
    _premise(run, order, calls, **opts)
    joined = _flights_are_the_yardsticks(run, order, calls, **opts)
    _slots_changed_hands(calls)
    if opts is NO_MODEL:                                                    # every pair >= 1 of A restarts, also pair 0 of the resumed call
        assert joined[1]["segment"].tolist() == [0, 1, 2, 3, 4, 5] and joined[1]["cause"].tolist() == [0] + [_lib.VO_ERR_NO_MODEL] * 5
        assert joined[0]["segment"].tolist()[:3] == [0, 1, 2] and joined[0]["segment"][5] >= 0
    else:                                                                   # A's map runs dry: pair 3 = pair 0 of the resumed call restarts
        assert joined[1]["segment"].tolist() == [0, 0, 0, 1, 1, 1] and joined[1]["cause"].tolist() == [0, 0, 0, _lib.VO_ERR_TOO_FEW, 0, 0]
        assert len(calls[0]["maps"][1]["cam_frame"]) == 3 and len(calls[0]["maps"][1]["points"]) == 0


def test_one_sequence_lost_across_a_call_while_the_other_lives(run):
    from visual_odometry_amd.frontend import stream_slice
    order = ("L", "A")
    calls = run.streams(order, ((4, 1, 4), (2, 2, 2)))
    _premise(run, order, calls)
    joined = _flights_are_the_yardsticks(run, order, calls)
    _slots_changed_hands(calls)
    failed = [int(run.whole("L")["pairs"][p]["res"]["status"]) for p in (3, 4)]
    o = stream_slice(calls[1]["out"], 0)                                    # L's call 1 is the failing pair 4 alone: lost from end to end
    assert o["carried_frame"].tolist() == [0, 1, 2, 3] and not o["poses"].any() and o["segment"].tolist() == [-1] and o["status"].tolist() == [failed[1]]
    assert stream_slice(calls[1]["out"], 1)["status"].tolist() == [0, 0]    # ... beside A's two good pairs
    assert stream_slice(calls[2]["out"], 0)["cause"].tolist() == [failed[0], 0, 0, 0] and joined[0]["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1]


def test_snapshots_of_the_second_sequence_in_a_resumed_call(run):
    from visual_odometry_amd.frontend import stream_slice
    order, splits = ("L", "A"), ((3, 3, 3), (2, 2, 2))
    plain = run.streams(order, splits)
    assert stream_slice(plain[1]["out"], 1)["n_cam"].tolist() == [4, 4]      # A's pair 3 (pair 1 of call 1) evicts
    for pair, stage in ((0, 1), (1, 4)):
        want = run.whole("A", snapshot=(2 + pair, stage))["snap"]
        calls = run.streams(order, splits, snapshot=(1, 1, pair, stage))
        _same(want, calls[1]["snap"], S.MAP_KEYS, (pair, stage))
        for a, b in zip(plain, calls):                                      # the snapshot does not alter any output
            for s in (0, 1):
                _same(stream_slice(a["out"], s), stream_slice(b["out"], s), SHARED + SEG_KEYS, (pair, stage))
                _same(a["maps"][s], b["maps"][s], S.MAP_KEYS, (pair, stage))
    assert len(run.whole("A", snapshot=(3, 4))["snap"]["cam_frame"]) == 4 and len(run.whole("A", snapshot=(2, 1))["snap"]["cam_frame"]) == 4


def test_call_equals_call(run):
    from visual_odometry_amd.frontend import stream_slice
    a = run.streams(("L", "A"), ((4, 5), (3, 3)), cached=False)
    b = run.streams(("L", "A"), ((4, 5), (3, 3)), cached=False)
    for x, y in zip(a, b):
        for s in (0, 1):
            _same(stream_slice(x["out"], s), stream_slice(y["out"], s), SHARED + SEG_KEYS)
            _same(x["maps"][s], y["maps"][s], S.MAP_KEYS)


def test_switches_off(run):
    """no bundle adjustment, no filter, no eviction: every segment of every flight is vo_tracks_pnp_batch on its pairs"""
    off = dict(ba_iterations=0, filter_threshold=0.0, max_cameras=10)
    order = ("L", "A")
    calls = run.streams(order, ((4, 5), (3, 3)), **off)
    _premise(run, order, calls, **off)
    joined = _flights_are_the_yardsticks(run, order, calls, **off)
    assert joined[0]["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1] and joined[0]["n_cam"].tolist() == [2, 3, 4, 4, 4, 2, 3, 4, 5]
    from visual_odometry_amd.frontend import split_segments
    for s, flight in enumerate(order):
        got = joined[s]
        assert not got["chi2"].any()
        for sg in split_segments(got["segment"], got["poses_pnp"], got["poses"], got["seg_poses_pnp"], got["seg_poses"]):
            a0, n = sg["first_pair"], sg["n_pairs"]
            h = run.resident(flight); fe = h["fe"]
            fe.run_pairs([[a0 + j, a0 + j + 1] for j in range(n)], run.K, want_points=True)
            h["resident"] = None                                            # (the flight's own pairs are no longer the latest run)
            lc = fe.localize_chain(n, run.K)
            assert np.array_equal(sg["poses_pnp"], lc["poses"]) and np.array_equal(sg["poses"], lc["poses"]), (flight, a0)
            for key in ("n_corr", "n_inl", "status"):
                assert np.array_equal(got[key][a0:a0 + n], lc[key]), (flight, a0, key)
            assert np.array_equal(got["n_pts"][a0:a0 + n], lc["n_map"]) and got["n_cam"][a0:a0 + n].tolist() == list(range(2, n + 2)), (flight, a0)


def test_refusals(run):
    """every refusal leaves the stream as it was: after each of them the good call gives the bytes it gives without it, which
    end the flights at the yardsticks' bytes"""
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import MATCH_RATIO, join_streams, stream_slice
    K = run.K
    h = run.fe(8); fe = h["fe"]; h["resident"] = None
    for flight, first in (("X", 0), ("Y", 4)):                              # X in slots 0 .. 3, Y in slots 4 .. 7
        fe.upload(np.stack([run.frame(flight, f) for f in range(4)]), first_slot=first); fe.detect(first, 4)
    opts = dict(max_cameras=MAX_CAMERAS)

    def start():
        fe.run_pairs([[0, 1], [1, 2], [4, 5], [5, 6]], K, want_points=True)
        return fe.slam_streams([2, 2], K, total_pairs=[3, 3], **opts)      # the anchors are slots 2 and 6

    def good():
        fe.run_pairs([[2, 3], [6, 7]], K, want_points=True)
        return fe.slam_streams([1, 1], K, resume=True, **opts)

    def refused(lengths, code=_lib.VO_ERR_INVALID, **kw):
        with pytest.raises(_lib.VoError) as e:
            fe.slam_streams(lengths, kw.pop("K", K), resume=True, **{**opts, **kw})
        assert e.value.code == code, (e.value.code, code, lengths, kw)

    fe.run_pairs([[0, 1]], K, want_points=True)
    fe.slam_chain(1, K)                                                     # (a chain call drops whatever stream there was)
    fe.run_pairs([[2, 3], [6, 7]], K, want_points=True)
    refused([1, 1])                                                         # there is no stream at all
    first = start(); want = good()
    joined = join_streams([first, want])
    for s, flight in enumerate(("X", "Y")):
        _join_is_whole(run.whole(flight), joined[s], flight)

    def then_good(what):
        """... and the stream is as it was: the good call gives the bytes it gives without the refusal"""
        again = good()
        for s in (0, 1):
            _same(stream_slice(want, s), stream_slice(again, s), SHARED + SEG_KEYS, (what, s))

    both = [[2, 3], [6, 7]]
    cases = [("another number of sequences", both, [2], {}), ("another number of sequences", both, [1, 1, 0], {}),
             ("a changed option", both, [1, 1], dict(free_cameras=3)), ("a changed K", both, [1, 1], dict(K=K * 1.0001)),
             ("every sequence idle", both, [0, 0], {}),
             ("the idle sequence's anchor among the other's pairs", [[2, 6]], [1, 0], {}),
             ("the idle sequence's anchor among the other's later pairs", [[2, 3], [3, 6]], [2, 0], {}),
             ("an advancing sequence's anchor among the other's pairs", [[2, 6], [6, 7]], [1, 1], {}),
             ("a pair 0 that does not start at its anchor", [[1, 3], [6, 7]], [1, 1], {}),
             ("a pair 0 that ends at its anchor", [[2, 3], [7, 6]], [1, 1], {}),
             ("2 + 2 pairs pass total_pairs[0] = 3", [[2, 3], [3, 0], [6, 7]], [2, 1], {})]
    for what, pairs, lengths, kw in cases:
        start()
        fe.run_pairs(pairs, K, want_points=True)
        refused(lengths, **kw)
        then_good(what)
    start()
    fe.run_pairs(both, K, opts=fe.make_opts(match_mode=MATCH_RATIO, want_points=True)); refused([1, 1], code=_lib.VO_ERR_UNSUPPORTED)
    then_good("ratio matches")
    start()
    fe.run_pairs([[2, 3]], K, want_points=True)                             # the single-stream entries do not continue a multi-stream
    for entry in (fe.slam_stream_restart, fe.slam_stream):
        with pytest.raises(_lib.VoError) as e:
            entry(1, K, resume=True, **opts)
        assert e.value.code == _lib.VO_ERR_INVALID
    then_good("the single-stream entries")
    # an advancing sequence whose anchor slot was written is refused; the other sequence goes on alone
    start()
    fe.upload(run.frame("X", 2)[None], first_slot=2); fe.detect(2, 1)
    fe.run_pairs([[2, 3], [6, 7]], K, want_points=True); refused([1, 1])
    fe.run_pairs([[6, 7]], K, want_points=True)
    alone = fe.slam_streams([0, 1], K, resume=True, **opts)
    _same(stream_slice(want, 1), stream_slice(alone, 1), SHARED + SEG_KEYS, "Y alone")
    # a multi-stream does not continue a single stream, and leaves it continuable
    fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
    fe.slam_stream_restart(2, K, total_pairs=3, **opts)
    fe.run_pairs([[2, 3]], K, want_points=True)
    refused([1])
    one = fe.slam_stream_restart(1, K, resume=True, **opts)
    _same(stream_slice(want, 0), one, SHARED + SEG_KEYS, "X as a single stream")
    # resume = 0 needs a pair in every sequence
    fe.run_pairs([[0, 1]], K, want_points=True)
    with pytest.raises(_lib.VoError) as e:
        fe.slam_streams([1, 0], K, total_pairs=[3, 3], **opts)
    assert e.value.code == _lib.VO_ERR_INVALID

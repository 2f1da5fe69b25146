"""GPU: seats of a multi-stream (vo_slam_streams_open / vo_slam_streams_replace; FrontEnd.slam_streams_open,
slam_streams_replace, split_flights, flight_pool) — a sequence whose flight has ended takes another one.  The contract is one
equality: for every flight, the calls from the one in which it took its seat to its last compute the bytes slam_stream_restart
computes for that flight alone with the same chunking — every output, the map after every call, the statistics rows — whichever
seat it takes, whatever sat there before, whatever the other seats do.  All comparisons are exact (array_equal, shape, dtype).

The shapes and the harness are tests/test_gpu_slam_streams.py's (synth.sequence(7, 640, 480, step=4.0), 1000 features,
max_cameras = 4); its flights A, L, L6 and three more, which localise every pair (asserted on the yardsticks, so that an all-lost
flight cannot hide anything):
  R    A reversed, frames 6..0    6 pairs, evicts at pairs 3-5
  T    frames 2..6                4 pairs, evicts at pair 3
  U    frames 6..3                3 pairs
  L6c  L6 without its last frame  5 pairs: 0-2 segment 0, 3 and 4 fail — the flight ends lost
Every case runs on a slot pool with fewer slots than frames, handed out from one free list.  A slot a replaced seat's anchor gave
up goes to the next frame that can show something new there: the cases assert that a frame of the seat's new flight landed in such
a slot and that a frame of another seat's flight did.  The premise, asserted first: a pair's vo_pairs_run result does not depend
on the slots of its frames or on the other pairs of the run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
from test_gpu_slam_streams import FLIGHTS, MAX_CAMERAS, SEG_KEYS, SHARED, Run, _copy, _same  # noqa: E402

pytestmark = pytest.mark.gpu

SEAT_FLIGHTS = dict(FLIGHTS, R=[6, 5, 4, 3, 2, 1, 0], T=[2, 3, 4, 5, 6], U=[6, 5, 4, 3], L6c=[0, 1, 2, 3, None, 2])
NEVER_FAIL = ("A", "R", "T", "U")
STATS = ("total_sqerr", "mean_sqerr", "max_sqerr", "n_high", "obs_hist", "obs_matrix", "cam_frame")


class SeatRun(Run):
    """the harness of test_gpu_slam_streams.py on the flights above: the yardstick (slam_stream_restart on one flight alone, with
    its pair results, its statistics rows and a snapshot) and the multi-stream with seats, both cached"""

    def __init__(self):
        super().__init__()
        self.alone_cache, self.seats_cache = {}, {}

    def frame(self, flight, f):
        k = SEAT_FLIGHTS[flight][f]
        return self.blank if k is None else self.frames[k]

    def alone(self, flight, split, snapshot=None, stats=False, **opts):
        """slam_stream_restart over the chunks of `split` with slot reuse; snapshot = (call, pair, stage)
        -> list of dict(out, map, pairs, snap, stats) per call"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (flight, tuple(split), snapshot, stats, tuple(sorted(opts.items())))
        if key in self.alone_cache:
            return self.alone_cache[key]
        assert sum(split) <= len(SEAT_FLIGHTS[flight]) - 1
        n_slots = max(4, max(split) + 1)
        h = self.fe(n_slots); fe = h["fe"]; h["resident"] = None
        fe.map_stats(stats)
        try:
            free, slot_of, calls, at = list(range(n_slots)), {}, [], 0
            for c, n in enumerate(split):
                for f in range(at + (c > 0), at + n + 1):
                    slot_of[f] = free.pop(0)
                    fe.upload(self.frame(flight, f)[None], first_slot=slot_of[f]); fe.detect(slot_of[f], 1)
                got = self.pair_results(fe, [[slot_of[at + j], slot_of[at + j + 1]] for j in range(n)])
                snap = snapshot[1:] if snapshot is not None and snapshot[0] == c else None
                out = fe.slam_stream_restart(n, self.K, resume=c > 0, total_pairs=sum(split), snapshot=snap, **opts)
                calls.append(dict(out=_copy(out), map=fe.slam_map(0), pairs=got, snap=fe.slam_map(1) if snap is not None else None,
                                  stats=fe.slam_stats(0) if stats else None))
                for f in range(at, at + n):
                    free.append(slot_of.pop(f))
                free.sort()
                at += n
        finally:
            fe.map_stats(False)
        self.alone_cache[key] = calls
        return calls

    def seats(self, n_seats, script, n_slots, start="open", capacity=9, snapshot=None, stats=False, cached=True, hooks=None, **opts):
        """A multi-stream of n_seats seats.  script: one (replace, advance) per call — replace: the seats replaced before the call, as
        seat or (seat, bound); advance: {seat: (flight, n)}, a flight name the seat does not hold takes the (vacant) seat.
        start = "open": slam_streams_open first; "resume0": call 0 is slam_streams(resume=False).  snapshot = (call, seat, pair,
        stage).  hooks: {call: fn(fe)} run before that call's replaces.
        -> dict(calls = list of dict(out, maps, snap, stats, pairs {seat: results}) per call,
                flights = per seat the list of (flight, took at call, split), ended = per seat the call before which each flight's
                seat was replaced (the number of calls if never), landed = set of (slot, "new" | "other"))"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (n_seats, repr(script), n_slots, start, capacity, snapshot, stats, tuple(sorted(opts.items())))
        if cached and hooks is None and key in self.seats_cache:
            return self.seats_cache[key]
        h = self.fe(n_slots); fe = h["fe"]; h["resident"] = None
        fe.map_stats(stats)
        try:
            if start == "open":
                fe.slam_streams_open(n_seats, capacity, self.K, **opts)
            free, held, done, anchor = list(range(n_slots)), [None] * n_seats, [0] * n_seats, [None] * n_seats
            vacated, landed, flights, calls, n_frames = {}, set(), [[] for _ in range(n_seats)], [], 0
            ended = [[] for _ in range(n_seats)]
            for c, (replace, advance) in enumerate(script):
                if hooks and c in hooks:
                    hooks[c](fe)
                for r in replace:
                    s, bound = r if isinstance(r, tuple) else (r, capacity)
                    fe.slam_streams_replace(s, bound)
                    if held[s] is not None:
                        vacated[anchor[s]] = s; free.append(anchor[s]); free.sort(); ended[s].append(c)
                    held[s], anchor[s], done[s] = None, None, 0
                lengths, pairs, of = [0] * n_seats, [], {}
                for s in range(n_seats):
                    if s not in advance:
                        continue
                    flight, n = advance[s]
                    if held[s] != flight:
                        assert held[s] is None, "a seat is replaced before another flight takes it"
                        held[s] = flight; flights[s].append([flight, c, []])
                    slots = [] if anchor[s] is None else [anchor[s]]
                    for f in range(done[s] + len(slots), done[s] + n + 1):
                        kind = lambda x: "new" if vacated[x] == s else "other"  # noqa: E731
                        slot = next((x for x in free if x in vacated and (x, kind(x)) not in landed), next((x for x in free if x not in vacated), free[0]))
                        free.remove(slot)
                        if slot in vacated:
                            landed.add((slot, kind(slot)))
                        slots.append(slot); n_frames += 1
                        fe.upload(self.frame(flight, f)[None], first_slot=slot); fe.detect(slot, 1)
                    of[s] = (len(pairs), n, slots)
                    pairs += [[slots[j], slots[j + 1]] for j in range(n)]
                    lengths[s] = n; flights[s][-1][2].append(n)
                got = self.pair_results(fe, pairs)
                snap = snapshot[1:] if snapshot is not None and snapshot[0] == c else None
                if c == 0 and start == "resume0":
                    out = fe.slam_streams(lengths, self.K, total_pairs=[capacity] * n_seats, snapshot=snap, **opts)
                else:
                    out = fe.slam_streams(lengths, self.K, resume=True, snapshot=snap, **opts)
                calls.append(dict(out=_copy(out), maps=[fe._slam_chains_map(s, 0) for s in range(n_seats)],
                                  snap=fe.slam_map(1, seq=snap[0]) if snap is not None else None,
                                  stats=[fe.slam_stats(s) for s in range(n_seats)] if stats else None,
                                  pairs={s: got[a:a + n] for s, (a, n, _) in of.items()}))
                for s, (_, n, slots) in of.items():
                    free += slots[:-1]; anchor[s] = slots[-1]; done[s] += n
                free.sort()
            assert n_slots < n_frames                                       # fewer slots than frames: slots are reused
        finally:
            fe.map_stats(False)
        ended = [e + [len(calls)] * (len(fl) - len(e)) for e, fl in zip(ended, flights)]
        res = dict(calls=calls, flights=[[tuple(f[:2]) + (tuple(f[2]),) for f in fl] for fl in flights], ended=ended, landed=landed)
        if cached and hooks is None:
            self.seats_cache[key] = res
        return res


@pytest.fixture(scope="module")
def run():
    return SeatRun()


def _flights_are_alone(run, res, stats=False, **opts):
    """every flight of every seat, call by call: the premise, every output, the map after each of its calls (and unchanged after a
    call in which it was idle), the statistics rows; then the joined flight.  -> {(seat, flight): joined dict}"""
    from visual_odometry_amd.frontend import join_stream, split_flights, stream_slice
    calls = res["calls"]
    per_seat = split_flights([c["out"] for c in calls], [[f[1] for f in fl] for fl in res["flights"]])
    joined = {}
    for s, fl in enumerate(res["flights"]):
        assert len(per_seat[s]) == len(fl)
        for i, (flight, took, split) in enumerate(fl):
            what = (s, flight, split)
            want = run.alone(flight, split, stats=stats, **opts)
            if flight in NEVER_FAIL:
                assert all((w["out"]["status"] == 0).all() and (w["out"]["segment"] == 0).all() for w in want), what
            last = res["ended"][s][i]                                               # until its seat is replaced, the map is its own
            mine = [c for c in range(took, last) if len(stream_slice(calls[c]["out"], s)["status"]) > 0]
            assert len(mine) == len(split) == len(per_seat[s][i]), what
            for k, c in enumerate(mine):
                for got, w in zip(calls[c]["pairs"][s], want[k]["pairs"]):           # the premise
                    assert got["res"]["status"] == w["res"]["status"], what
                    for key in ("q", "t", "d", "mask"):
                        assert np.array_equal(got[key], w[key]), (what, c, key)
                    if w["res"]["status"] == 0:
                        for key in w["res"].dtype.names:
                            if key != "reserved":
                                assert np.asarray(got["res"][key]).tobytes() == np.asarray(w["res"][key]).tobytes(), (what, c, key)
                        assert got["X"].tobytes() == w["X"].tobytes(), (what, c)
                sl = per_seat[s][i][k]
                assert set(sl) == set(want[k]["out"]), what
                _same(sl, want[k]["out"], tuple(want[k]["out"]), (what, "call", c))
                assert calls[c]["out"]["n_carried"][s] == len(sl["carried_frame"])
                until = mine[k + 1] if k + 1 < len(mine) else last
                for cc in range(c, until):                                           # its own call, then the calls it sits out
                    _same(calls[cc]["maps"][s], want[k]["map"], S.MAP_KEYS, (what, "map after call", cc))
                if stats:
                    _same(calls[c]["stats"][s], want[k]["stats"], STATS, (what, "statistics of call", c))
            a, b = join_stream(per_seat[s][i]), join_stream([w["out"] for w in want])
            assert set(a) == set(b), what
            _same(a, b, tuple(b), (what, "joined"))
            joined[(s, flight)] = a
    return joined


def _starts_from_zero(j):
    assert j["segment"][0] == 0 and j["cause"][0] == 0 and j["status"][0] == 0 and (np.diff(j["segment"]) >= 0).all()


def test_replacement_beside_a_live_seat(run):
    from visual_odometry_amd.frontend import stream_slice
    script = [([], {0: ("L", 3), 1: ("A", 2)}), ([], {0: ("L", 3), 1: ("A", 2)}), ([], {1: ("A", 2)}),
              ([(1, 6)], {0: ("L", 3), 1: ("R", 3)}), ([], {1: ("R", 3)})]
    res = run.seats(2, script, n_slots=9, start="resume0")
    assert res["flights"] == [[("L", 0, (3, 3, 3))], [("A", 0, (2, 2, 2)), ("R", 3, (3, 3))]]
    joined = _flights_are_alone(run, res)
    assert {k for _, k in res["landed"]} == {"new", "other"}, res["landed"]   # R and L both had a frame in the slot A's anchor gave up
    r = joined[(1, "R")]
    _starts_from_zero(r)
    assert r["segment"].tolist() == [0] * 6 and r["n_cam"].tolist() == [2, 3, 4, 4, 4, 4]
    assert res["calls"][3]["out"]["n_carried"].tolist()[1] == 0 and res["calls"][4]["out"]["n_carried"].tolist() == [0, 3]
    assert res["calls"][4]["maps"][1]["cam_frame"].tolist() == [3, 4, 5, 6]  # counted along R, not along the seat
    # L beside A and then R is L beside A alone: the existing (L, A) run's bytes, chunk by chunk
    la = run.streams(("L", "A"), ((3, 3, 3), (2, 2, 2)))
    for mine, theirs in ((0, 0), (1, 1), (3, 2)):
        _same(stream_slice(res["calls"][mine]["out"], 0), stream_slice(la[theirs]["out"], 0), SHARED + SEG_KEYS, ("L", mine))
        _same(res["calls"][mine]["maps"][0], la[theirs]["maps"][0], S.MAP_KEYS, ("L's map", mine))


@pytest.mark.parametrize("before, after", [(("L", (4, 5)), ("U", (2, 1))), (("L6c", (3, 2)), ("T", (2, 2)))], ids=["longer", "lost"])
def test_a_shorter_flight_after_a_longer_one_and_after_a_lost_one(run, before, after):
    (b, bs), (a, as_) = before, after
    script = [([], {0: (b, bs[0]), 1: ("A", 2)}), ([], {0: (b, bs[1]), 1: ("A", 2)}),
              ([(0, sum(as_))], {0: (a, as_[0])}), ([], {0: (a, as_[1]), 1: ("A", 2)})]
    res = run.seats(2, script, n_slots=9)
    assert res["flights"][0] == [(b, 0, bs), (a, 2, as_)]
    joined = _flights_are_alone(run, res)
    assert {k for _, k in res["landed"]} == {"new", "other"}, res["landed"]
    old, new = joined[(0, b)], joined[(0, a)]
    if b == "L":
        assert old["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1] and old["n_cam"].tolist()[-2:] == [4, 4]    # ended with evictions
    else:
        assert old["segment"].tolist() == [0, 0, 0, -1, -1] and (old["status"][3:] != 0).all()                      # ended lost
    _starts_from_zero(new)
    assert new["segment"].tolist() == [0] * sum(as_) and not new["cause"].any()
    assert res["calls"][2]["out"]["n_carried"].tolist()[0] == 0


def test_a_vacant_seat_sits_out(run):
    from visual_odometry_amd.frontend import stream_slice
    script = [([], {0: ("A", 2), 1: ("U", 3)}), ([1], {0: ("A", 2)}), ([(1, 4)], {0: ("A", 2), 1: ("T", 2)}), ([], {1: ("T", 2)})]
    res = run.seats(2, script, n_slots=7)
    assert res["flights"][1] == [("U", 0, (3,)), ("T", 2, (2, 2))]
    joined = _flights_are_alone(run, res)
    assert {k for _, k in res["landed"]} == {"new", "other"}, res["landed"]
    _starts_from_zero(joined[(1, "T")])
    idle = res["calls"][1]
    assert all(len(idle["maps"][1][k]) == 0 for k in S.MAP_KEYS)            # vacant and reset: its map reports empty
    sl = stream_slice(idle["out"], 1)
    assert sl["poses_pnp"].shape == (1, 3, 4) and not sl["poses_pnp"].any() and not sl["poses"].any()
    assert len(sl["status"]) == 0 and idle["out"]["n_carried"].tolist()[1] == 0 and len(sl["carried_frame"]) == 0


def test_both_seats_replaced_before_the_same_call(run):
    script = [([], {0: ("U", 3), 1: ("T", 2)}), ([], {1: ("T", 2)}), ([0, 1], {0: ("R", 3), 1: ("A", 3)}), ([], {0: ("R", 3), 1: ("A", 3)})]
    res = run.seats(2, script, n_slots=8)
    assert res["flights"] == [[("U", 0, (3,)), ("R", 2, (3, 3))], [("T", 0, (2, 2)), ("A", 2, (3, 3))]]
    joined = _flights_are_alone(run, res)
    assert {k for _, k in res["landed"]} == {"new", "other"} and len({x for x, _ in res["landed"]}) == 2, res["landed"]
    _starts_from_zero(joined[(0, "R")]); _starts_from_zero(joined[(1, "A")])


def test_open_is_a_resume0_start(run):
    from visual_odometry_amd.frontend import stream_slice
    script = [([], {0: ("A", 3), 1: ("R", 3)}), ([], {0: ("A", 3), 1: ("R", 3)})]
    opened, started = run.seats(2, script, n_slots=8, capacity=6), run.seats(2, script, n_slots=8, capacity=6, start="resume0")
    _flights_are_alone(run, opened)
    _flights_are_alone(run, started)
    for c, (x, y) in enumerate(zip(opened["calls"], started["calls"])):
        assert x["out"]["seq_off"].tolist() == y["out"]["seq_off"].tolist() and x["out"]["n_carried"].tolist() == y["out"]["n_carried"].tolist()
        for s in (0, 1):
            _same(stream_slice(x["out"], s), stream_slice(y["out"], s), SHARED + SEG_KEYS, ("call", c, "seat", s))
            _same(x["maps"][s], y["maps"][s], S.MAP_KEYS, ("map after call", c, "seat", s))
    # one seat: slam_stream_restart itself, lost frames and all
    one = run.seats(1, [([], {0: ("L", 4)}), ([], {0: ("L", 5)})], n_slots=6)
    j = _flights_are_alone(run, one)[(0, "L")]
    assert j["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1]


def test_statistics_of_a_flight_in_a_reused_seat(run):
    from visual_odometry_amd import _lib
    script = [([], {0: ("A", 3), 1: ("U", 3)}), ([(1, 4)], {0: ("A", 3), 1: ("T", 2)}), ([], {1: ("T", 2)})]
    refused = []

    def other_setting(fe):
        fe.map_stats(False)                                                 # the stream was opened with statistics on
        fe.run_pairs([[0, 1]], run.K, want_points=True)
        with pytest.raises(_lib.VoError) as e:
            fe.slam_streams([0, 1], run.K, resume=True, max_cameras=MAX_CAMERAS)
        refused.append(e.value.code)
        fe.map_stats(True)

    res = run.seats(2, script, n_slots=8, stats=True, hooks={2: other_setting})
    assert refused == [_lib.VO_ERR_INVALID]
    _flights_are_alone(run, res, stats=True)                                # ... and the stream went on to the same bytes
    t = [c["stats"][1] for c in res["calls"][1:]]
    assert t[0]["cam_frame"][0].tolist()[:2] == [0, 1] and t[1]["cam_frame"][-1].tolist() == [1, 2, 3, 4]   # counted along T
    assert len(res["calls"][2]["stats"][0]["total_sqerr"]) == 0              # A was idle in the last call: no rows


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
def test_snapshot_on_a_flights_first_call_in_a_reused_seat(run, stage):
    script = [([], {0: ("A", 2), 1: ("U", 3)}), ([(1, 4)], {0: ("A", 2), 1: ("T", 2)})]
    plain = run.seats(2, script, n_slots=7)
    for pair in (0, 1):
        want = run.alone("T", (2,), snapshot=(0, pair, stage))[0]["snap"]
        got = run.seats(2, script, n_slots=7, snapshot=(1, 1, pair, stage))
        _same(want, got["calls"][1]["snap"], S.MAP_KEYS, (pair, stage))
        assert len(want["cam_frame"]) == 2 + pair and want["cam_frame"][0] == 0
        for a, b in zip(plain["calls"], got["calls"]):                      # the snapshot does not alter any output
            for s in (0, 1):
                _same(a["maps"][s], b["maps"][s], S.MAP_KEYS, (pair, stage))


def test_call_equals_call(run):
    from visual_odometry_amd.frontend import stream_slice
    script = [([], {0: ("L6c", 3), 1: ("A", 3)}), ([], {0: ("L6c", 2), 1: ("A", 3)}), ([0, 1], {0: ("T", 3), 1: ("U", 3)})]
    a, b = run.seats(2, script, n_slots=8, cached=False), run.seats(2, script, n_slots=8, cached=False)
    for x, y in zip(a["calls"], b["calls"]):
        for s in (0, 1):
            _same(stream_slice(x["out"], s), stream_slice(y["out"], s), SHARED + SEG_KEYS)
            _same(x["maps"][s], y["maps"][s], S.MAP_KEYS)


def test_refusals(run):
    """every refusal leaves the stream as it was: the flights still end at the bytes they have alone"""
    from visual_odometry_amd import _lib
    K, opts = run.K, dict(max_cameras=MAX_CAMERAS)

    def refused(fn, *args, **kw):
        with pytest.raises(_lib.VoError) as e:
            fn(*args, **kw)
        assert e.value.code == _lib.VO_ERR_INVALID, (e.value.code, args)

    def before_call_1(fe):                                                  # seats 0 (A) and 1 (U) are held
        for seq, bound in ((-1, 3), (2, 3), (0, 0), (0, 7), (1, -1)):       # seq out of range, total_pairs out of range (capacity 6)
            refused(fe.slam_streams_replace, seq, bound)

    def before_call_2(fe):                                                  # seat 1 is vacant (replaced before call 1), seat 0 holds A
        refused(fe.slam_streams_replace, 1, 7)
        fe.slam_streams_replace(1, 6)                                       # a vacant seat: only the bound
        fe.run_pairs([[0, 1]], K, want_points=True)
        refused(fe.slam_streams, [0, 0], K, resume=True, **opts)            # every seat idle
        refused(fe.slam_streams, [1, 1], K, resume=True, **opts)            # not all the pairs of the run
        fe.slam_streams_replace(1, 4)

    script = [([], {0: ("A", 2), 1: ("U", 3)}), ([1], {0: ("A", 2)}), ([], {0: ("A", 2), 1: ("T", 2)}), ([], {1: ("T", 2)})]
    res = run.seats(2, script, n_slots=7, capacity=6, hooks={1: before_call_1, 2: before_call_2})
    _flights_are_alone(run, res)
    # a new flight's pair 0 may start anywhere but at a slot another sequence holds
    h = run.fe(8); fe = h["fe"]; h["resident"] = None
    fe.upload(np.stack([run.frame("U", f) for f in range(4)]), first_slot=0); fe.detect(0, 4)
    fe.upload(np.stack([run.frame("T", f) for f in range(4)]), first_slot=4); fe.detect(4, 4)
    fe.slam_streams_open(2, 3, K, **opts)
    fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
    first = fe.slam_streams([2, 0], K, resume=True, **opts)                 # U's anchor is slot 2
    fe.run_pairs([[2, 3], [2, 5]], K, want_points=True)
    refused(fe.slam_streams, [1, 1], K, resume=True, **opts)
    fe.run_pairs([[2, 3], [4, 5], [5, 2]], K, want_points=True)
    refused(fe.slam_streams, [1, 2], K, resume=True, **opts)
    fe.run_pairs([[2, 3], [4, 5]], K, want_points=True)
    second = fe.slam_streams([1, 1], K, resume=True, **opts)
    from visual_odometry_amd.frontend import stream_slice
    alone = run.alone("U", (2, 1))
    for got, want in ((first, alone[0]), (second, alone[1])):
        _same(stream_slice(got, 0), want["out"], tuple(want["out"]), "U after the refusals")
    _same(stream_slice(second, 1), run.alone("T", (1,))[0]["out"], SHARED + SEG_KEYS, "T's first pair")
    # no stream at all; a stream of the single kinds, which stays continuable
    fe.run_pairs([[0, 1]], K, want_points=True)
    fe.slam_chain(1, K)                                                     # (a chain call drops whatever stream there was)
    refused(fe.slam_streams_replace, 0, 1)
    fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
    one = fe.slam_stream_restart(2, K, total_pairs=3, **opts)
    refused(fe.slam_streams_replace, 0, 1)
    fe.run_pairs([[2, 3]], K, want_points=True)
    two = fe.slam_stream_restart(1, K, resume=True, **opts)
    for got, want in ((one, alone[0]), (two, alone[1])):
        _same(got, want["out"], tuple(want["out"]), "the single stream after the refusal")
    refused(fe.slam_streams_open, 0, 3, K, **opts)                           # no seats; a capacity of no pairs
    refused(fe.slam_streams_open, 2, [3, 0], K, **opts)


def test_flight_pool(run):
    from visual_odometry_amd.flight_pool import FlightPool, plan_calls
    names = ["A", "U", "R", "T"]
    stacks = [np.stack([run.frame(n, f) for f in range(len(SEAT_FLIGHTS[n]))]) for n in names]
    lengths = [len(s) - 1 for s in stacks]
    h = run.fe(9); fe = h["fe"]; h["resident"] = None
    assert fe.max_frames < sum(len(s) for s in stacks)
    pool = FlightPool(fe, run.K, n_seats=2, chunk=3, capacity=6, max_cameras=MAX_CAMERAS)
    results = pool.run(stacks)
    plan = plan_calls(lengths, 2, 3, fe.max_frames)
    assert pool.plan == plan and len(pool.outs) == len(plan)
    assert pool.seat_of == [0, 1, 1, 0]                                     # U ends first: R takes its seat; T takes A's
    for f, name in enumerate(names):
        seat = next(s for c in plan for s in c["took"] if c["flights"][s] == f)
        assert pool.seat_of[f] == seat
        split = tuple(plan[c]["lengths"][seat] for c in pool.calls_of[f])
        assert sum(split) == lengths[f] and max(split) <= 3
        from visual_odometry_amd.frontend import join_stream
        want = join_stream([w["out"] for w in run.alone(name, split)])
        assert set(results[f]) == set(want), name
        _same(results[f], want, tuple(want), (name, "flight pool"))
        assert (want["status"] == 0).all()

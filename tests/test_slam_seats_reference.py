"""No GPU: the two pure helpers of the seats.  split_flights takes the flights of every seat out of the calls of one slam_streams
stream — against the CPU walkers of tests/test_slam_streams_reference.py: a seat hosts two flights with an idle call between them,
beside a seat whose one flight is idle in the middle; the yardstick is join_stream of each flight walked alone.
flight_pool.plan_calls is held to its properties over a few lists of flight lengths: every frame scheduled once and in order, no
slot with two live frames, an anchor in its slot until its flight advances or ends, no call beyond n_slots or chunk, none all idle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_slam_streams_reference import _pack, _same_dict, walked  # noqa: E402,F401  (walked: the module's fixture)


def _seated(walked):
    """seat 0: A (2 + 4), vacant and idle in call 2, then L (4 + 1 + 4); seat 1: L (4 + 1 + 4) with an idle call in the middle, then vacant"""
    A, L = walked["A"], walked["L"]
    zero = (np.zeros((3, 4)), np.zeros((3, 4)))
    hold = (L[1]["poses_pnp"][-1], L[1]["poses"][-1])
    rows = [[(A[0], None), (L[0], None)], [(A[1], None), (L[1], None)], [(None, zero), (None, hold)],
            [(L[0], None), (L[2], None)], [(L[1], None), (None, zero)], [(L[2], None), (None, zero)]]
    return [_pack(r) for r in rows], [[0, 3], [0]]


def test_split_flights_gives_every_flight_its_calls(walked):
    from visual_odometry_amd.frontend import join_stream, split_flights
    outs, took = _seated(walked)
    flights = split_flights(outs, took)
    assert [len(f) for f in flights] == [2, 1] and [len(c) for c in flights[0]] == [2, 3] and len(flights[1][0]) == 3
    for got, name in ((flights[0][0], "A"), (flights[0][1], "L"), (flights[1][0], "L")):
        for sl, want in zip(got, walked[name]):
            _same_dict(want, sl, name)
        _same_dict(join_stream(walked[name]), join_stream(got), name)
    L = join_stream(flights[0][1])
    assert L["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1] and L["cause"][0] == 0 and len(L["poses"]) == 10
    flights[0][0][0]["poses"][:] = -1
    assert not (split_flights(outs, took)[0][0][0]["poses"] == -1).any()                     # copies


def test_split_flights_refuses_what_is_not_a_schedule(walked):
    from visual_odometry_amd.frontend import split_flights
    outs, took = _seated(walked)
    for bad in ([[0, 3]], [[0, 3], [0], []], [[3, 0], [0]], [[0, 2], [0]], [[0, 6], [0]], [[1, 3], [0]], [[0, 3], []]):
        with pytest.raises(ValueError):
            split_flights(outs, bad)
    with pytest.raises(ValueError):
        split_flights([], [])
    with pytest.raises(ValueError):
        split_flights([outs[0], _pack([(walked["L"][1], None)])], took)                       # another number of sequences


CASES = [([6, 3, 6, 4], 2, 3, 9), ([1], 1, 1, 2), ([5, 1, 1, 1, 7, 2], 3, 2, 12), ([4, 9, 24, 5, 4, 13, 7, 4, 18, 6, 11, 8], 4, 4, 24),
         ([3, 3, 3], 5, 2, 9), ([2, 9], 2, 4, 10)]


@pytest.mark.parametrize("lengths, n_seats, chunk, n_slots", CASES)
def test_plan_calls_properties(lengths, n_seats, chunk, n_slots):
    from visual_odometry_amd.flight_pool import plan_calls
    plan = plan_calls(lengths, n_seats, chunk, n_slots)
    in_slot, anchor, seat_flight, nxt, started = {}, {}, [None] * n_seats, [0] * len(lengths), []
    for c, call in enumerate(plan):
        assert len(call["lengths"]) == len(call["flights"]) == n_seats
        assert sum(call["lengths"]) > 0 and max(call["lengths"]) <= chunk                    # never all idle, never beyond chunk
        for s in call["replace"]:                                                            # a flight that has ended, and only such a one
            f = seat_flight[s]
            assert f is not None and nxt[f] == lengths[f] + 1
            del in_slot[anchor.pop(f)]
            seat_flight[s] = None
        for s in call["took"]:
            assert seat_flight[s] is None
            seat_flight[s] = call["flights"][s]
            started.append(call["flights"][s])
        assert seat_flight == call["flights"]
        assert all((n > 0) == (f is not None) for n, f in zip(call["lengths"], call["flights"]))   # whoever holds a seat advances
        assert all(f is not None for f in call["flights"]) or len(started) == len(lengths)   # a seat is vacant only when no flight waits
        new = {}
        for f, k, slot in call["frames"]:
            assert k == nxt[f] and 0 <= slot < n_slots and slot not in in_slot and slot not in new   # once, in order, in a free slot
            nxt[f] += 1
            new[slot] = (f, k)
        in_slot.update(new)
        assert len(in_slot) <= n_slots
        want = []
        for s, n in enumerate(call["lengths"]):
            f = call["flights"][s]
            if n == 0:
                continue
            first = nxt[f] - n - 1
            slots = [next(x for x, v in in_slot.items() if v == (f, k)) for k in range(first, first + n + 1)]
            if f in anchor:
                assert slots[0] == anchor[f]                                                 # the anchor kept its slot until now
            want += [[slots[j], slots[j + 1]] for j in range(n)]
            for x in slots[:-1]:
                del in_slot[x]
            anchor[f] = slots[-1]
        assert call["pairs"] == want
        assert sorted(in_slot) == sorted(anchor.values())                                    # after a call only the anchors are held
    assert started == list(range(len(lengths))) and nxt == [n + 1 for n in lengths]           # list order; every frame scheduled


def test_plan_calls_raises():
    from visual_odometry_amd.flight_pool import plan_calls
    with pytest.raises(ValueError):
        plan_calls([6, 3, 6, 4], 2, 3, 7)                                                    # call 0 alone needs 8 slots
    for bad in (([], 2, 3, 9), ([3, 0], 2, 3, 9), ([3], 0, 3, 9), ([3], 1, 0, 9)):
        with pytest.raises(ValueError):
            plan_calls(*bad)
    # the step rounds of a pool against waves of n_seats flights, each as long as its longest
    lengths = [4, 9, 24, 5, 4, 13, 7, 4, 18, 6, 11, 8]
    pool = sum(max(c["lengths"]) for c in plan_calls(lengths, 4, 4, 24))
    waves = sum(max(lengths[i:i + 4]) for i in range(0, len(lengths), 4))
    assert pool < waves

"""Many flights of unequal length on the few seats of one slam_streams stream: a seat whose flight has ended takes the next one
that waits (FrontEnd.slam_streams_replace), so no seat idles while flights wait.  plan_calls is the schedule as a pure function;
FlightPool runs it on a FrontEnd.  Every flight's result is what slam_stream_restart computes for that flight alone with the
same chunking, byte for byte — whichever seat it took and whatever sat there before."""
from __future__ import annotations

import numpy as np

from .frontend import join_stream, split_flights


def plan_calls(lengths, n_seats, chunk, n_slots):
    """The calls that walk flights of lengths[f] pairs (lengths[f] + 1 frames) on n_seats seats, `chunk` pairs at most per seat
    and call, on a pool of n_slots frame slots.  Pure: no GPU, no library.
    Flights are taken in list order.  Before a call every seat whose flight is finished is replaced, and a vacant seat takes the
    next waiting flight in that same call; every seat that holds a flight advances by up to `chunk` pairs.  Slots come from one
    free list, lowest first: after a call every slot is free but the anchors — the last frames — of the flights that go on.
    Returns a list with one dict per call:
      lengths  [n_seats] pairs per seat in the call (0: the seat is vacant; it happens only when no flight waits)
      replace  the seats whose flight ended with the call before: slam_streams_replace comes before this call's uploads
      took     the seats a new flight takes in this call
      flights  [n_seats] the flight in every seat during the call, None for a vacant seat
      frames   (flight, frame, slot) for every frame to upload and detect before the call, in the order of the seats
      pairs    the call's pairs as [slot of frame 1, slot of frame 2], sequence after sequence: run_pairs' argument
    ValueError on a bad argument or when n_slots cannot hold a call (the anchors and the call's new frames)."""
    lengths = [int(v) for v in lengths]
    n_seats, chunk, n_slots = int(n_seats), int(chunk), int(n_slots)
    if not lengths or min(lengths) < 1:
        raise ValueError(f"every flight has at least one pair, got {lengths}")
    if n_seats < 1 or chunk < 1:
        raise ValueError(f"n_seats and chunk are at least 1, got {n_seats} and {chunk}")
    waiting = list(range(len(lengths)))
    flight = [None] * n_seats                     # the flight in a seat, pairs of it done, slot of its last frame
    done = [0] * n_seats
    anchor = [None] * n_seats
    free = list(range(n_slots))
    calls = []
    while True:
        replace = [s for s in range(n_seats) if flight[s] is not None and done[s] == lengths[flight[s]]]
        for s in replace:
            free.append(anchor[s])
            flight[s], anchor[s] = None, None
        free.sort()
        if not waiting and all(f is None for f in flight):
            return calls
        took = []
        for s in range(n_seats):
            if flight[s] is None and waiting:
                flight[s], done[s] = waiting.pop(0), 0
                took.append(s)
        call = dict(lengths=[], replace=replace, took=took, flights=list(flight), frames=[], pairs=[])
        given_back = []
        for s in range(n_seats):
            f = flight[s]
            n = 0 if f is None else min(chunk, lengths[f] - done[s])
            call["lengths"].append(n)
            if n == 0:
                continue
            slots = [] if anchor[s] is None else [anchor[s]]
            for k in range(done[s] + len(slots), done[s] + n + 1):
                if not free:
                    raise ValueError(f"{n_slots} slots cannot hold call {len(calls)}: {sum(a is not None for a in anchor)} anchors and its new frames")
                slots.append(free.pop(0))
                call["frames"].append((f, k, slots[-1]))
            call["pairs"] += [[slots[j], slots[j + 1]] for j in range(n)]
            given_back += slots[:-1]
            anchor[s] = slots[-1]
            done[s] += n
        free += given_back
        calls.append(call)


class FlightPool:
    """plan_calls on a FrontEnd: FlightPool(fe, K, n_seats, chunk, capacity, **slam_streams' options).  capacity is the longest
    flight, in pairs, a seat may hold.  fe needs max_frames slots for the plan (n_seats anchors and n_seats * chunk + n_seats new
    frames at most) and max_pairs >= n_seats * chunk."""

    def __init__(self, fe, K, n_seats, chunk, capacity, **options):
        self.fe, self.K = fe, np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        self.n_seats, self.chunk, self.capacity, self.options = int(n_seats), int(chunk), int(capacity), dict(options)
        self.plan, self.outs, self.seat_of, self.calls_of = [], [], [], []

    def run(self, flights):
        """flights: a list of frame stacks [n_f, H, W] (n_f >= 2).  Opens a stream of vacant seats and runs the plan: before every call
        the ended flights' seats are replaced, the call's new frames uploaded and detected, run_pairs, slam_streams(resume=True).
        Returns one whole-flight dict per flight, in list order: join_stream over the flight's calls (split_flights).  Afterwards
        self.plan is the plan, self.outs the calls' dicts, self.seat_of[f] the flight's seat and self.calls_of[f] its calls."""
        fe = self.fe
        lengths = [len(f) - 1 for f in flights]
        if lengths and max(lengths) > self.capacity:
            raise ValueError(f"a flight of {max(lengths)} pairs does not fit a seat of capacity {self.capacity}")
        plan = plan_calls(lengths, self.n_seats, self.chunk, fe.max_frames)
        if max(sum(c["lengths"]) for c in plan) > fe.max_pairs:
            raise ValueError(f"a call of the plan has more pairs than the front end's max_pairs = {fe.max_pairs}")
        fe.slam_streams_open(self.n_seats, self.capacity, self.K, **self.options)
        outs, took_seat = [], [[] for _ in range(self.n_seats)]
        seat_of, calls_of = [None] * len(flights), [[] for _ in flights]
        for c, call in enumerate(plan):
            for s in call["replace"]:
                nxt = call["flights"][s]
                fe.slam_streams_replace(s, self.capacity if nxt is None else lengths[nxt])
            for f, k, slot in call["frames"]:
                fe.upload(flights[f][k][None], first_slot=slot)
                fe.detect(slot, 1)
            fe.run_pairs(call["pairs"], self.K, want_points=True)
            outs.append(fe.slam_streams(call["lengths"], self.K, resume=True, **self.options))
            for s in call["took"]:
                took_seat[s].append(c)
                seat_of[call["flights"][s]] = s
            for s, f in enumerate(call["flights"]):
                if f is not None:
                    calls_of[f].append(c)
        per_seat = split_flights(outs, took_seat)
        order = [[call["flights"][s] for call in plan if s in call["took"]] for s in range(self.n_seats)]
        results = [None] * len(flights)
        for s in range(self.n_seats):
            for f, slices in zip(order[s], per_seat[s]):
                results[f] = join_stream(slices)
        self.plan, self.outs, self.seat_of, self.calls_of = plan, outs, seat_of, calls_of
        return results

#!/usr/bin/env python3
"""Many flights of unequal length on the few seats of one multi-stream: a seat whose flight has ended takes the next one that
waits (FrontEnd.slam_streams_open / slam_streams_replace, flight_pool.FlightPool), so no seat idles while flights wait and the
front end needs frame slots for one call only, not for whole flights.

    python examples/flight_pool.py [--seats 2] [--chunk 3] [--flights 5 3 7 2 4] [--width 640 --height 480]

A handful of synthetic flights — cuts of one seeded flight, some flown backwards; the third one flies through a blank frame and loses
tracking — are walked on fewer seats.  Printed per flight: its seat, the calls it took part in and its segments; then the step
rounds of the pool against those of waves of `seats` flights, each wave as long as its longest flight."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_odometry_amd import synth  # noqa: E402
from visual_odometry_amd.flight_pool import FlightPool, plan_calls  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd, split_segments  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seats", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=3, help="pairs per seat and call at most")
    ap.add_argument("--flights", type=int, nargs="+", default=[5, 3, 7, 2, 4], help="pairs per flight")
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--step", type=float, default=4.0, help="flight distance per frame (the camera is 30 units above the ground)")
    a = ap.parse_args()
    lengths = a.flights
    n = max(lengths) + 1
    seq = synth.sequence(n, a.width, a.height, step=a.step)
    K, frames = seq["K"], seq["frames"]
    flights = []
    for f, m in enumerate(lengths):                             # every other flight is flown backwards, from the far end
        flights.append(frames[:m + 1].copy() if f % 2 == 0 else frames[::-1][:m + 1].copy())
    if len(flights) > 2 and lengths[2] >= 4:
        flights[2][2] = 127                                     # a blank frame: two pairs fail, the flight starts a new map behind them
    S, chunk = a.seats, a.chunk
    slots = S * (chunk + 2)                                     # per seat: an anchor and a call's chunk + 1 new frames at most
    fe = FrontEnd(a.height, a.width, max_frames=slots, max_pairs=S * chunk, nfeatures=1000)
    pool = FlightPool(fe, K, n_seats=S, chunk=chunk, capacity=max(lengths), max_cameras=4)
    results = pool.run(flights)
    print(f"{len(lengths)} flights of {lengths} pairs ({sum(m + 1 for m in lengths)} frames) on {S} seats and {slots} frame slots, {len(pool.plan)} calls of at most "
          f"{chunk} pairs per seat")
    for c, call in enumerate(pool.plan):
        print(f"call {c}: replaced {call['replace']}, flights in the seats {call['flights']}, pairs {call['lengths']}, new frames in slots {[x for _, _, x in call['frames']]}")
    for f, r in enumerate(results):
        segs = split_segments(r["segment"], r["poses_pnp"], r["poses"], r["seg_poses_pnp"], r["seg_poses"])
        print(f"flight {f}: seat {pool.seat_of[f]}, calls {pool.calls_of[f]}, status {r['status'].tolist()}, segment {r['segment'].tolist()}, cause {r['cause'].tolist()}")
        for i, sg in enumerate(segs):
            track = np.array([-P[:, :3].T @ P[:, 3] for P in sg["poses"]])
            print(f"  segment {i}: frames {sg['first_pair']}..{sg['first_pair'] + sg['n_pairs']}, last camera centre in its own gauge {np.round(track[-1], 2)}")
    rounds = sum(max(c["lengths"]) for c in plan_calls(lengths, S, chunk, slots))
    waves = sum(max(lengths[i:i + S]) for i in range(0, len(lengths), S))
    print(f"step rounds: {rounds} with the pool, {waves} in waves of {S} flights")


if __name__ == "__main__":
    main()

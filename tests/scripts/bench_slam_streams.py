#!/usr/bin/env python3
"""Measurement of several map streams carried from call to call (vo_slam_streams / FrontEnd.slam_streams): the job of
bench_slam_chain.py — 64 consecutive 1280x720 ORB pairs of the closed flight, 2000 features, the reference's defaults — cut into
S in {1, 2, 4, 8, 16} sequences of 64 / S pairs on disjoint slot ranges (a frame two sequences share sits in two slots) and walked
in calls of at most --chunk pairs per sequence.  All frames stay resident, one FrontEnd per S; what is timed is the map step (the
sum of the stream's calls: carry, set-up, steps, downloads), not vo_pairs_run, which runs untimed before every call.  Medians of
--repeats runs after a warm-up, the S values and their yardsticks interleaved in one process.
Yardsticks: at S = 1 slam_stream_restart on the same pairs with the same chunking; at S > 1 slam_chains(restart=True) on the same
sequences in one call.  The margin a yardstick gets is its own max - min spread plus 1 % of its median.  A second pass with the
library's event brackets on splits every S by stage.  Prints a text report; nothing here is a pass / fail number."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from visual_odometry_amd import synth  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd, join_stream, join_streams  # noqa: E402

STAGES = dict(misc="chain steps", slam_ba_prepare="k_slam_ba_prepare", slam_bundle_adjust="k_bundle_adjust", slam_filter="k_slam_filter",
              slam_camera_limit="k_slam_limit")
KEYS = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials", "poses_pnp", "poses", "segment", "cause")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--distinct-frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=8)
    args = ap.parse_args()
    P = args.pairs
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:P + 1], seq["K"]
    fes = {}
    for S in args.sequences:                                   # sequence s: frames s q .. s q + q in slots s (q + 1) .. s (q + 1) + q
        assert P % S == 0
        q = P // S
        fe = FrontEnd(args.height, args.width, max_frames=P + S, max_pairs=P, nfeatures=args.nfeatures)
        fe.upload(np.concatenate([frames[s * q:s * q + q + 1] for s in range(S)])); fe.detect(0, P + S)
        fes[S] = fe
        print(f"S = {S}: {P + S} frames resident", file=sys.stderr, flush=True)

    def pairs_of(S, a, b):                                     # pairs a .. b - 1 of every sequence
        q = P // S
        return np.array([[s * (q + 1) + k, s * (q + 1) + k + 1] for s in range(S) for k in range(a, b)], np.int32)

    def streams(S):
        fe, q, dt, outs = fes[S], P // S, 0.0, []
        for a in range(0, q, args.chunk):
            b = min(a + args.chunk, q)
            fe.run_pairs(pairs_of(S, a, b), K, want_points=True)
            t0 = time.perf_counter()
            outs.append(fe.slam_streams([b - a] * S, K, resume=a > 0, total_pairs=[q] * S))
            dt += time.perf_counter() - t0
        return dt, join_streams(outs)

    def single():                                              # S = 1's yardstick
        fe, dt, outs = fes[1], 0.0, []
        for a in range(0, P, args.chunk):
            b = min(a + args.chunk, P)
            fe.run_pairs(pairs_of(1, a, b), K, want_points=True)
            t0 = time.perf_counter()
            outs.append(fe.slam_stream_restart(b - a, K, resume=a > 0, total_pairs=P))
            dt += time.perf_counter() - t0
        return dt, [join_stream(outs)]

    def chains(S):                                             # S > 1's yardstick
        fe, q = fes[S], P // S
        fe.run_pairs(pairs_of(S, 0, q), K, want_points=True)
        t0 = time.perf_counter()
        out = fe.slam_chains([q] * S, K, restart=True)
        return time.perf_counter() - t0, out

    jobs = []
    for S in args.sequences:
        jobs.append((("streams", S), lambda S=S: streams(S)))
        jobs.append((("yardstick", S), single if S == 1 else (lambda S=S: chains(S))))
    for _ in range(2):                                         # warm-up: allocations, code objects
        for _, fn in jobs:
            fn()
    times, outs = {k: [] for k, _ in jobs}, {}
    for _ in range(args.repeats):
        for k, fn in jobs:
            dt, outs[k] = fn()
            times[k].append(dt)
    prof = {}
    for S in args.sequences:
        fes[S].profile(True)
        for _ in range(3):
            streams(S)
        prof[S] = fes[S].profile_read()
        fes[S].profile(False)
    print(f"job: {P} consecutive {args.width}x{args.height} ORB pairs, {args.nfeatures} features, the reference's defaults, one MI355X, one process, all frames "
          f"resident, cut into S sequences of {P} / S pairs on disjoint slots, calls of at most {args.chunk} pairs per sequence; medians of {args.repeats} runs, "
          f"the S values and their yardsticks interleaved; timed: the map step's calls only")
    print("yardstick: S = 1 slam_stream_restart with the same chunking; S > 1 slam_chains(restart=True) on the same sequences in one call")
    print("  S  calls   slam_streams ms (min .. max)     yardstick ms (min .. max)        margin ms   streams - yardstick          ms/frame   frames/s   localised   same bytes as the yardstick")
    for S in args.sequences:
        t, y = times[("streams", S)], times[("yardstick", S)]
        mt, my = statistics.median(t), statistics.median(y)
        margin = max(y) - min(y) + 0.01 * my
        got, want = outs[("streams", S)], outs[("yardstick", S)]
        same = all(np.array_equal(got[s][k], want[s][k]) for s in range(S) for k in KEYS)
        ok = sum(int((o["status"] == 0).sum()) for o in got)
        calls = -(-(P // S) // args.chunk)
        print(f" {S:2d}  {calls:5d}   {1e3 * mt:8.2f} ({1e3 * min(t):8.2f} .. {1e3 * max(t):8.2f})   {1e3 * my:8.2f} ({1e3 * min(y):8.2f} .. {1e3 * max(y):8.2f})   {1e3 * margin:8.2f}   "
              f"{1e3 * (mt - my):+9.2f} {'within the margin' if mt - my <= margin else 'BEYOND the margin':18s}  {1e3 * mt / P:8.3f}   {P / mt:8.1f}   {ok}/{P}       {same}")
    print("split of slam_streams (event brackets on, 3 runs; ms per run and event brackets per run):")
    print("  S   " + "".join(f"{v:>28s}" for v in STAGES.values()) + "        sum")
    for S in args.sequences:
        ms = [prof[S].get(k, (0.0, 0))[0] / 3 for k in STAGES]
        n = [prof[S].get(k, (0.0, 0))[1] // 3 for k in STAGES]
        print(f" {S:2d}   " + "".join(f"{a:20.3f} {b:7d}" for a, b in zip(ms, n)) + f"   {sum(ms):8.3f}")


if __name__ == "__main__":
    main()

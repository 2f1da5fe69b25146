#!/usr/bin/env python3
"""Measurement of the seats of a multi-stream (vo_slam_streams_open / vo_slam_streams_replace): a dozen flights of unequal length, 4
to 24 pairs, cut from the resident 1280x720 run of bench_slam_chain.py — the closed flight, 2000 features, the reference's defaults —
onto slots of their own, and walked on S = 4 and S = 8 seats in calls of at most --chunk pairs per seat, in two ways:
  pool   flight_pool.plan_calls: a seat whose flight has ended is replaced and takes the next waiting flight in the same call;
  waves  slam_streams(resume=False) per wave of S flights in list order, the seats of the shorter flights idle until the wave's
         longest flight has ended — the only schedule there is without seats, and the yardstick: its kernels are the ones the
         library had before.
All frames stay resident; the two schedules alternate in one process, medians of --repeats runs after a warm-up.  Timed: the map
step (open, replace and the slam_streams calls) and, beside it, the wall time of the whole job with the untimed part — vo_pairs_run
before every call — included.  The margin the yardstick gets is its own max - min spread plus 1 % of its median.  A second pass
with the library's event brackets on splits both schedules by stage.  Writes a text report; nothing here is a pass / fail number."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from visual_odometry_amd import synth  # noqa: E402
from visual_odometry_amd.flight_pool import plan_calls  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd, join_stream, join_streams, split_flights  # noqa: E402

STAGES = dict(misc="carry + chain steps", slam_ba_prepare="k_slam_ba_prepare", slam_bundle_adjust="k_bundle_adjust", slam_filter="k_slam_filter",
              slam_camera_limit="k_slam_limit")
KEYS = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials", "poses_pnp", "poses", "segment", "cause")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seats", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--lengths", type=int, nargs="+", default=[4, 9, 24, 5, 4, 13, 7, 4, 18, 6, 11, 8])
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--distinct-frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slam_seats_bench.txt"))
    args = ap.parse_args()
    lengths, chunk = args.lengths, args.chunk
    first = np.concatenate([[0], np.cumsum([n + 1 for n in lengths])])      # flight f: frames and slots first[f] .. first[f] + lengths[f]
    n_frames = int(first[-1])
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    K = seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n_frames, max_pairs=max(args.seats) * chunk, nfeatures=args.nfeatures)
    fe.upload(seq["frames"][:n_frames]); fe.detect(0, n_frames)
    print(f"{len(lengths)} flights, {sum(lengths)} pairs, {n_frames} frames resident", file=sys.stderr, flush=True)

    def pairs_of(f, a, n):
        return [[int(first[f]) + k, int(first[f]) + k + 1] for k in range(a, a + n)]

    def pool(S):
        plan = plan_calls(lengths, S, chunk, 1 << 20)                      # (only the schedule: every frame has a slot of its own)
        done, outs, took, t_map = [0] * len(lengths), [], [[] for _ in range(S)], 0.0
        t_all = time.perf_counter()
        fe.slam_streams_open(S, max(lengths), K)
        t_map += time.perf_counter() - t_all
        for c, call in enumerate(plan):
            t0 = time.perf_counter()
            for s in call["replace"]:
                fe.slam_streams_replace(s, max(lengths) if call["flights"][s] is None else lengths[call["flights"][s]])
            t_map += time.perf_counter() - t0
            pairs = []
            for s, n in enumerate(call["lengths"]):
                f = call["flights"][s]
                if n:
                    pairs += pairs_of(f, done[f], n); done[f] += n
            fe.run_pairs(pairs, K, want_points=True)
            t0 = time.perf_counter()
            outs.append(fe.slam_streams(call["lengths"], K, resume=True))
            t_map += time.perf_counter() - t0
            for s in call["took"]:
                took[s].append(c)
        wall = time.perf_counter() - t_all
        order = [[call["flights"][s] for call in plan if s in call["took"]] for s in range(S)]
        joined = [None] * len(lengths)
        for s, fl in enumerate(split_flights(outs, took)):
            for f, slices in zip(order[s], fl):
                joined[f] = join_stream(slices)
        return t_map, wall, joined, sum(max(c["lengths"]) for c in plan), len(plan)

    def waves(S):
        t_map, joined, rounds, calls = 0.0, [], 0, 0
        t_all = time.perf_counter()
        for w in range(0, len(lengths), S):
            fl = list(range(w, min(w + S, len(lengths))))
            outs = []
            for a in range(0, max(lengths[f] for f in fl), chunk):
                ns = [max(0, min(chunk, lengths[f] - a)) for f in fl]
                fe.run_pairs(sum((pairs_of(f, a, n) for f, n in zip(fl, ns)), []), K, want_points=True)
                t0 = time.perf_counter()
                outs.append(fe.slam_streams(ns, K, resume=a > 0, total_pairs=[lengths[f] for f in fl]))
                t_map += time.perf_counter() - t0
                rounds += max(ns); calls += 1
            joined += join_streams(outs)
        return t_map, time.perf_counter() - t_all, joined, rounds, calls

    jobs = [((kind, S), (lambda S=S, fn=fn: fn(S))) for S in args.seats for kind, fn in (("pool", pool), ("waves", waves))]
    for _, fn in jobs:                                                      # warm-up: allocations, code objects
        fn()
    t_map, t_wall, last = {k: [] for k, _ in jobs}, {k: [] for k, _ in jobs}, {}
    for _ in range(args.repeats):
        for k, fn in jobs:
            a, b, *rest = fn()
            t_map[k].append(a); t_wall[k].append(b); last[k] = rest
    prof = {}
    for k, fn in jobs:
        fe.profile(True)
        for _ in range(3):
            fn()
        prof[k] = fe.profile_read()
        fe.profile(False)
    P = sum(lengths)
    rep = [f"job: {len(lengths)} flights of {lengths} pairs ({P} pairs) cut from consecutive {args.width}x{args.height} ORB frames of the closed flight onto slots of "
           f"their own, {args.nfeatures} features, the reference's defaults, one MI355X, one process, all {n_frames} frames resident; calls of at most {chunk} pairs "
           f"per seat; medians of {args.repeats} runs after a warm-up, the two schedules alternating",
           "pool: plan_calls on S seats of a stream opened vacant (slam_streams_open / slam_streams_replace); waves: slam_streams(resume=False) per wave of S flights "
           "in list order — the yardstick, whose margin is its own max - min spread plus 1 % of its median",
           "timed as `map`: open, replace and the slam_streams calls; `wall`: the whole job, vo_pairs_run before every call included",
           "  S  schedule  calls  step rounds  seats at work / round   map ms (min .. max)               wall ms     map ms / step round    frames/s (map)   localised   same bytes as the waves"]
    for S in args.seats:
        for kind in ("waves", "pool"):
            t, w = t_map[(kind, S)], t_wall[(kind, S)]
            joined, rounds, calls = last[(kind, S)]
            same = all(np.array_equal(joined[f][k], last[("waves", S)][0][f][k]) for f in range(len(lengths)) for k in KEYS)
            ok = sum(int((o["status"] == 0).sum()) for o in joined)
            mt = statistics.median(t)
            rep.append(f" {S:2d}  {kind:8s}  {calls:5d}  {rounds:11d}  {P / rounds:21.2f}   {1e3 * mt:8.2f} ({1e3 * min(t):8.2f} .. {1e3 * max(t):8.2f})   {1e3 * statistics.median(w):8.2f}   "
                       f"{1e3 * mt / rounds:12.3f}           {P / mt:8.1f}         {ok}/{P}     {same}")
        (yw, rw), (yp, rp) = ((t_map[(k, S)], last[(k, S)][1]) for k in ("waves", "pool"))
        per_w, per_p = statistics.median(yw) / rw, statistics.median(yp) / rp
        margin = (max(yw) - min(yw) + 0.01 * statistics.median(yw)) / rw
        rep.append(f"     S = {S}: the pool's time per step round - the waves' = {1e3 * (per_p - per_w):+.3f} ms, margin {1e3 * margin:.3f} ms per step round: "
                   f"{'within the margin' if per_p - per_w <= margin else 'BEYOND the margin'}; step rounds {rp} against {rw} ({100.0 * (rw - rp) / rw:.1f} % saved), "
                   f"map time {1e3 * statistics.median(yp):.2f} against {1e3 * statistics.median(yw):.2f} ms ({100.0 * (1 - statistics.median(yp) / statistics.median(yw)):.1f} % saved)")
    rep.append("split by stage (event brackets on, 3 runs; ms per run and event brackets per run; second line: ms per step round):")
    rep.append("  S  schedule  " + "".join(f"{v:>28s}" for v in STAGES.values()) + "        sum")
    for S in args.seats:
        for kind in ("waves", "pool"):
            ms = [prof[(kind, S)].get(k, (0.0, 0))[0] / 3 for k in STAGES]
            n = [prof[(kind, S)].get(k, (0.0, 0))[1] // 3 for k in STAGES]
            r = last[(kind, S)][1]
            rep.append(f" {S:2d}  {kind:8s}  " + "".join(f"{a:20.3f} {b:7d}" for a, b in zip(ms, n)) + f"   {sum(ms):8.3f}")
            rep.append("     / round   " + "".join(f"{a / r:20.3f}        " for a in ms) + f"   {sum(ms) / r:8.3f}")
    rep.append("not measured here: the reset's own time (it is inside the carry launch, bracketed with the chain steps), and the cost with real uploads between the calls")
    text = "\n".join(rep) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurement of what a stream's descriptor store costs (vo_set_stream_rows; k_stream_rows_append, k_stream_rows_select): the job
of bench_slam_stream.py — 64 consecutive 1280x720 ORB pairs of the closed flight, 2000 features, the reference's defaults, all 65
frames resident — walked as slam_stream in chunks of 16, the store alternating off and on in one process, medians of --repeats
each.  What is timed is the sum of the stream's slam_stream calls (carry, steps, the append with the store on, downloads), not
uploads, detection or vo_pairs_run.  The yardstick is the store-off median of the same job; its margin is the store-off runs' own
max - min spread plus 1 %.  Expected: one append launch per call, moving at most kp_cap * D bytes per new frame.  Also timed, on
the stream the last store-on run leaves: map_from_stream() of the whole map and of a 4-frame window (select, counts back,
k_map_gather, wait).  A pass with the library's event brackets on splits both forms by stage (the append falls under misc).
NOT measured here: flights beyond --pairs, SIFT rows (D = 128) at a real kp_cap, the append under real slot reuse.
Prints a text report; nothing here is a pass / fail number."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from visual_odometry_amd import synth  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd  # noqa: E402

STAGES = dict(misc="chain steps (gather, solvePnPRansac, pose, triangulate, add, carry[, append])", slam_ba_prepare="k_slam_ba_prepare",
              slam_bundle_adjust="k_bundle_adjust", slam_filter="k_slam_filter", slam_camera_limit="k_slam_limit")
PER_PAIR = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--distinct-frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--window", type=int, default=4)
    args = ap.parse_args()
    n = args.pairs + 1
    p = n - 1
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:n], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n, max_pairs=p, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, n)

    def stream(store):
        fe.stream_rows(-1 if store else 0)
        dt, outs = 0.0, []
        for a in range(0, p, args.chunk):
            b = min(a + args.chunk, p)
            fe.run_pairs(np.stack([np.arange(a, b), np.arange(a, b) + 1], 1).astype(np.int32), K, want_points=True)
            t0 = time.perf_counter()
            outs.append(fe.slam_stream(b - a, K, resume=a > 0, total_pairs=p))
            dt += time.perf_counter() - t0
        return dt, {k: np.concatenate([o[k] for o in outs]) for k in PER_PAIR}

    forms = [("store off", lambda: stream(False)), ("store on (capacity -1)", lambda: stream(True))]
    for _ in range(2):                                         # warm-up: allocations, code objects
        for _, fn in forms:
            fn()
    times, outs = {name: [] for name, _ in forms}, {}
    for _ in range(args.repeats):
        for name, fn in forms:
            dt, outs[name] = fn()
            times[name].append(dt)
    # the stream the last store-on run left is live: stage its map
    info, m = fe.stream_rows_info(), fe.slam_map(0)
    last = int(m["pt_feature"][:, 0].max()) if len(m["pt_feature"]) else 0
    win = (max(last - args.window + 1, 0), last + 1)
    stage = {"whole map": [], f"frames [{win[0]}, {win[1]})": []}
    sizes = {}
    for _ in range(2 + args.repeats):
        for name, a in zip(stage, ((0, None), win)):
            t0 = time.perf_counter()
            r = fe.map_from_stream(*a)
            stage[name].append(time.perf_counter() - t0)
            sizes[name] = r
    prof = {}
    for name, fn in forms:
        fe.profile(True)
        for _ in range(3):
            fn()
        prof[name] = fe.profile_read()
        fe.profile(False)
    fe.stream_rows(0)
    ms = lambda t: 1e3 * t / p                                 # noqa: E731
    base = forms[0][0]
    m0 = statistics.median(times[base])
    spread = max(times[base]) - min(times[base])
    margin = spread + 0.01 * m0
    calls = (p + args.chunk - 1) // args.chunk
    print(f"job: {p} consecutive {args.width}x{args.height} ORB pairs, {args.nfeatures} features, slam_stream in chunks of {args.chunk} ({calls} calls), one MI355X, "
          f"one context, all frames resident; medians of {args.repeats} alternating runs; timed: the slam_stream calls only")
    for name, _ in forms:
        t = times[name]
        same = all(np.array_equal(outs[base][k], outs[name][k]) for k in PER_PAIR)
        print(f"{name:24s} {ms(statistics.median(t)):.3f} ms/frame   min {ms(min(t)):.3f} max {ms(max(t)):.3f}   localised {int((outs[name]['status'] == 0).sum())}/{p}   "
              f"per-pair outputs {'identical bytes' if same else 'DIFFER'}")
    print(f"margin = spread of the store-off runs {ms(spread):.3f} + 1 % of their median = {ms(margin):.3f} ms/frame")
    d = statistics.median(times[forms[1][0]]) - m0
    print(f"store on - store off: {ms(d):+.3f} ms/frame ({1e6 * d / calls:+.1f} us per call): {'within the margin' if d <= margin else 'BEYOND the margin'}")
    D = 32
    print(f"store: capacity {info['capacity']} rows ({info['capacity'] * D / 2 ** 20:.1f} MiB of rows + {4 * n * fe.kp_cap / 2 ** 20:.1f} MiB of row_of), "
          f"stored {info['stored']}, dropped {info['dropped']}; live map {len(m['points'])} points")
    for name, t in stage.items():
        t = t[2:]
        print(f"map_from_stream, {name:18s} {1e6 * statistics.median(t):8.1f} us   min {1e6 * min(t):.1f} max {1e6 * max(t):.1f}   staged {sizes[name]['n']} without a row {sizes[name]['without_row']}")
    print("split (event brackets on, 3 runs each; ms per frame, one column per form in the order above):")
    for key, label in STAGES.items():
        print(f"  {label:82s} " + " ".join(f"{prof[name].get(key, (0.0, 0))[0] / 3 / p:8.4f}" for name, _ in forms))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurement of what carrying the map between calls costs (vo_slam_stream beside vo_slam_chain): the chunk bench_slam_chain.py
uses — 64 consecutive 1280x720 ORB pairs of the closed flight, 2000 features, the reference's defaults — walked as one slam_chain
call and as a stream in chunks of 16 and of 8 pairs, the three forms alternating in one process, medians of --repeats each.  All
65 frames stay resident: what is timed is the map step (the slam_chain call; the sum of a stream's slam_stream calls — carry, set-up,
steps, downloads), not uploads, detection or vo_pairs_run, which run untimed before every call.  The yardstick is the slam_chain
median of the same job; the margin it gets is that job's own max - min spread of the slam_chain runs plus 1 %.  A second pass with
the library's event brackets on splits every form's time by stage (k_slam_carry falls under the chain steps).
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

STAGES = dict(misc="chain steps (gather, solvePnPRansac, pose, triangulate, add[, carry])", slam_ba_prepare="k_slam_ba_prepare",
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
    ap.add_argument("--chunks", type=int, nargs="+", default=[16, 8])
    args = ap.parse_args()
    n = args.pairs + 1
    p = n - 1
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:n], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n, max_pairs=p, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, n)

    def chain():
        fe.run_pairs(np.stack([np.arange(p), np.arange(p) + 1], 1).astype(np.int32), K, want_points=True)
        t0 = time.perf_counter()
        out = fe.slam_chain(p, K)
        return time.perf_counter() - t0, out

    def stream(chunk):
        dt, outs = 0.0, []
        for a in range(0, p, chunk):
            b = min(a + chunk, p)
            fe.run_pairs(np.stack([np.arange(a, b), np.arange(a, b) + 1], 1).astype(np.int32), K, want_points=True)
            t0 = time.perf_counter()
            outs.append(fe.slam_stream(b - a, K, resume=a > 0, total_pairs=p))
            dt += time.perf_counter() - t0
        return dt, {k: np.concatenate([o[k] for o in outs]) for k in PER_PAIR}

    forms = [("slam_chain, one call", chain)] + [(f"slam_stream, chunks of {c}", (lambda c=c: stream(c))) for c in args.chunks]
    for _ in range(2):                                         # warm-up: allocations, code objects
        for _, fn in forms:
            fn()
    times, outs = {name: [] for name, _ in forms}, {}
    for _ in range(args.repeats):
        for name, fn in forms:
            dt, outs[name] = fn()
            times[name].append(dt)
    prof = {}
    for name, fn in forms:
        fe.profile(True)
        for _ in range(3):
            fn()
        prof[name] = fe.profile_read()
        fe.profile(False)
    ms = lambda t: 1e3 * t / p                                 # noqa: E731
    base = forms[0][0]
    m0 = statistics.median(times[base])
    spread = max(times[base]) - min(times[base])
    margin = spread + 0.01 * m0
    print(f"chunk: {p} consecutive {args.width}x{args.height} ORB pairs, {args.nfeatures} features, one MI355X, one context, all frames resident; "
          f"medians of {args.repeats} alternating runs; timed: the slam_chain / slam_stream calls only")
    for name, _ in forms:
        t = times[name]
        same = all(np.array_equal(outs[base][k], outs[name][k]) for k in PER_PAIR)
        print(f"{name:28s} {ms(statistics.median(t)):.3f} ms/frame   min {ms(min(t)):.3f} max {ms(max(t)):.3f}   localised {int((outs[name]['status'] == 0).sum())}/{p}   "
              f"per-pair outputs {'identical bytes' if same else 'DIFFER'}")
    print(f"margin = spread of the slam_chain runs {ms(spread):.3f} + 1 % of their median = {ms(margin):.3f} ms/frame")
    for name, _ in forms[1:]:
        d = statistics.median(times[name]) - m0
        print(f"{name} - slam_chain: {ms(d):+.3f} ms/frame: {'within the margin' if d <= margin else 'BEYOND the margin'}")
    print("split (event brackets on, 3 runs each; ms per frame, one column per form in the order above):")
    for key, label in STAGES.items():
        print(f"  {label:76s} " + " ".join(f"{prof[name].get(key, (0.0, 0))[0] / 3 / p:8.4f}" for name, _ in forms))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurement of what the restart form of the stream costs on a flight that never fails (vo_slam_stream_restart beside
vo_slam_stream): the chunk bench_slam_chain.py uses — 64 consecutive 1280x720 ORB pairs of the closed flight, 2000 features, the
reference's defaults — walked in chunks of 16 pairs through slam_stream and through slam_stream_restart, the two forms alternating
in one process, medians of --repeats each after a warm-up.  All 65 frames stay resident: what is timed is the map step (the sum
of a stream's calls — carry, set-up, steps, downloads), not uploads, detection or vo_pairs_run, which run untimed before every
call.  The yardstick is the slam_stream median of the same job; the margin it gets is that job's own max - min spread of the
slam_stream runs plus 1 %.  Expected: one more launch per step (k_slam_restart_stream).  A second pass with the library's event
brackets on splits both forms' time by stage (the restart kernel and k_slam_carry fall under the chain steps).
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
from visual_odometry_amd.frontend import FrontEnd, join_stream  # noqa: E402

STAGES = dict(misc="chain steps (carry, gather, solvePnPRansac, pose[, restart], triangulate, add)", slam_ba_prepare="k_slam_ba_prepare",
              slam_bundle_adjust="k_bundle_adjust", slam_filter="k_slam_filter", slam_camera_limit="k_slam_limit")
SHARED = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials", "poses_pnp", "poses")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--distinct-frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=16)
    args = ap.parse_args()
    n = args.pairs + 1
    p = n - 1
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:n], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n, max_pairs=p, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, n)

    def stream(restart):
        call = fe.slam_stream_restart if restart else fe.slam_stream
        dt, outs = 0.0, []
        for a in range(0, p, args.chunk):
            b = min(a + args.chunk, p)
            fe.run_pairs(np.stack([np.arange(a, b), np.arange(a, b) + 1], 1).astype(np.int32), K, want_points=True)
            t0 = time.perf_counter()
            outs.append(call(b - a, K, resume=a > 0, total_pairs=p))
            dt += time.perf_counter() - t0
        return dt, join_stream(outs)

    forms = [("slam_stream", lambda: stream(False)), ("slam_stream_restart", lambda: stream(True))]
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
    base, on = forms[0][0], forms[1][0]
    m0 = statistics.median(times[base])
    spread = max(times[base]) - min(times[base])
    margin = spread + 0.01 * m0
    print(f"chunk: {p} consecutive {args.width}x{args.height} ORB pairs, {args.nfeatures} features, one MI355X, one context, all frames resident, "
          f"streams in chunks of {args.chunk} pairs; medians of {args.repeats} alternating runs; timed: the stream's calls only")
    for name, _ in forms:
        t = times[name]
        same = all(np.array_equal(outs[base][k], outs[name][k]) for k in SHARED)
        print(f"{name:22s} {ms(statistics.median(t)):.3f} ms/frame   min {ms(min(t)):.3f} max {ms(max(t)):.3f}   localised {int((outs[name]['status'] == 0).sum())}/{p}   "
              f"shared outputs {'identical bytes' if same else 'DIFFER'}")
    print(f"segments of the restart stream: {sorted(set(outs[on]['segment'].tolist()))}, causes {sorted(set(outs[on]['cause'].tolist()))}")
    print(f"margin = spread of the slam_stream runs {ms(spread):.3f} + 1 % of their median = {ms(margin):.3f} ms/frame")
    d = statistics.median(times[on]) - m0
    print(f"{on} - {base}: {ms(d):+.3f} ms/frame: {'within the margin' if d <= margin else 'BEYOND the margin'}")
    print("split (event brackets on, 3 runs each; ms per frame and event brackets per run, one column pair per form in the order above):")
    for key, label in STAGES.items():
        print(f"  {label:84s} " + " ".join(f"{prof[name].get(key, (0.0, 0))[0] / 3 / p:8.4f} {prof[name].get(key, (0.0, 0))[1] // 3:5d}" for name, _ in forms))
    print("what a restart itself costs on a flight that does fail: unmeasured")


if __name__ == "__main__":
    main()

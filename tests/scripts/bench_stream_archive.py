#!/usr/bin/env python3
"""Measurement of what a stream's archive of evicted points costs (vo_set_stream_archive; k_slam_limit_stream_archive,
k_stream_archive_count / _emit, k_map_gather_from): the job of bench_stream_rows.py — 64 consecutive 1280x720 ORB pairs of the
closed flight, 2000 features, all 65 frames resident — walked as slam_stream in chunks of 16 with --max-cameras 8, so that the limit
of every pair from pair 7 on evicts a camera (57 of 64 steps); store only and store + archive alternate in one process, medians of
--repeats each.  What is timed is the sum of the stream's slam_stream calls, not uploads, detection or vo_pairs_run.  The yardstick
is the store-only median of the same job (its launches are the parent's); its margin is the store-only runs' own max - min spread
plus 1 %.  Also timed, on the stream the last archive run leaves: map_from_stream_archive() of a 4-frame window of the flight's
start and of the whole flight (select over the live map and over the archive, counts back, two gathers, wait).  A pass with the
library's event brackets on splits both forms by stage: slam_camera_limit holds k_slam_limit_stream / k_slam_limit_stream_archive.
No threshold is fixed in advance for any of these.  NOT measured here: SIFT rows (D = 128), archives beyond this job's.
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

STAGES = dict(misc="chain steps (gather, solvePnPRansac, pose, triangulate, add, carry, append)", slam_ba_prepare="k_slam_ba_prepare",
              slam_bundle_adjust="k_bundle_adjust", slam_filter="k_slam_filter", slam_camera_limit="k_slam_limit_stream[_archive]")
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
    ap.add_argument("--max-cameras", type=int, default=8)
    args = ap.parse_args()
    n = args.pairs + 1
    p = n - 1
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:n], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n, max_pairs=p, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, n)
    fe.stream_rows(-1)

    def stream(archive):
        fe.stream_archive(-1 if archive else 0)
        dt, outs = [], []
        for a in range(0, p, args.chunk):
            b = min(a + args.chunk, p)
            fe.run_pairs(np.stack([np.arange(a, b), np.arange(a, b) + 1], 1).astype(np.int32), K, want_points=True)
            t0 = time.perf_counter()
            outs.append(fe.slam_stream(b - a, K, resume=a > 0, total_pairs=p, max_cameras=args.max_cameras))
            dt.append(time.perf_counter() - t0)
        return dt, {k: np.concatenate([o[k] for o in outs]) for k in PER_PAIR}

    forms = [("store only", lambda: stream(False)), ("store + archive (-1)", lambda: stream(True))]
    for _ in range(2):                                         # warm-up: allocations, code objects
        for _, fn in forms:
            fn()
    times, first, outs = {name: [] for name, _ in forms}, {name: [] for name, _ in forms}, {}
    for _ in range(args.repeats):
        for name, fn in forms:
            dt, outs[name] = fn()
            times[name].append(sum(dt)); first[name].append(dt[0])        # (the call that starts the stream allocates and clears)
    # the stream the last archive run left is live: stage from it
    info, arc, m = fe.stream_rows_info(), fe.stream_archive_info(), fe.slam_map(0)
    evicting = int((np.concatenate([[2], outs[forms[1][0]]["n_cam"][:-1] + 1]) > args.max_cameras).sum())
    stage = {f"frames [0, {args.window})": (0, args.window), "the whole flight": (0, None)}
    took, sizes = {k: [] for k in stage}, {}
    for _ in range(2 + args.repeats):
        for name, a in stage.items():
            t0 = time.perf_counter()
            r = fe.map_from_stream_archive(*a)
            took[name].append(time.perf_counter() - t0)
            sizes[name] = r
    prof = {}
    for name, fn in forms:
        fe.profile(True)
        for _ in range(3):
            fn()
        prof[name] = fe.profile_read()
        fe.profile(False)
    fe.stream_rows(0); fe.stream_archive(0)
    ms = lambda t: 1e3 * t / p                                 # noqa: E731
    base = forms[0][0]
    m0 = statistics.median(times[base])
    spread = max(times[base]) - min(times[base])
    margin = spread + 0.01 * m0
    calls = (p + args.chunk - 1) // args.chunk
    print(f"job: {p} consecutive {args.width}x{args.height} ORB pairs, {args.nfeatures} features, slam_stream in chunks of {args.chunk} ({calls} calls), "
          f"max_cameras {args.max_cameras} ({evicting} of {p} steps evict a camera), one MI355X, one context, all frames resident; medians of {args.repeats} "
          f"alternating runs; timed: the slam_stream calls only")
    for name, _ in forms:
        t = times[name]
        same = all(np.array_equal(outs[base][k], outs[name][k]) for k in PER_PAIR)
        print(f"{name:24s} {ms(statistics.median(t)):.3f} ms/frame   min {ms(min(t)):.3f} max {ms(max(t)):.3f}   localised {int((outs[name]['status'] == 0).sum())}/{p}   "
              f"per-pair outputs {'identical bytes' if same else 'DIFFER'}")
    print(f"margin = spread of the store-only runs {ms(spread):.3f} + 1 % of their median = {ms(margin):.3f} ms/frame")
    d = statistics.median(times[forms[1][0]]) - m0
    print(f"store + archive - store only: {ms(d):+.3f} ms/frame ({1e6 * d / max(evicting, 1):+.1f} us per evicting step): "
          f"{'within the margin' if abs(d) <= margin else 'BEYOND the margin'}")
    f0, f1 = (statistics.median(first[name]) for name, _ in forms)
    print(f"of which the call that starts the stream (allocations and their clearing; 1 of {calls} calls): {1e3 * f0:.3f} -> {1e3 * f1:.3f} ms, {1e3 * (f1 - f0):+.3f} ms "
          f"= {ms(f1 - f0):+.3f} ms/frame of this job; the {calls - 1} resumed calls together: {ms(d - (f1 - f0)):+.3f} ms/frame")
    D = 32
    print(f"archive: capacity {arc['capacity']} entries ({arc['capacity'] * (D + 40) / 2 ** 20:.1f} MiB), stored {arc['stored']} "
          f"({arc['stored'] / max(evicting, 1):.0f} per evicting step), dropped {arc['dropped']}; store: stored {info['stored']} of {info['capacity']}; "
          f"live map {len(m['points'])} points of {len(m['cam_frame'])} cameras")
    for name, t in took.items():
        t, r = t[2:], sizes[name]
        print(f"map_from_stream_archive, {name:18s} {1e6 * statistics.median(t):8.1f} us   min {1e6 * min(t):.1f} max {1e6 * max(t):.1f}   staged {r['n']} "
              f"({r['n'] - r['n_archived']} live + {r['n_archived']} archived) without a row {r['without_row']}")
    print("split (event brackets on, 3 runs each; ms per frame, one column per form in the order above):")
    for key, label in STAGES.items():
        print(f"  {label:82s} " + " ".join(f"{prof[name].get(key, (0.0, 0))[0] / 3 / p:8.4f}" for name, _ in forms))


if __name__ == "__main__":
    main()

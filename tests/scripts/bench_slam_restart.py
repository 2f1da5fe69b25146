#!/usr/bin/env python3
"""Measurement of what restart=True costs on a chain that never fails (vo_slam_chains_restart beside vo_slam_chains): the chunk
bench_slam_chain.py uses — 64 consecutive 1280x720 ORB pairs of the closed flight, 2000 features, resident in HBM, the reference's
defaults — as one sequence, the two entries alternating in one process, medians of --repeats calls each.  The yardstick is the
restart=False median of the same job; the margin it gets is that job's own max - min spread of the off runs plus 1 %: the added
kernels are microsecond launches beside milliseconds per frame, so anything beyond the spread is a finding, and the report says
which bracket grew.  A second pass with the library's event brackets on splits both forms' time by stage.
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

STAGES = dict(misc="chain steps (gather, solvePnPRansac, pose, [restart,] triangulate, add)", slam_ba_prepare="k_slam_ba_prepare",
              slam_bundle_adjust="k_bundle_adjust", slam_filter="k_slam_filter", slam_camera_limit="k_slam_limit")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--distinct-frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    n = args.pairs + 1
    p = n - 1
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:n], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n, max_pairs=p, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, n)
    fe.run_pairs(np.stack([np.arange(p), np.arange(p) + 1], 1).astype(np.int32), K, want_points=True)
    off = lambda: fe.slam_chains([p], K)[0]                    # noqa: E731
    on = lambda: fe.slam_chains([p], K, restart=True)[0]       # noqa: E731
    off(); on(); off(); on()                                   # warm-up: allocations, code objects
    t_off, t_on = [], []
    for _ in range(args.repeats):
        dt, a = timed(off); t_off.append(dt)
        dt, b = timed(on); t_on.append(dt)
    same = all(np.array_equal(a[k], b[k]) for k in a)
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    spread = max(t_off) - min(t_off)
    margin = spread + 0.01 * m_off
    prof = {}
    for name, fn in (("off", off), ("on", on)):
        fe.profile(True)
        for _ in range(3):
            fn()
        prof[name] = fe.profile_read()
        fe.profile(False)
    ms = lambda t: 1e3 * t / p                                 # noqa: E731
    print(f"chunk: {p} consecutive {args.width}x{args.height} ORB pairs, {args.nfeatures} features, one sequence, one MI355X, one context; "
          f"medians of {args.repeats} alternating calls")
    print(f"restart=False (vo_slam_chains):         {ms(m_off):.3f} ms/frame   min {ms(min(t_off)):.3f} max {ms(max(t_off)):.3f}   localised {int((a['status'] == 0).sum())}/{p}")
    print(f"restart=True  (vo_slam_chains_restart): {ms(m_on):.3f} ms/frame   min {ms(min(t_on)):.3f} max {ms(max(t_on)):.3f}   localised {int((b['status'] == 0).sum())}/{p}   "
          f"segments {len(b['segments'])}   outputs {'identical bytes' if same else 'DIFFER'}")
    print(f"on - off: {ms(m_on - m_off):+.3f} ms/frame; margin = spread of the off runs {ms(spread):.3f} + 1 % of their median = {ms(margin):.3f} ms/frame: "
          f"{'within the margin' if m_on - m_off <= margin else 'BEYOND the margin'}")
    print("split (event brackets on, 3 calls each; ms per frame off / on / on - off):")
    for key, label in STAGES.items():
        x, y = prof["off"].get(key, (0.0, 0))[0] / 3 / p, prof["on"].get(key, (0.0, 0))[0] / 3 / p
        print(f"  {label:76s} {x:8.4f} {y:8.4f} {y - x:+8.4f}")


if __name__ == "__main__":
    main()

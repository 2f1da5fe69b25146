#!/usr/bin/env python3
"""Measurement of the localisation chain with the map's per-frame bundle adjustment (vo_slam_chain / FrontEnd.slam_chain) on the
chunk config.tracks_pnp_chain uses — 64 consecutive 1280x720 ORB pairs of the closed flight, 2000 features, resident in HBM —
with the reference's defaults (40 LM iterations, 2 free cameras, filter at 1.0, 18 cameras), beside localize_chain
(vo_tracks_pnp_batch) on the same run in the same process, the two alternating, medians of --repeats calls each.  A second pass
with the library's event brackets on splits slam_chain's time into chain steps / BA prepare / BA / filter / camera limit.
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
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:n], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n, max_pairs=n - 1, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, n)
    fe.run_pairs(np.stack([np.arange(n - 1), np.arange(n - 1) + 1], 1).astype(np.int32), K, want_points=True)
    chain = lambda: fe.localize_chain(n - 1, K)          # noqa: E731
    slam = lambda: fe.slam_chain(n - 1, K)               # noqa: E731
    chain(); slam(); chain(); slam()                     # warm-up: allocations, code objects
    tc, ts = [], []
    for _ in range(args.repeats):
        tc.append(timed(chain)[0])
        dt, out = timed(slam)
        ts.append(dt)
    lc = chain()
    mc, ms = statistics.median(tc), statistics.median(ts)
    ok = int((out["status"] == 0).sum())
    fe.profile(True)
    for _ in range(3):
        slam()
    prof = fe.profile_read()
    fe.profile(False)
    m = fe.slam_map(0)
    p = n - 1
    print(f"chunk: {p} consecutive {args.width}x{args.height} ORB pairs, {args.nfeatures} features, one MI355X, one context; medians of {args.repeats} alternating calls")
    print(f"localize_chain (vo_tracks_pnp_batch): {1e3 * mc / p:.3f} ms/frame  {p / mc:.1f} frames/s   min {1e3 * min(tc) / p:.3f} max {1e3 * max(tc) / p:.3f} ms/frame   localised {int((lc['status'] == 0).sum())}/{p}")
    print(f"slam_chain     (vo_slam_chain, defaults): {1e3 * ms / p:.3f} ms/frame  {p / ms:.1f} frames/s   min {1e3 * min(ts) / p:.3f} max {1e3 * max(ts) / p:.3f} ms/frame   localised {ok}/{p}")
    print(f"slam_chain map at the end: {len(m['cam_frame'])} cameras, {len(m['points'])} points, {len(m['obs_cam'])} observations; "
          f"per pair: LM iterations mean {out['ba_iterations'][:ok].mean():.1f}, trials mean {out['ba_trials'][:ok].mean():.1f}, "
          f"observations max {int(out['n_obs'].max())}, points max {int(out['n_pts'].max())}")
    print("slam_chain split (event brackets on, 3 calls; ms per frame, launches per call):")
    names = dict(misc="chain steps (gather, solvePnPRansac, pose, triangulate, add)", slam_ba_prepare="k_slam_ba_prepare", slam_bundle_adjust="k_bundle_adjust",
                 slam_filter="k_slam_filter", slam_camera_limit="k_slam_limit")
    total = 0.0
    for key, label in names.items():
        t, cnt = prof.get(key, (0.0, 0))
        total += t
        print(f"  {label:62s} {t / 3 / p:8.4f} ms/frame   {cnt // 3:4d} brackets")
    print(f"  {'sum of the brackets':62s} {total / 3 / p:8.4f} ms/frame")


if __name__ == "__main__":
    main()

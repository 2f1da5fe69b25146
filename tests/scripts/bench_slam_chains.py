#!/usr/bin/env python3
"""Measurement of the map step for several sequences in one call (vo_slam_chains / FrontEnd.slam_chains): S in {1, 2, 4, 8, 16}
sequences of 15 pairs each, cut from the 256-view closed flight at 1280x720 (2000 features) onto disjoint 16-frame slot ranges,
the reference's defaults (40 LM iterations, 2 free cameras, filter at 1.0, 18 cameras).  A host clock around the synchronising
call after warm-up, medians of --repeats calls with the S values interleaved in one process (each call follows a run_pairs of
its 15 S pairs, which is not timed).  Then, on one resident run of 15 pairs, slam_chains([15]) beside slam_chain(15), the two
alternating; then the library's event brackets per S, and the maps' sizes.  Prints a text report; nothing here is a pass / fail
number."""
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

OUT_KEYS = ("poses_pnp", "poses", "chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--pairs", type=int, default=15, help="pairs per sequence")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--repeats-single", type=int, default=9)
    args = ap.parse_args()
    P, smax = args.pairs, max(args.sequences)
    n = smax * (P + 1)
    seq = synth.sequence(n, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:n], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n, max_pairs=smax * P, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, n)

    def pairs_of(S):        # sequence s: frames / slots s (P + 1) .. s (P + 1) + P
        return np.array([[s * (P + 1) + k, s * (P + 1) + k + 1] for s in range(S) for k in range(P)], np.int32)

    def resident(S):
        fe.run_pairs(pairs_of(S), K, want_points=True)

    for S in args.sequences:                                # warm-up: allocations, code objects
        resident(S); fe.slam_chains([P] * S, K); fe.slam_chains([P] * S, K)
    t = {S: [] for S in args.sequences}
    last = {}
    for _ in range(args.repeats):
        for S in args.sequences:
            resident(S)
            dt, last[S] = timed(lambda: fe.slam_chains([P] * S, K))
            t[S].append(dt)
    print(f"{P} pairs per sequence, {args.width}x{args.height} ORB, {args.nfeatures} features, the reference's defaults, one MI355X, one context; "
          f"medians of {args.repeats} calls, the S values interleaved")
    print("  S   ms per call (min .. max)        ms per frame   frames/s (all sequences)   localised   identical to S = 1's sequence 0")
    for S in args.sequences:
        med = statistics.median(t[S])
        ok = sum(int((o["status"] == 0).sum()) for o in last[S])
        same = all(np.array_equal(last[S][0][k], last[min(args.sequences)][0][k]) for k in OUT_KEYS)
        print(f" {S:2d}   {1e3 * med:8.2f} ({1e3 * min(t[S]):8.2f} .. {1e3 * max(t[S]):8.2f})   {1e3 * med / P:8.3f}      {S * P / med:8.1f}              {ok}/{S * P}      {same}")

    # one sequence: the new entry beside vo_slam_chain, on the same resident run
    resident(1)
    one = lambda: fe.slam_chain(P, K)                      # noqa: E731
    many = lambda: fe.slam_chains([P], K)                  # noqa: E731
    one(); many(); one(); many()
    t1, tm = [], []
    for _ in range(args.repeats_single):
        dt, a = timed(one); t1.append(dt)
        dt, b = timed(many); tm.append(dt)
    same = all(np.array_equal(a[k], b[0][k]) for k in OUT_KEYS)
    print(f"one sequence of {P} pairs on the same resident run, alternating, medians of {args.repeats_single}:")
    for label, v in (("slam_chain(15)    ", t1), ("slam_chains([15]) ", tm)):
        print(f"  {label} {1e3 * statistics.median(v):8.2f} ms per call (min {1e3 * min(v):8.2f} max {1e3 * max(v):8.2f})   {1e3 * statistics.median(v) / P:7.3f} ms per frame")
    print(f"  outputs identical: {same}")

    names = dict(misc="chain steps", slam_ba_prepare="k_slam_ba_prepare", slam_bundle_adjust="k_bundle_adjust", slam_filter="k_slam_filter",
                 slam_camera_limit="k_slam_limit")
    print("split (event brackets on, 3 calls; ms per step = per frame of every sequence) and the maps at the end:")
    print("  S   " + "".join(f"{v:>20s}" for v in names.values()) + "      sum   cameras / points / observations (largest map)")
    for S in args.sequences:
        resident(S)
        fe.profile(True)
        for _ in range(3):
            fe.slam_chains([P] * S, K)
        prof = fe.profile_read()
        fe.profile(False)
        ms = [prof.get(k, (0.0, 0))[0] / 3 / P for k in names]
        maps = [fe.slam_map(0, seq=s) for s in range(S)]
        big = max(maps, key=lambda m: len(m["obs_cam"]))
        print(f" {S:2d}   " + "".join(f"{v:20.4f}" for v in ms) + f" {sum(ms):8.4f}   {len(big['cam_frame'])} / {len(big['points'])} / {len(big['obs_cam'])}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurement of FrontEnd.epipolar_stats (vo_pairs_epipolar / k_pairs_epipolar): --pairs consecutive ORB pairs of the closed synthetic
flight, resident in HBM, vo_pairs_run untimed before; what is timed is the statistics call alone (upload of K, one launch, the
downloads), with and without the per-inlier distances, and the kernel's own event bracket (stage `misc`).  Medians of --repeats calls
after a warm-up.  Prints a text report; nothing here is a pass / fail number."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from visual_odometry_amd import synth  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--distinct-frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=21)
    args = ap.parse_args()
    P = args.pairs
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:P + 1], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=P + 1, max_pairs=P, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, P + 1)
    res, _ = fe.run_pairs([[k, k + 1] for k in range(P)], K)
    n_inl = res["n_inl"].copy()

    def timed(want_dist):
        out = []
        for _ in range(args.repeats + 3):
            t = time.perf_counter(); fe.epipolar_stats(K, want_dist=want_dist); out.append((time.perf_counter() - t) * 1e3)
        return out[3:]

    plain, with_dist = timed(False), timed(True)
    fe.profile(True)
    for _ in range(args.repeats):
        fe.epipolar_stats(K)
    ms, launches = fe.profile_read()["misc"]                    # (summed ms, launches) of the stage the kernel is bracketed as
    k_ms = ms / max(launches, 1)
    fe.profile(False)
    st = fe.epipolar_stats(K)
    print(f"{P} pairs {args.width}x{args.height}, {args.nfeatures} ORB features, kp_cap {fe.kp_cap}; inliers per pair: mean {n_inl.mean():.1f}, max {n_inl.max()}")
    print(f"epipolar_stats(K)                 median {statistics.median(plain):.3f} ms  (min {min(plain):.3f}, max {max(plain):.3f}; {args.repeats} calls)")
    print(f"epipolar_stats(K, want_dist=True) median {statistics.median(with_dist):.3f} ms  (min {min(with_dist):.3f}, max {max(with_dist):.3f})")
    print(f"k_pairs_epipolar event bracket    {k_ms:.4f} ms per launch of {P} workgroups")
    print(f"mean distance over the pairs {st['mean'].mean():.4f} px, largest {st['max'].max():.4f} px")


if __name__ == "__main__":
    main()

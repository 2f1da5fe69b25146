#!/usr/bin/env python3
"""Measurement of the map statistics of the resident map (vo_set_slam_stats / FrontEnd.map_stats) on the chunk bench_slam_chain.py
uses — 64 consecutive 1280x720 ORB pairs of the closed flight, 2000 features, resident in HBM, the reference's defaults:
slam_chain with statistics off and on, alternating in one process, medians of --repeats calls each after a warm-up, then a pass
with the library's event brackets on that splits the on-call's time, the statistics kernel's bracket included.
The yardstick is the off median of this same job: with the switch off the call's launches are the parent's (the host loops
launch k_slam_stats only behind the switch, and tests/test_gpu_slam_stats.py finds every output byte-identical).  Margin of an
off / off comparison: this job's own max - min spread of the off runs plus 1 %.  There is no pass bar on the on-cost.
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
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="shader clock assumed when the bracket is turned into cycles (not measured here)")
    args = ap.parse_args()
    n = args.pairs + 1
    seq = synth.sequence(args.distinct_frames, args.width, args.height, cache_dir="/tmp", trajectory="loop")
    frames, K = seq["frames"][:n], seq["K"]
    fe = FrontEnd(args.height, args.width, max_frames=n, max_pairs=n - 1, nfeatures=args.nfeatures)
    fe.upload(frames); fe.detect(0, n)
    fe.run_pairs(np.stack([np.arange(n - 1), np.arange(n - 1) + 1], 1).astype(np.int32), K, want_points=True)

    def slam(on):
        fe.map_stats(on)
        return fe.slam_chain(n - 1, K)

    for on in (False, True, False, True):                # warm-up: allocations, code objects
        slam(on)
    t_off, t_on = [], []
    for _ in range(args.repeats):
        dt, off = timed(lambda: slam(False))
        t_off.append(dt)
        dt, out = timed(lambda: slam(True))
        t_on.append(dt)
    st = fe.slam_stats()
    same = all(np.asarray(off[k]).tobytes() == np.asarray(out[k]).tobytes() for k in off)
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    fe.profile(True)
    for _ in range(3):
        slam(True)
    prof = fe.profile_read()
    fe.profile(False)
    fe.map_stats(False)
    p = n - 1
    spread = (max(t_off) - min(t_off)) / m_off
    print(f"chunk: {p} consecutive {args.width}x{args.height} ORB pairs, {args.nfeatures} features, one MI355X, one context; medians of {args.repeats} alternating calls")
    print(f"slam_chain, statistics off: {1e3 * m_off / p:.4f} ms/frame  {p / m_off:.1f} frames/s   min {1e3 * min(t_off) / p:.4f} max {1e3 * max(t_off) / p:.4f} ms/frame")
    print(f"slam_chain, statistics on : {1e3 * m_on / p:.4f} ms/frame  {p / m_on:.1f} frames/s   min {1e3 * min(t_on) / p:.4f} max {1e3 * max(t_on) / p:.4f} ms/frame")
    print(f"on - off: {1e3 * (m_on - m_off) / p:+.4f} ms/frame ({100 * (m_on / m_off - 1):+.2f} %); spread of the off runs (max - min) {100 * spread:.2f} %, "
          f"margin of an off / off comparison {100 * spread + 1:.2f} %; outputs of the last off and on call byte-identical: {same}")
    n_obs = out["n_obs"].astype(np.int64)
    print(f"map per pair: observations mean {n_obs.mean():.0f} max {int(n_obs.max())}, points max {int(out['n_pts'].max())}, cameras max {int(out['n_cam'].max())}; "
          f"last row: mean sqerr {st['mean_sqerr'][-1]:.4f}, max {st['max_sqerr'][-1]:.3f}, n_high {int(st['n_high'][-1])}, "
          f"points with 0 / 1 / 2 observations {st['obs_hist'][-1][:3].tolist()}, newest camera's column of the matrix sums to {int(st['obs_matrix'][-1].sum(0)[int(out['n_cam'][-1]) - 1])}")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import map_stats_reference as R                        # the plain-Python checker, on the map the last call left
    m = fe.slam_map(0)
    want, nc = R.stats(m, K), len(m["cam_frame"])
    exact = (np.float64(want["total_sqerr"]).tobytes() == st["total_sqerr"][-1].tobytes() and np.float64(want["max_sqerr"]).tobytes() == st["max_sqerr"][-1].tobytes()
             and want["n_high"] == st["n_high"][-1] and np.array_equal(want["obs_hist"], st["obs_hist"][-1])
             and np.array_equal(want["obs_matrix"], st["obs_matrix"][-1][:nc, :nc]) and st["cam_frame"][-1][:nc].tolist() == m["cam_frame"].tolist())
    print(f"last row against the checker on slam_map(0) ({nc} cameras, {len(m['points'])} points, {len(m['obs_cam'])} observations), bytes and integers: {'equal' if exact else 'DIFFERENT'}; "
          f"newest camera with the one before it: {int(st['obs_matrix'][-1][nc - 2, nc - 1])} points, checker {int(want['obs_matrix'][nc - 2, nc - 1])}")
    print("slam_chain split, statistics on (event brackets on, 3 calls; ms per frame, brackets per call):")
    names = dict(misc="chain steps (gather, solvePnPRansac, pose, triangulate, add)", slam_ba_prepare="k_slam_ba_prepare", slam_bundle_adjust="k_bundle_adjust",
                 slam_filter="k_slam_filter", slam_camera_limit="k_slam_limit", slam_map_statistics="k_slam_stats")
    total = 0.0
    for key, label in names.items():
        t, cnt = prof.get(key, (0.0, 0))
        total += t
        print(f"  {label:62s} {t / 3 / p:8.4f} ms/frame   {cnt // 3:4d} brackets")
    print(f"  {'sum of the brackets':62s} {total / 3 / p:8.4f} ms/frame")
    t_stats, cnt = prof.get("slam_map_statistics", (0.0, 0))
    if cnt:
        per_launch_us = 1e3 * t_stats / cnt
        cyc_per_obs = per_launch_us * 1e-6 * args.clock_ghz * 1e9 / max(n_obs.mean(), 1)
        print(f"k_slam_stats bracket: {per_launch_us:.1f} us per launch, {1e3 * per_launch_us / max(n_obs.mean(), 1):.2f} ns per observation of the mean map "
              f"= {cyc_per_obs:.1f} cycles per observation at an ASSUMED {args.clock_ghz} GHz (the bracket includes the launch; one dependent f64 add is a few cycles)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""vo_map_align_guided's matching stage against vo_map_align's, in the same process on the same data (docs/kernels/k_map_fuse.md,
Measured):
    python tests/scripts/bench_map_align_guided.py [--reps 9] [--maps 4096,65536] [--out profiles/map_align_guided_bench.txt]
ORB and SIFT rows; staged maps of 4096 and 65536 points, uniform in a box 4 units thick at 16 points per unit volume; Q = 8 query maps
of 8192 points, half of them staged points seen again (a gauge of its own per map, Gaussian noise of 0.004 per axis, rows nudged) and
half new points in the same box; the priors are the generating similarities perturbed by 0.002 rad and 0.01 units.  Three radii that
put about 1, 8 and 64 staged points in a sphere at that density.
What is compared is match_nn + match_select from the stage brackets: k_align_gather + k_nn_align + k_align_select for vo_map_align,
k_align_gather + the claim table's memset + k_fuse_grid + k_fuse_match + k_fuse_select for the guided call.  Median and range over
--reps calls after a warm-up call; no threshold is set on them."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import relocalize_reference as R  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--maps", default="4096,65536")
ap.add_argument("--queries", type=int, default=8)
ap.add_argument("--rows", type=int, default=8192)
ap.add_argument("--per-sphere", default="1,8,64")
ap.add_argument("--out", default="")
args = ap.parse_args()
Q, N, MAX_ERROR, DENSITY, THICK = args.queries, args.rows, 0.05, 16.0, 4.0
radii = [(k, float(np.cbrt(3 * k / (4 * np.pi * DENSITY)))) for k in (int(v) for v in args.per_sphere.split(","))]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scene(det, npt, seed):
    rng = np.random.default_rng(seed)
    side = float(np.sqrt(npt / (DENSITY * THICK)))
    box = lambda n: np.column_stack([rng.uniform(0, side, n), rng.uniform(0, side, n), rng.uniform(0, THICK, n)])
    X = box(npt)
    rows = R.rand_rows(rng, npt, det)
    dR = R.rotation([0.3, -0.5, 0.8], 0.002)
    q_rows, q_pts, priors = [], [], []
    for q in range(Q):
        s = float(rng.uniform(0.5, 2)); Rm = R.rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)); t = rng.uniform(-4, 4, 3)
        n_dup = min(N // 2, npt)
        ids = rng.choice(npt, n_dup, replace=False)
        y = np.concatenate([X[ids] + rng.normal(0, 0.004, (n_dup, 3)), box(N - n_dup)])
        f = R.rand_rows(rng, N, det)
        f[:n_dup] = rows[ids]
        f[:n_dup, :2] ^= rng.integers(0, 2, (n_dup, 2), dtype=np.uint8)    # near, not equal
        order = rng.permutation(N)
        q_rows.append(f[order]); q_pts.append(((y - t) @ Rm / s)[order])
        priors.append(np.concatenate([[s * 1.0002], (dR @ Rm).reshape(9), dR @ t + np.array([0.01, -0.006, 0.008])]))
    return X, rows, np.concatenate(q_rows), np.concatenate(q_pts), np.stack(priors)


def timed(fe, call):
    """(median, min, max) of match_nn + match_select in ms over --reps calls, and the last result"""
    call()
    ts = []
    for _ in range(args.reps):
        fe.profile(True)
        out = call()
        p = fe.profile_read()
        ts.append(p["match_nn"][0] + p["match_select"][0])
    fe.profile(False)
    ts.sort()
    return (ts[len(ts) // 2], ts[0], ts[-1]), out


off = np.arange(Q + 1, dtype=np.int32) * N
for det in ("orb", "sift"):
    if det == "sift":
        fe = FrontEnd(32, 32, max_frames=1, max_pairs=1, detector="sift", kp_cap=64)
    else:
        fe = FrontEnd(64, 64, max_frames=1, max_pairs=1, nfeatures=64, nlevels=1)
    for npt in [int(v) for v in args.maps.split(",")]:
        X, rows, q_rows, q_pts, priors = scene(det, npt, 3000 + npt)
        fe.stage_map(rows, X)
        (med, lo, hi), out = timed(fe, lambda: fe.align_maps(q_rows, q_pts, MAX_ERROR, offsets=off))
        say(f"{det} staged {npt}, {Q} query maps x {N} rows")
        say(f"  brute force             match_nn + match_select {med:9.3f} ms (range {lo:.3f} .. {hi:.3f}, {args.reps} reps); "
            f"matches {out['n_match'].mean():.0f}, inliers {out['n_inl'].mean():.0f} per map, ok {int((out['status'] == 0).sum())}/{Q}")
        for k, r in radii:
            (gm, glo, ghi), g = timed(fe, lambda: fe.align_maps_guided(q_rows, q_pts, priors, r, MAX_ERROR, offsets=off))
            say(f"  guided ~{k:2d}/sphere r={r:.3f} match_nn + match_select {gm:9.3f} ms (range {glo:.3f} .. {ghi:.3f}); matches {g['n_match'].mean():.0f}, "
                f"inliers {g['n_inl'].mean():.0f}, points seen {g['n_seen'].mean():.0f} per map, ok {int((g['status'] == 0).sum())}/{Q}; "
                f"brute force / guided = {med / max(gm, 1e-9):.2f}")
    fe.ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")

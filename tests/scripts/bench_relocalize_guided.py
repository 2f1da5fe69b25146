#!/usr/bin/env python3
"""The matching stage of vo_map_localize_guided next to that of vo_map_localize (docs/kernels/k_map_guided.md, Measured):
    python tests/scripts/bench_relocalize_guided.py [--reps 9] [--frames 8] [--maps 4096,65536] [--radii 8,32,128] [--out FILE.json]
On the same staged map and the same Q slots of 2000 keypoints, for both detectors: match_nn + match_select of one
FrontEnd.relocalize call (k_nn_map / k_nn_map_orb both ways + k_map_select: every keypoint against every point) and of one
FrontEnd.relocalize_guided call per radius (k_guided_grid + k_guided_match + k_guided_select), from the stage brackets, with
matches and inliers of each.  Every frame sees 2000 of the map's points from a pose of its own — their rows with a few elements
nudged, float32 projections, 10 % of them at a wrong pixel — and the prior is that pose turned by 0.002 rad and moved by 0.01 units
(about 3 px).  Each timed call is preceded by a warm-up call of the same shape; times are the median and the range over --reps
calls, each read from a profile reset of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import relocalize_reference as R  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rows", type=int, default=2000)
ap.add_argument("--maps", default="4096,65536")
ap.add_argument("--radii", default="8,32,128")
ap.add_argument("--out", default=None, help="write the table as JSON")
args = ap.parse_args()
Q, N = args.frames, args.rows
radii = [float(v) for v in args.radii.split(",")]


def scene(det, npt, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (npt, 3))
    rows = R.rand_rows(rng, npt, det)
    frames, priors = [], []
    dR = R.rotation([0.3, -0.5, 0.8], 0.002)
    for q in range(Q):
        Rm = R.rotation(rng.normal(size=3), rng.uniform(0.05, 0.4)); t = np.array([0.3, -0.2, 6.0]) + rng.normal(0, 0.3, 3)
        ids = rng.choice(npt, min(N, npt), replace=False)
        Xc = X[ids] @ Rm.T + t
        uv = ((Xc / Xc[:, 2:]) @ R.K.T)[:, :2]
        wrong = rng.random(len(ids)) < 0.1
        uv[wrong] += rng.uniform(40, 120, (int(wrong.sum()), 2))
        f = np.stack([R.nudge(r, int(k), det) for r, k in zip(rows[ids], rng.integers(0, 3, len(ids)))])
        frames.append((f, uv.astype(np.float32)))
        priors.append(np.hstack([dR @ Rm, (dR @ t + np.array([0.01, -0.006, 0.008])).reshape(3, 1)]))
    return X, rows, frames, np.stack(priors)


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


table = []
for det in ("orb", "sift"):
    if det == "sift":
        fe = FrontEnd(32, 32, max_frames=Q, max_pairs=Q, detector="sift", kp_cap=N)
    else:
        fe = FrontEnd(64, 64, max_frames=Q, max_pairs=Q, nfeatures=N, nlevels=1)
    slots = np.arange(Q, dtype=np.int32)
    for npt in [int(v) for v in args.maps.split(",")]:
        X, rows, frames, priors = scene(det, npt, 2000 + npt)
        for q, (f, xy) in enumerate(frames):
            (fe.set_sift_rows if det == "sift" else fe.set_orb_rows)(q, f, xy)
        fe.stage_map(rows, X)
        (med, lo, hi), out = timed(fe, lambda: fe.relocalize(slots, R.K))
        print(f"{det} map {npt}, {Q} slots x {N} keypoints (kp_cap {fe.kp_cap})")
        print(f"  brute force      match_nn + match_select {med:8.3f} ms (range {lo:.3f} .. {hi:.3f}, {args.reps} reps); "
              f"matches {out['n_match'].mean():.0f}, inliers {out['n_inl'].mean():.0f} per frame, ok {int((out['status'] == 0).sum())}/{Q}")
        table.append(dict(detector=det, map=npt, call="vo_map_localize", radius=None, ms=med, ms_min=lo, ms_max=hi,
                          matches=float(out["n_match"].mean()), inliers=float(out["n_inl"].mean())))
        for r in radii:
            (gm, glo, ghi), g = timed(fe, lambda: fe.relocalize_guided(slots, R.K, priors, r))
            print(f"  guided {r:5g} px  match_nn + match_select {gm:8.3f} ms (range {glo:.3f} .. {ghi:.3f}); matches {g['n_match'].mean():.0f}, "
                  f"inliers {g['n_inl'].mean():.0f}, points seen {g['n_seen'].mean():.0f} per frame, ok {int((g['status'] == 0).sum())}/{Q}; "
                  f"{med / gm:.1f}x faster than brute force" if gm > 0 else "")
            table.append(dict(detector=det, map=npt, call="vo_map_localize_guided", radius=r, ms=gm, ms_min=glo, ms_max=ghi,
                              matches=float(g["n_match"].mean()), inliers=float(g["n_inl"].mean()), seen=float(g["n_seen"].mean())))
    fe.ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(frames=Q, keypoints=N, reps=args.reps, rows=table), fh, indent=1)

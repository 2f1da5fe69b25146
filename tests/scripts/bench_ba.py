#!/usr/bin/env python3
"""Measurement of the bundle-adjustment row (Map.optimize_map, src/map.py:104-186): B independent maps of the reference's
steady-state shape (18 cameras, 2 of them free, as freeze_nonlast_cameras leaves them) per launch on one MI355X, beside the
numpy restatement (tests/ba_reference.py) on a bounded sample of the same maps.  Prints one JSON line.  There is no earlier
bundle adjustment to compare with, so there is no target."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ba_reference as R  # noqa: E402
from visual_odometry_amd import _lib, map_filters as mf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--cameras", type=int, default=18)
    ap.add_argument("--free", type=int, default=2)
    ap.add_argument("--points", type=int, default=600)
    ap.add_argument("--visibility", type=float, default=0.4)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=4)
    args = ap.parse_args()
    maps = [R.make_map(5000 + b, ncam=args.cameras, npt=args.points, nfixed=args.cameras - args.free, vis=args.visibility)
            for b in range(args.problems)]
    probs = [R.args(m) for m in maps]
    nobs = np.array([len(m["oc"]) for m in maps])
    ctx = _lib.default_context()
    mf.bundle_adjust_batch(probs[:2], R.F0, R.CX, R.CY, args.iterations, ctx=ctx)                     # warm-up
    ctx.check(ctx.lib.vo_profile_enable(ctx.handle, 1)); ctx.check(ctx.lib.vo_profile_reset(ctx.handle))
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = mf.bundle_adjust_batch(probs, R.F0, R.CX, R.CY, args.iterations, ctx=ctx)
    dt = (time.perf_counter() - t0) / args.steps
    ms = np.zeros(_lib.VO_STAGE_COUNT, np.float32); cnt = np.zeros(_lib.VO_STAGE_COUNT, np.int32)
    ctx.check(ctx.lib.vo_profile_read(ctx.handle, ms.ctypes.data, cnt.ctypes.data))
    ctx.check(ctx.lib.vo_profile_enable(ctx.handle, 0))
    names = [ctx.lib.vo_stage_name(i).decode() for i in range(_lib.VO_STAGE_COUNT)]
    kernel_ms = float(ms[names.index("misc")] / max(cnt[names.index("misc")], 1))
    one = time.perf_counter()
    mf.bundle_adjust(*probs[0], R.F0, R.CX, R.CY, args.iterations, ctx=ctx)
    one = time.perf_counter() - one
    n_cpu = min(args.problems, args.cpu_sample)
    t1 = time.perf_counter()
    same, worst = 0, 0.0
    for b in range(n_cpu):
        r = R.lm(*probs[b], iterations=args.iterations)
        same += int((r["iterations"], r["trials"]) == (out[b]["iterations"], out[b]["trials"]))
        worst = max(worst, float(np.abs(r["poses"] - out[b]["poses"]).max()), float(np.abs(r["points"] - out[b]["points"]).max()))
    cpu = (time.perf_counter() - t1) / max(n_cpu, 1)
    print(json.dumps({
        "metric": "bundle adjustments/s", "value": round(args.problems / dt, 1), "unit": "problems/s", "n_gpus": 1,
        "config": {"problems_per_launch": args.problems, "cameras": args.cameras, "free_cameras": args.free, "points_per_problem": args.points,
                   "observations_per_problem_mean": float(nobs.mean()), "observations_per_problem_max": int(nobs.max()),
                   "iterations": args.iterations, "huber_delta": 1.0},
        "ms_per_launch_with_copies": round(1000 * dt, 3), "kernel_ms_per_launch": round(kernel_ms, 3),
        "problems_per_s_kernel_only": round(args.problems / (kernel_ms * 1e-3), 1) if kernel_ms > 0 else None,
        "ms_single_problem_call_with_copies": round(1000 * one, 3),
        "ok_fraction": float(np.mean([o["status"] == 0 for o in out])), "mean_trials": float(np.mean([o["trials"] for o in out])),
        "mean_iterations": float(np.mean([o["iterations"] for o in out])),
        "mean_chi2_before": float(np.mean([o["chi2_before"] for o in out])), "mean_chi2_after": float(np.mean([o["chi2_after"] for o in out])),
        "cpu_baseline": {"value": round(1.0 / cpu, 3), "unit": "problems/s", "cores": 1, "kind": "numpy restatement, not a g2o timing",
                         "sample": f"{n_cpu} of the same problems through tests/ba_reference.py, one thread",
                         "same_iterations_and_trials": f"{same}/{n_cpu}", "max_abs_difference": worst}}))


if __name__ == "__main__":
    main()

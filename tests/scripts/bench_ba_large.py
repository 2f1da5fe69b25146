#!/usr/bin/env python3
"""vo_bundle_adjust_large through its stage bracket (docs/kernels/k_bundle_adjust_large.md):
    python tests/scripts/bench_ba_large.py [--free 64 128 256 512] [--phases DIR]
One map each of 64, 128, 256 and 512 free cameras (plus two fixed ones), banded visibility: cameras along a line, every point seen
by about 8 consecutive cameras, about 300 points per camera; 10 iterations; the median of 5 calls after a warm-up.  The time is
vo_profile_read's `misc` bracket: hipEvents around the whole LM loop, i.e. every kernel, the clears of S and the host's reads of the
decision record, without the upload of the lists and the download of the result.  Beside it the numpy checker
(tests/ba_reference.lm) on the 64- and 128-camera maps; both must agree to 1e-6 before a time is printed.  No threshold is set on
any figure.
Per-phase times are taken in a run of their own, because tracing slows the host:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/scripts/bench_ba_large.py --free 256 --once
    python tests/scripts/bench_ba_large.py --phases DIR
--phases reads the kernel statistics rocprofv3 left under DIR and adds the kernels up by phase (linearise, build S, factor, step and
cost), per trial.  The factorisation's f64 rate is the dense count n^3 / 3 (n = 6 F) per trial over the time of its kernels."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ba_reference as R  # noqa: E402

REPS, ITER = 5, 10
PHASES = {"linearise": ("k_gba_lin_points", "k_gba_lin_cams", "k_gba_lambda0"), "build S": ("k_gba_hpi", "k_gba_build", "fillBuffer", "memset"),
          "factor": ("k_gba_panel", "k_gba_update", "k_gba_backsub"), "step and cost": ("k_gba_step_cams", "k_gba_step_points", "k_gba_decide")}


banded_map = R.banded_map                            # seed 0, 300 points per camera: the defaults


def misc_ms(ctx, _lib):
    ms = np.zeros(_lib.VO_STAGE_COUNT, np.float32); n = np.zeros(_lib.VO_STAGE_COUNT, np.int32)
    ctx.check(ctx.lib.vo_profile_read(ctx.handle, ms.ctypes.data, n.ctypes.data))
    i = [ctx.lib.vo_stage_name(k).decode() for k in range(_lib.VO_STAGE_COUNT)].index("misc")
    assert n[i] == 1
    return float(ms[i])


def measure(frees, once):
    from visual_odometry_amd import _lib, map_filters
    ctx = _lib.default_context()
    ctx.check(ctx.lib.vo_profile_enable(ctx.handle, 1))
    for free in frees:
        m = banded_map(free)
        call = lambda: map_filters.bundle_adjust_large(*m, R.F0, R.CX, R.CY, iterations=ITER, ctx=ctx)  # noqa: E731
        out = call()                                                          # warm-up
        if once:
            print(f"F = {free}: one call after the warm-up, {call()['trials']} trials")
            continue
        times = []
        for _ in range(REPS):
            ctx.check(ctx.lib.vo_profile_reset(ctx.handle))
            t0 = time.perf_counter(); out = call(); wall = time.perf_counter() - t0
            times.append((misc_ms(ctx, _lib), wall * 1e3))
        med = float(np.median([t[0] for t in times])); lo = min(t[0] for t in times); hi = max(t[0] for t in times)
        n = 6 * free
        line = (f"F = {free}: {len(m[0])} cameras, {len(m[2])} points, {len(m[3])} observations, chi2 {out['chi2_before']:.6g} -> {out['chi2_after']:.6g}, "
                f"{out['iterations']} iterations, {out['trials']} trials: misc {med:.2f} ms (min {lo:.2f}, max {hi:.2f}, {REPS} calls) = {med / out['trials']:.3f} ms per trial; "
                f"whole call (lists, upload, download) {np.median([t[1] for t in times]):.1f} ms; dense factor count {n ** 3 / 3 / 1e9:.3f} GFLOP per trial")
        if free <= 128:
            t0 = time.perf_counter(); ref = R.lm(*m, iterations=ITER); cpu = time.perf_counter() - t0
            d = max(float(np.abs(out["poses"] - ref["poses"]).max()), float(np.abs(out["points"] - ref["points"]).max()))
            assert (out["iterations"], out["trials"]) == (ref["iterations"], ref["trials"]) and d < 1e-6 and abs(out["chi2_after"] - ref["chi2_after"]) <= 1e-6 * ref["chi2_after"], (d, out["chi2_after"], ref["chi2_after"])
            line += f"; numpy checker {cpu:.2f} s, largest |gpu - cpu| {d:.1e}"
        print(line, flush=True)


def phases(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no *kernel_stats.csv under {directory}"
    total = {k: 0.0 for k in PHASES}; calls = {k: 0 for k in PHASES}; other = 0.0
    decide = 0
    for path in files:
        for row in csv.DictReader(open(path)):
            name, ns, n = row["Name"], float(row["TotalDurationNs"]), int(row["Calls"])
            if "k_gba_decide" in name:
                decide += n
            for ph, keys in PHASES.items():
                if any(k in name for k in keys):
                    total[ph] += ns; calls[ph] += n
                    break
            else:
                other += ns
    assert decide, "no k_gba_decide in the trace"
    print(f"{decide} trials in the trace (warm-up included); kernel time per trial, linearise per iteration counted over the trials:")
    for ph in PHASES:
        print(f"  {ph:<14} {total[ph] / decide / 1e6:9.3f} ms  ({calls[ph] / decide:.1f} launches)")
    print(f"  other kernels  {other / decide / 1e6:9.3f} ms")
    return total, decide


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--free", type=int, nargs="+", default=[64, 128, 256, 512])
    ap.add_argument("--once", action="store_true", help="a warm-up and one call per map, no timing: the run to trace")
    ap.add_argument("--phases", metavar="DIR", help="add up rocprofv3's kernel statistics under DIR by phase")
    a = ap.parse_args()
    if a.phases:
        total, trials = phases(a.phases)
        if len(a.free) == 1:
            n = 6 * a.free[0]
            print(f"  factorisation: {n ** 3 / 3 / 1e9:.3f} GFLOP per trial over {total['factor'] / trials / 1e6:.3f} ms = {n ** 3 / 3 / (total['factor'] / trials) :.2f} GFLOP/s (f64)")
        return
    measure(a.free, a.once)


if __name__ == "__main__":
    main()

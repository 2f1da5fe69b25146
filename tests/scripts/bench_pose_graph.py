#!/usr/bin/env python3
"""k_pose_graph through its stage bracket (docs/kernels/k_pose_graph.md):
    python tests/scripts/bench_pose_graph.py
(a) 256 graphs of N = 64 with 4 loop edges in one launch, (b) one graph of N = 4096 with 32 loop edges; 10 iterations each.  Beside
the kernel the checker's rules restated with scipy.sparse on the CPU (the same Levenberg-Marquardt, H in CSC, a sparse LU of
H + lambda I); both paths must agree before a time is printed.  Kernel time is vo_profile_read's `misc` bracket (hipEvents around
the launch, copies excluded), the median of REPS launches after a warm-up; no threshold is set on any figure."""
import os
import sys
import time

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pose_graph_reference as P  # noqa: E402
from visual_odometry_amd import _lib, map_filters  # noqa: E402

REPS, ITER = 5, 10


def optimize_sparse(sims, fixed, edges, meas, info, iterations):
    """pose_graph_reference.optimize with the dense Hessian replaced by CSC + splu (no Huber; a singular LU is a failed trial)"""
    S = np.array(sims, np.float64).reshape(-1, 13).copy()
    fixed = np.asarray(fixed).astype(bool); edges = np.asarray(edges, np.int64)
    free = np.flatnonzero(~fixed); col = -np.ones(len(S), np.int64); col[free] = np.arange(len(free)); n = 7 * len(free)
    Ji = [P.adjoint(c) for c in meas]

    def evaluate(Sx):
        out = [P.edge_error(meas[k], Sx[i], Sx[j]) for k, (i, j) in enumerate(edges.tolist())]
        return float(sum(float((info[k] * e * e).sum()) for k, (e, _) in enumerate(out))), out

    cur, ee = evaluate(S)
    chi0, lam, ni, trials, n_it = cur, None, 2.0, 0, 0
    for _ in range(iterations):
        n_it += 1
        rows, cols, vals = [], [], []
        b = np.zeros(n)
        for k, (i, j) in enumerate(edges.tolist()):
            J = {i: Ji[k], j: -P.adjoint(ee[k][1])}
            for a in (i, j):
                if col[a] < 0:
                    continue
                b[7 * col[a]:7 * col[a] + 7] -= J[a].T @ (info[k] * ee[k][0])
                for c in (i, j):
                    if col[c] >= 0:
                        blk = J[a].T @ (info[k][:, None] * J[c])
                        r0, c0 = 7 * col[a], 7 * col[c]
                        rows.append(np.repeat(np.arange(r0, r0 + 7), 7)); cols.append(np.tile(np.arange(c0, c0 + 7), 7)); vals.append(blk.ravel())
        H = scipy.sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()
        if lam is None:
            lam = 1e-5 * H.diagonal().max()
        rho, q_max = 0.0, 0
        while True:
            trials += 1
            try:
                d = scipy.sparse.linalg.splu(H + lam * scipy.sparse.identity(n, format="csc")).solve(b)
                ok = bool(np.all(np.isfinite(d)))
            except RuntimeError:
                ok = False
            rho = -1.0
            if ok:
                S2 = S.copy()
                for c, v in enumerate(free):
                    S2[v] = P.sim3_compose(P.sim3_exp(d[7 * c:7 * c + 7]), S[v])
                tmp, ee2 = evaluate(S2)
                scale = float((d * (lam * d + b)).sum())
                if np.isfinite(tmp) and np.isfinite(scale) and scale > 0:
                    rho = (cur - tmp) / scale
            if rho > 0:
                t3 = 2 * rho - 1
                lam *= max(1.0 / 3.0, min(1.0 - t3 * t3 * t3, 2.0 / 3.0)); ni = 2.0
                cur, ee, S = tmp, ee2, S2
            else:
                lam *= ni; ni *= 2
            q_max += 1
            if not (rho < 0 and q_max < 10):
                break
        if q_max == 10 or rho == 0 or not np.isfinite(lam):
            break
    return dict(sims=S, chi2_initial=chi0, chi2_final=cur, iterations=n_it, trials=trials)


def kernel_ms(ctx, problems):
    map_filters.optimize_pose_graph_batch(problems, iterations=ITER, ctx=ctx)            # warm-up
    times = []
    for _ in range(REPS):
        ctx.check(ctx.lib.vo_profile_reset(ctx.handle))
        out = map_filters.optimize_pose_graph_batch(problems, iterations=ITER, ctx=ctx)
        ms = np.zeros(_lib.VO_STAGE_COUNT, np.float32); n = np.zeros(_lib.VO_STAGE_COUNT, np.int32)
        ctx.check(ctx.lib.vo_profile_read(ctx.handle, ms.ctypes.data, n.ctypes.data))
        i = [ctx.lib.vo_stage_name(k).decode() for k in range(_lib.VO_STAGE_COUNT)].index("misc")
        assert n[i] == 1
        times.append(float(ms[i]))
    return out, float(np.median(times)), min(times), max(times)


def agree(name, got, ref):
    d = float(np.abs(got["sims"] - ref["sims"]).max())
    assert got["status"] == 0 and d < 1e-6 and abs(got["chi2_final"] - ref["chi2_final"]) <= 1e-6 * max(ref["chi2_final"], 1e-12), (name, d, got["chi2_final"], ref["chi2_final"])
    return d


def main():
    ctx = _lib.default_context()
    ctx.check(ctx.lib.vo_profile_enable(ctx.handle, 1))
    # (a) the batch
    graphs = [P.make_graph(64, [(0, 63), (8, 40), (16, 56), (24, 48)], seed=100 + b, noise=1e-3) for b in range(256)]
    out, med, lo, hi = kernel_ms(ctx, [P.args(g) for g in graphs])
    t0 = time.perf_counter()
    refs = [optimize_sparse(*P.args(g), ITER) for g in graphs[:8]]
    cpu = (time.perf_counter() - t0) / 8
    worst = max(agree(f"batch {b}", out[b], refs[b]) for b in range(8))
    trials = sum(o["trials"] for o in out)
    print(f"(a) 256 graphs, N = 64, 4 loops, {ITER} iterations ({trials} trials in all): kernel {med:.3f} ms (min {lo:.3f}, max {hi:.3f}, {REPS} launches) "
          f"= {256 / med * 1e3:.0f} graphs/s; CPU scipy.sparse {cpu * 1e3:.1f} ms per graph = {1 / cpu:.1f} graphs/s; largest |gpu - cpu| on 8 graphs {worst:.1e}")
    # (b) one long flight
    g = P.make_graph(4096, [(128 * k, 4095 - 127 * k) for k in range(16)] + [(64 + 128 * k, 2048 + 64 * k + 1) for k in range(16)], seed=7, noise=1e-3, scale_drift=2e-4)
    out, med, lo, hi = kernel_ms(ctx, [P.args(g)])
    t0 = time.perf_counter()
    ref = optimize_sparse(*P.args(g), ITER)
    cpu = time.perf_counter() - t0
    d = agree("long", out[0], ref)
    print(f"(b) 1 graph, N = 4096, 32 loops, {ITER} iterations ({out[0]['trials']} trials, chi2 {out[0]['chi2_initial']:.3g} -> {out[0]['chi2_final']:.3g}): "
          f"kernel {med:.2f} ms (min {lo:.2f}, max {hi:.2f}, {REPS} launches) = {1e3 / med:.2f} graphs/s; CPU scipy.sparse {cpu:.1f} s; |gpu - cpu| {d:.1e}")


if __name__ == "__main__":
    main()

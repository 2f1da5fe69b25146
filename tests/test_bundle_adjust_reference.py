"""CPU: the bundle-adjustment checker (tests/ba_reference.py) checked on its own — Jacobians, recovery of the truth,
scipy's Huber minimum, g2o's Levenberg control flow — the summation-order floor the GPU tolerances are derived from, and
the declaration / export of the device entry points."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_analytic_jacobians_equal_central_differences():
    rng = np.random.default_rng(5)
    for _ in range(20):
        dR, dt = R.se3_exp(np.r_[rng.normal(0, 0.3, 3), rng.normal(0, 0.5, 3)])
        T = np.c_[dR, dt][None]
        X = np.array([[rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(5, 12)]])
        xy = np.array([[600.0, 250.0]]); oc = op = np.array([0])
        _, q = R.residuals(T, X, oc, op, xy, R.F0, R.CX, R.CY)
        Jp, Jx = R.jacobians(T, q, oc, R.F0)
        h = 1e-6
        num_p = np.zeros((2, 6)); num_x = np.zeros((2, 3))
        for k in range(6):
            d = np.zeros(6); d[k] = h
            ep = R.residuals(R.pose_update(d, R.quat_from_rot(dR), T[0])[1][None], X, oc, op, xy, R.F0, R.CX, R.CY)[0][0]
            em = R.residuals(R.pose_update(-d, R.quat_from_rot(dR), T[0])[1][None], X, oc, op, xy, R.F0, R.CX, R.CY)[0][0]
            num_p[:, k] = (ep - em) / (2 * h)
        for k in range(3):
            d = np.zeros(3); d[k] = h
            num_x[:, k] = (R.residuals(T, X + d, oc, op, xy, R.F0, R.CX, R.CY)[0][0] - R.residuals(T, X - d, oc, op, xy, R.F0, R.CX, R.CY)[0][0]) / (2 * h)
        assert np.abs(num_p - Jp[0]).max() <= 1e-6 * np.abs(Jp[0]).max()
        assert np.abs(num_x - Jx[0]).max() <= 1e-6 * np.abs(Jx[0]).max()


def test_quaternion_state_keeps_rotations_orthonormal():
    m = R.make_map(3, ncam=6, npt=200, nfixed=2)
    r = R.lm(*R.args(m))
    for T in r["poses"]:
        assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(T[:, :3]) - 1) < 1e-12


def test_zero_noise_recovers_the_truth():
    m = R.make_map(7, ncam=6, npt=200, nfixed=2, noise=0.0, outliers=0.0)
    r = R.lm(*R.args(m))
    assert r["chi2_before"] > 1e3 and r["chi2_after"] < 1e-12 * len(m["oc"])
    assert np.abs(r["poses"] - m["poses_true"]).max() < 1e-8 and np.abs(r["points"] - m["points_true"]).max() < 1e-7
    assert np.array_equal(r["poses"][:2], m["poses"][:2])                       # fixed cameras: untouched


def test_final_chi2_is_scipys_huber_minimum():
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix
    # the gauge-fixed shapes the order floor was first measured on: 6 cameras (2 or 4 fixed, 300 points), 18 cameras (16 fixed, 600 points)
    for seed, ncam, nfixed, npt, vis in ((0, 6, 2, 300, 0.8), (1, 6, 4, 300, 0.8), (2, 18, 16, 600, 0.4), (3, 6, 2, 300, 0.8)):
        m = R.make_map(seed, ncam=ncam, npt=npt, nfixed=nfixed, vis=vis)
        r = R.lm(*R.args(m))
        free = np.flatnonzero(~m["fixed"]); T0, X0, oc, op, xy = r["poses"], r["points"], m["oc"], m["op"], m["xy"]
        nf = 6 * len(free)

        def fun(v):
            T = T0.copy()
            for c, k in enumerate(free):
                T[k] = R.pose_update(v[6 * c:6 * c + 6], R.quat_from_rot(T0[k, :, :3]), T0[k])[1]
            e, _ = R.residuals(T, X0 + v[nf:].reshape(-1, 3), oc, op, xy, R.F0, R.CX, R.CY)
            return np.sqrt((e * e).sum(1))      # scipy's Huber acts per scalar residual, g2o's on the edge's norm: fold the pair into one

        sp = lil_matrix((len(oc), nf + 3 * npt), dtype=int)
        colc = -np.ones(ncam, int); colc[free] = np.arange(len(free))
        for i in range(len(oc)):
            if colc[oc[i]] >= 0:
                sp[i, 6 * colc[oc[i]]:6 * colc[oc[i]] + 6] = 1
            sp[i, nf + 3 * op[i]:nf + 3 * op[i] + 3] = 1
        s = least_squares(fun, np.zeros(nf + 3 * npt), loss="huber", f_scale=1.0, jac_sparsity=sp, xtol=1e-14, ftol=1e-14, gtol=1e-12, max_nfev=200)
        rel = abs(2 * s.cost - r["chi2_after"]) / r["chi2_after"]
        print(f"seed {seed}: LM chi2 {r['chi2_after']:.9f}, scipy polish {2 * s.cost:.9f}, relative difference {rel:.2e}")
        assert rel <= 1e-9


def test_levenberg_control_flow():
    m = R.make_map(41, ncam=4, npt=60, nfixed=2)
    r = R.lm(*R.args(m), iterations=7)
    assert r["iterations"] == 7 and r["trials"] >= 7                          # `iterations` honoured: there is no convergence test
    assert R.lm(*R.args(m), iterations=0)["iterations"] == 0
    # a start far from the minimum (0.5 rad, 1 unit, 4 units off): some steps make the cost worse.  Every rejected trial
    # multiplies lambda by nu = 2, 4, 8, ... (nu doubles until a step is accepted); an accepted one by a factor in [1/3, 2/3]
    m = R.make_map(41, ncam=4, npt=60, nfixed=2, pert_r=0.5, pert_t=1.0, pert_x=4.0)
    trace = []
    r = R.lm(*R.args(m), lam_trace=trace)
    assert len(trace) == r["trials"] == len(r["accepts"]) and r["chi2_after"] < 1e-3 * r["chi2_before"]
    streak, longest = 0, 0
    for i in range(len(trace) - 1):
        ratio = trace[i + 1] / trace[i]
        if r["accepts"][i]:
            assert 1 / 3 - 1e-12 <= ratio <= 2 / 3 + 1e-12
            streak = 0
        else:
            streak += 1; longest = max(longest, streak)
            assert abs(ratio - 2.0 ** streak) <= 1e-12 * ratio, (i, ratio, streak)
    assert longest >= 3
    # a start the first step cannot improve: a free camera nothing constrains (H = 0, lambda = 0: the factorisation fails, which
    # g2o scores as chi2 = DBL_MAX).  Ten failed trials end the run in its first iteration
    trace = []
    r = R.lm(m["poses"], m["fixed"], m["points"], m["oc"][:0], m["op"][:0], m["xy"][:0], lam_trace=trace)
    assert (r["iterations"], r["trials"], sum(r["accepts"])) == (1, 10, 0) and len(trace) == 10
    assert np.array_equal(r["poses"], R.lm(m["poses"], m["fixed"], m["points"], m["oc"][:0], m["op"][:0], m["xy"][:0], iterations=0)["poses"])


def test_edge_behind_the_camera_stays_finite():
    m = R.make_map(43, ncam=4, npt=60, nfixed=2)
    m["points"][5] = [0.1, 0.2, -3.0]                                          # z < 0 in every camera
    m["points"][9, 2] = -m["poses"][2, 2, 3] / m["poses"][2, 2, 2] if m["poses"][2, 2, 2] else 0.0
    r = R.lm(*R.args(m))
    assert np.all(np.isfinite(r["poses"])) and np.all(np.isfinite(r["points"])) and np.isfinite(r["chi2_after"])
    assert r["chi2_after"] <= r["chi2_before"]


def test_degenerate_maps():
    m = R.make_map(44, ncam=3, npt=40, nfixed=3)                               # structure only: no free camera
    r = R.lm(*R.args(m))
    assert np.array_equal(r["poses"], m["poses"]) and r["chi2_after"] < r["chi2_before"]
    m = R.make_map(45, ncam=4, npt=40, nfixed=2)
    keep = m["oc"] != 3                                                        # a free camera without observations: delta = 0
    r = R.lm(m["poses"], m["fixed"], m["points"], m["oc"][keep], m["op"][keep], m["xy"][keep])
    assert np.abs(r["poses"][3] - m["poses"][3]).max() < 1e-15 and r["chi2_after"] < r["chi2_before"]
    r = R.lm(m["poses"], m["fixed"], m["points"], m["oc"][:0], m["op"][:0], m["xy"][:0])     # no observations at all
    assert np.array_equal(r["points"], m["points"]) and r["chi2_after"] == 0 and r["trials"] == 10


@pytest.mark.parametrize("case", R.PARITY_CASES + R.GAUGE_FREE_CASES, ids=lambda c: "seed%d_%dcam_%dfixed_%dpt" % c[:4])
def test_reference_order_floor(case):
    """Two summation orders of the same numpy LM.  The floor per quantity is what test_gpu_bundle_adjust.py multiplies by
    100 (R.tolerances; the measured floors and tolerances are tabulated in that file's header).  A case whose two orders
    take different accept / reject decisions is no parity case and its seed is replaced: see R.PARITY_CASES."""
    gauge_free = case in R.GAUGE_FREE_CASES
    a, floor, same = R.order_floor(case, normalise=gauge_free)
    tol = R.tolerances(a, floor, normalise=gauge_free)
    print("order floor", case, {k: f"{v:.2e}" for k, v in floor.items()}, "-> tolerance", {k: f"{v:.2e}" for k, v in tol.items()})
    assert same, "the two orders disagree on an accept / reject decision: not a parity case, replace the seed"
    assert a["iterations"] == case[5] and np.isfinite(a["chi2_after"]) and a["chi2_after"] < a["chi2_before"]


def test_device_entry_points_are_declared_and_exported():
    from visual_odometry_amd import _lib, map_filters
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("vo_bundle_adjust", "vo_bundle_adjust_batch"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/vo_hip.h"
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert "vo_ba_opts" in header and "VO_BA_MAX_CAMERAS 64" in header and "VO_BA_MAX_FREE" in header
    import ctypes
    assert ctypes.sizeof(_lib.BaOpts) == 16 and _lib.BaOpts.huber_delta.offset == 8
    for name in ("bundle_adjust", "bundle_adjust_batch", "optimize_map"):
        assert callable(getattr(map_filters, name))

"""GPU: the bundle adjustment of one large map (vo_bundle_adjust_large, map_filters.bundle_adjust_large / optimize_map_large)
against the numpy restatement tests/ba_reference.py, by the rule of tests/test_gpu_bundle_adjust.py: status, iterations and trials
equal; R, t, X and chi2 within ba_reference.tolerances (100 x the case's order floor, floored at 1e-12 relative), the floor
recomputed where the test runs; a case whose two CPU summation orders take different decisions is no parity case (asserted).

The factorisation's blocking (docs/kernels/k_bundle_adjust_large.md): panels of P = 8 free cameras (48 columns), trailing-update
tiles of T = 48 rows.  TILE_CASES takes P - 1, P, P + 1 and 2 P + 1 = 17 free cameras; the trailing update gets its second tile row
at 6 F + 1 - 48 > 48, i.e. F = 16, and 17 is one past it.  All of them agreed in two CPU orders at 10 iterations, so none was
shortened and no seed was replaced.  REJECT_CASES are wild starts found by a CPU search (ncam 8, seeds from 200 on, three
perturbation levels; the first seed already rejects trials): their two CPU orders agree through rejected trials, three in a row in
the first one.  Order floors as measured on the CPU (R / t / X / chi2):
  (101, 19, 2, 300, 0.4)  2e-16 / 1.8e-15 / 1.1e-14 / 1.1e-11      (111,  9, 2, 150, 0.5)  3.0e-16 / 2.7e-15 / 1.4e-14 / 0
  (105, 66, 60, 300, 0.1) 4e-16 / 1.8e-14 / 2.8e-14 / 7e-12        (112, 10, 2, 150, 0.5)  1.8e-16 / 1.3e-15 / 1.8e-14 / 2.0e-12
  (103, 40, 4, 500, 0.2)  3e-16 / 5e-15 / 1.9e-14 / 1.8e-11        (113, 11, 2, 150, 0.5)  2.0e-16 / 1.8e-15 / 1.1e-14 / 9.1e-13
  (102, 65, 2, 400, 0.1)  6e-15 / 5.8e-13 / 3.3e-13 / 4e-12        (114, 18, 2, 150, 0.5)  1.5e-16 / 2.7e-15 / 8.9e-15 / 2.3e-12
  (104, 130, 2, 600, 0.06) 4.7e-14 / 1.4e-11 / 3.5e-12 / 7e-12     (115, 19, 2, 150, 0.5)  2.2e-16 / 1.8e-15 / 3.6e-15 / 6.8e-12
  reject (200, 0.3, 1.0, 3.0) 4.9e-11 / 5.9e-10 / 1.6e-09 / 4.5e-07; reject (200, 0.8, 2.0, 6.0) 7.3e-15 / 7.2e-14 / 3.4e-13 / 1.0e-08
Past 128 free cameras the maps are banded flights (ba_reference.banded_map, 24 points per camera, 3 iterations, all trials accepted in
both CPU orders): 250 free (the last panel 12 columns wide) 1.1e-14 / 1.1e-12 / 6.0e-14 / 1.4e-11, 512 free (the capacity) 1.8e-13 /
2.0e-11 / 3.0e-13 / 5.4e-09; the checker takes about 8 s for both orders at 512, the device milliseconds.  One map of 66 000 points
(3 cameras, 198 000 observations) gives the wide reductions 258 partials, past the 256 lanes that add them: 7.4e-16 / 6.7e-15 /
4.1e-15 / 5.4e-09; its chi2 before holds _compare's 1e-12 relative like every other case (the two CPU orders differ by 5e-16)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (R.F0, R.CX, R.CY)
LARGE_CASES = [(101, 19, 2, 300, 0.4), (105, 66, 60, 300, 0.1), (103, 40, 4, 500, 0.2), (102, 65, 2, 400, 0.1), (104, 130, 2, 600, 0.06)]
TILE_CASES = [(111, 9, 2, 150, 0.5), (112, 10, 2, 150, 0.5), (113, 11, 2, 150, 0.5), (114, 18, 2, 150, 0.5), (115, 19, 2, 150, 0.5)]
REJECT_CASES = [(200, 0.3, 1.0, 3.0), (200, 0.8, 2.0, 6.0)]           # (seed, pert_r, pert_t, pert_x) of an 8-camera, 80-point map
BANDED_FREE = [250, 512]                                              # past the 128 free cameras of LARGE_CASES, to VO_BA_LARGE_MAX_FREE
SMALL_CASES = [R.PARITY_CASES[0], R.PARITY_CASES[9], R.PARITY_CASES[11]]


def _case_id(c):
    return "seed%d_%dcam_%dfixed_%dpt" % c[:4]


def _large_map(case):
    seed, ncam, nfixed, npt, vis = case
    return R.make_map(seed, ncam=ncam, npt=npt, nfixed=nfixed, vis=vis)


def _compare(problem, iterations, seed, normalise=False, delta=1.0, label=""):
    """The device against the first of two CPU summation orders, within the tolerance the two orders give."""
    from visual_odometry_amd import map_filters as mf
    ref, floor, same = R.order_floor_of(problem, iterations, seed, normalise, delta)
    assert same, "not a parity case: two CPU summation orders take different accept / reject decisions"
    tol = R.tolerances(ref, floor, normalise)
    g = mf.bundle_adjust_large(*problem, *CAM, iterations=iterations, huber_delta=delta)
    qg, qr = R.quantities(g["poses"], g["points"], g["chi2_after"], normalise), R.quantities(ref["poses"], ref["points"], ref["chi2_after"], normalise)
    diff = {k: float(np.abs(qg[k] - qr[k]).max()) for k in qg}
    print("case", label, "obs", len(problem[3]), "chi2", ref["chi2_before"], "->", ref["chi2_after"], "it/trials", g["iterations"], g["trials"], "accepts", ref["accepts"],
          "| floor", {k: f"{v:.1e}" for k, v in floor.items()}, "| tol", {k: f"{v:.1e}" for k, v in tol.items()}, "| gpu - ref", {k: f"{v:.1e}" for k, v in diff.items()})
    assert g["status"] == 0 and (g["iterations"], g["trials"]) == (ref["iterations"], ref["trials"])
    assert abs(g["chi2_before"] - ref["chi2_before"]) <= 1e-12 * ref["chi2_before"]
    for k in diff:
        assert diff[k] <= tol[k], (k, diff[k], tol[k])
    fx = np.asarray(problem[1]).astype(bool)
    assert np.array_equal(g["poses"][fx], np.asarray(problem[0])[fx])           # fixed cameras: the input bytes
    for T in g["poses"][~fx]:                                                   # free ones: out of a unit quaternion
        assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-12
    return g, ref


@pytest.mark.parametrize("case", LARGE_CASES, ids=_case_id)
def test_parity_beyond_the_small_kernel(ctx, case):
    _compare(R.args(_large_map(case)), 10, case[0], label=case)


@pytest.mark.parametrize("case", TILE_CASES, ids=_case_id)
def test_parity_at_panel_and_tile_boundaries(ctx, case):
    _compare(R.args(_large_map(case)), 10, case[0], label=case)


@pytest.mark.parametrize("free", BANDED_FREE)
def test_parity_to_capacity(ctx, free):
    """Banded flights (ba_reference.banded_map, 24 points per camera, 3 iterations): S has a band of 8 block columns filled in by
    the factorisation.  250 free cameras: 32 panels, the last one 12 columns wide; 512: the capacity, 64 panels, a 64 x 64 tile grid."""
    _compare(R.banded_map(free, seed=300 + free, per_camera=24), 3, 300 + free, label=("banded", free))


def test_parity_past_65536_points(ctx):
    """66 000 points are 258 workgroups of the per-point kernels: the wide reductions' lanes take a second partial (t + 256)."""
    g, _ = _compare(R.args(R.make_map(400, ncam=3, npt=66000, nfixed=2, vis=1.0)), 3, 400, label="258 partials")
    assert len(g["points"]) > 256 * 256


@pytest.mark.parametrize("case", REJECT_CASES, ids=lambda c: "seed%d_r%g" % c[:2])
def test_parity_through_rejected_trials(ctx, case):
    seed, pr, pt, px = case
    m = R.make_map(seed, ncam=8, npt=80, nfixed=2, vis=0.6, pert_r=pr, pert_t=pt, pert_x=px)
    g, ref = _compare(R.args(m), 10, seed, label=case)
    assert 0 in ref["accepts"] and g["trials"] > g["iterations"]


@pytest.mark.parametrize("case", SMALL_CASES, ids=_case_id)
def test_parity_within_the_small_kernel(ctx, case):
    _compare(R.args(R.case_map(case)), case[5], case[0], label=case)


def test_gauge_free_shape_up_to_scale(ctx):
    case = R.GAUGE_FREE_CASES[2]
    _compare(R.args(R.case_map(case)), case[5], case[0], normalise=True, label=case)


def _bytes(r):
    return (r["poses"].tobytes(), r["points"].tobytes(), np.float64(r["chi2_before"]).tobytes(), np.float64(r["chi2_after"]).tobytes(),
            r["iterations"], r["trials"], r["status"])


def test_calls_are_reproducible(ctx):
    from visual_odometry_amd import map_filters as mf, _lib
    m = _large_map(LARGE_CASES[4])
    a = mf.bundle_adjust_large(*R.args(m), *CAM, iterations=10)
    other = _lib.Context(0)
    try:
        mf.bundle_adjust_large(*R.args(_large_map(LARGE_CASES[0])), *CAM, iterations=3, ctx=other)   # another context's run in between
    finally:
        other.close()
    b = mf.bundle_adjust_large(*R.args(m), *CAM, iterations=10)
    assert a["chi2_after"] < a["chi2_before"] and _bytes(a) == _bytes(b)


def test_edges(ctx):
    from visual_odometry_amd import map_filters as mf
    m = R.make_map(71, ncam=4, npt=40, nfixed=2)
    none = (m["poses"], m["fixed"], m["points"], m["oc"][:0], m["op"][:0], m["xy"][:0])
    g, r = mf.bundle_adjust_large(*none, *CAM), R.lm(*none)                     # no observations: ten failed factorisations, nothing moves
    assert (g["iterations"], g["trials"], g["chi2_before"], g["chi2_after"]) == (r["iterations"], r["trials"], 0.0, 0.0) == (1, 10, 0.0, 0.0)
    assert np.array_equal(g["points"], m["points"]) and np.array_equal(g["poses"][m["fixed"]], m["poses"][m["fixed"]])
    assert np.abs(g["poses"] - r["poses"]).max() < 1e-15

    nopts = (m["poses"], m["fixed"], np.zeros((0, 3)), m["oc"][:0], m["op"][:0], m["xy"][:0])
    g, r = mf.bundle_adjust_large(*nopts, *CAM), R.lm(*nopts)                   # cameras alone: S = 0, ten pivots that are not positive
    assert (g["iterations"], g["trials"], g["chi2_after"]) == (r["iterations"], r["trials"], 0.0) == (1, 10, 0.0)
    assert g["points"].shape == (0, 3) and np.abs(g["poses"] - r["poses"]).max() < 1e-15

    s = R.make_map(72, ncam=3, npt=60, nfixed=3)                                # F = 0: structure only
    g, _ = _compare(R.args(s), 8, 72, label="structure only")
    assert np.array_equal(g["poses"], s["poses"])

    one = R.make_map(77, ncam=3, npt=60, nfixed=2, vis=1.0)                     # F = 1
    _compare(R.args(one), 8, 77, label="one free camera")

    keep = m["oc"] != 3                                                         # a free camera without observations: delta = 0
    lone = (m["poses"], m["fixed"], m["points"], m["oc"][keep], m["op"][keep], m["xy"][keep])
    g, _ = _compare(lone, 8, 71, label="free camera without observations")
    assert np.abs(g["poses"][3] - m["poses"][3]).max() < 1e-15

    extra = np.vstack([m["points"], [[1.0, -2.0, 9.0], [-0.0, 3.5, 7.25]]])     # points without observations: their input bytes
    g = mf.bundle_adjust_large(m["poses"], m["fixed"], extra, m["oc"], m["op"], m["xy"], *CAM)
    assert g["points"][-2:].tobytes() == extra[-2:].tobytes()
    assert g["points"][:-2].tobytes() == mf.bundle_adjust_large(*R.args(m), *CAM)["points"].tobytes()

    g, _ = _compare(R.args(m), 8, 71, delta=0.0, label="no robust kernel")      # huber_delta <= 0: plain least squares
    zero = mf.bundle_adjust_large(*R.args(m), *CAM, iterations=0)               # iterations = 0: chi2 alone; free rotations through the quaternion
    assert g["chi2_before"] > zero["chi2_before"] and (zero["iterations"], zero["trials"]) == (0, 0) and zero["chi2_after"] == zero["chi2_before"]
    r0 = R.lm(*R.args(m), iterations=0)
    assert abs(zero["chi2_before"] - r0["chi2_before"]) <= 1e-12 * r0["chi2_before"] and np.abs(zero["poses"] - r0["poses"]).max() < 1e-15
    assert zero["points"].tobytes() == m["points"].tobytes()


def test_outputs_stay_finite(ctx):
    """The inputs of test_gpu_bundle_adjust.py::test_outputs_stay_finite: an edge behind the camera, a point in a camera's plane, a wild start."""
    from visual_odometry_amd import map_filters as mf
    m = R.make_map(43, ncam=4, npt=60, nfixed=2)
    m["points"][5] = [0.1, 0.2, -3.0]
    m["points"][9, 2] = -m["poses"][2, 2, 3] / m["poses"][2, 2, 2]
    wild = R.make_map(41, ncam=4, npt=60, nfixed=2, pert_r=0.5, pert_t=1.0, pert_x=4.0)
    for x in (m, wild):
        g = mf.bundle_adjust_large(*R.args(x), *CAM)
        assert np.all(np.isfinite(g["poses"])) and np.all(np.isfinite(g["points"]))
        assert np.isfinite(g["chi2_before"]) and np.isfinite(g["chi2_after"]) and g["chi2_after"] <= g["chi2_before"]
        assert 1 <= g["iterations"] <= 40 and g["iterations"] <= g["trials"] <= 400


def test_refusals(ctx):
    import ctypes
    from visual_odometry_amd import map_filters as mf, _lib
    n = _lib.VO_BA_LARGE_MAX_FREE + 3                                           # 513 free cameras, one point each
    rng = np.random.default_rng(9)
    poses = np.tile(np.eye(3, 4), (n, 1, 1)); poses[:, 0, 3] = -0.1 * np.arange(n)
    points = np.c_[0.1 * np.arange(n), np.zeros(n), np.full(n, 8.0)] + rng.normal(0, 0.01, (n, 3))
    fixed = np.zeros(n, bool); fixed[:2] = True
    oc = np.arange(n, dtype=np.int32); op = oc.copy()
    xy = np.array([R.project(poses[i], points[i]) for i in range(n)])
    p, f, x, c, q, y = mf._ba_problem(poses, fixed, points, oc, op, xy)
    p0, x0 = p.copy(), x.copy()
    chi = np.zeros(2); it = np.zeros(1, np.int32); tr = np.zeros(1, np.int32)
    opts = _lib.BaOpts(5, 0, 1.0)
    lib, h = ctx.lib, ctx.handle
    call = lambda *a: lib.vo_bundle_adjust_large(h, *a, *CAM, ctypes.addressof(opts), chi.ctypes.data, it.ctypes.data, tr.ctypes.data)  # noqa: E731
    assert call(p.ctypes.data, f.ctypes.data, n, x.ctypes.data, n, c.ctypes.data, q.ctypes.data, y.ctypes.data, n) == _lib.VO_ERR_UNSUPPORTED
    assert p.tobytes() == p0.tobytes() and x.tobytes() == x0.tobytes() and it[0] == 0    # the refused map comes back unchanged
    with pytest.raises(_lib.VoError) as e:
        mf.bundle_adjust_large(poses, fixed, points, oc, op, xy, *CAM)
    assert e.value.code == _lib.VO_ERR_UNSUPPORTED
    fixed[2] = True                                                             # 512 free cameras: the capacity itself is taken
    g = mf.bundle_adjust_large(poses, fixed, points, oc, op, xy, *CAM, iterations=1)
    assert g["status"] == 0 and g["iterations"] == 1 and np.array_equal(g["poses"][:3], poses[:3])

    m = R.make_map(71, ncam=4, npt=40, nfixed=2)                                # an index out of range
    for bad_c, bad_p in ((4, 0), (0, -1)):
        boc, bop = m["oc"].copy(), m["op"].copy()
        boc[7], bop[7] = bad_c, bad_p
        with pytest.raises(_lib.VoError) as e:
            mf.bundle_adjust_large(m["poses"], m["fixed"], m["points"], boc, bop, m["xy"], *CAM)
        assert e.value.code == _lib.VO_ERR_INVALID
    with pytest.raises(_lib.VoError):
        mf.bundle_adjust_large(*R.args(m), *CAM, iterations=1001)
    # NULL arguments
    assert lib.vo_bundle_adjust_large(h, None, None, 0, None, 0, None, None, None, 0, *CAM, None, chi.ctypes.data, it.ctypes.data, tr.ctypes.data) == _lib.VO_ERR_INVALID
    assert lib.vo_bundle_adjust_large(h, None, None, 1, None, 0, None, None, None, 0, *CAM, ctypes.addressof(opts), chi.ctypes.data, it.ctypes.data, tr.ctypes.data) == _lib.VO_ERR_INVALID
    assert lib.vo_bundle_adjust_large(h, None, None, 0, None, 0, None, None, None, 0, *CAM, ctypes.addressof(opts), None, None, None) == _lib.VO_ERR_INVALID
    assert b"bad arguments" in lib.vo_last_error(h)


class Cam:
    def __init__(self, cid, R_, t, fixed): self.camera_id, self.R, self.t, self.fixed = cid, R_, t, fixed


class Pt:
    def __init__(self, pid, p): self.point_id, self.point = pid, p


class Obs:
    def __init__(self, pid, cid, xy): self.point_id, self.camera_id, self.image_coordinates = pid, cid, xy


def test_object_level_optimize_map_large(ctx):
    """Duck-typed records in, attributes written back as optimize_map writes them: what bundle_adjust_large returns."""
    from visual_odometry_amd import map_filters as mf
    m = _large_map(LARGE_CASES[0])
    n = len(m["poses"])
    cam_ids = [1000 - 7 * i for i in range(n)]                                  # ids are neither contiguous nor ascending
    cams = [Cam(cam_ids[i], m["poses"][i, :, :3].copy(), m["poses"][i, :, 3].copy(), bool(m["fixed"][i])) for i in range(n)]
    pts = [Pt(50 + 3 * j, tuple(m["points"][j])) for j in range(len(m["points"]))]
    obs = [Obs(50 + 3 * int(p), cam_ids[int(c)], tuple(xy)) for c, p, xy in zip(m["oc"], m["op"], m["xy"])]
    K = np.array([[R.F0, 0, R.CX], [0, R.F0, R.CY], [0, 0, 1.0]])
    c0, c1 = mf.optimize_map_large(cams, pts, obs, K, iterations=5)
    g = mf.bundle_adjust_large(*R.args(m), *CAM, iterations=5)
    assert (c0, c1) == (g["chi2_before"], g["chi2_after"]) and c1 < c0
    for i, c in enumerate(cams):
        assert isinstance(c.t, np.ndarray) and c.t.shape == (3,) and c.R.shape == (3, 3)
        assert np.array_equal(c.R, g["poses"][i, :, :3]) and np.array_equal(c.t, g["poses"][i, :, 3])
    assert np.array_equal(cams[0].R, m["poses"][0, :, :3]) and np.array_equal(cams[1].t, m["poses"][1, :, 3])
    for j, p in enumerate(pts):
        assert isinstance(p.point, np.ndarray) and p.point.shape == (3,) and np.array_equal(p.point, g["points"][j])


def test_example_global_ba(ctx):
    """examples/global_ba.py at a reduced size: the bundle adjustment lowers the chi2 the pose graph left and brings the cameras
    no further from the truth."""
    spec = importlib.util.spec_from_file_location("global_ba", os.path.join(ROOT, "examples", "global_ba.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    stages, ba = mod.run(frames=40, landmarks=3000, seed=0, iterations=10, out=lines.append)
    print("\n".join(lines))
    assert [s["name"] for s in stages] == ["dead reckoning", "pose graph + map", "bundle adjustment"] and ba["status"] == 0
    assert stages[1]["chi2"] < stages[0]["chi2"] and stages[2]["chi2"] < stages[1]["chi2"]
    assert stages[1]["centre_error"] < stages[0]["centre_error"] and stages[2]["centre_error"] <= stages[1]["centre_error"]
    assert abs(stages[2]["chi2"] - ba["chi2_after"]) <= 1e-9 * ba["chi2_after"]

"""GPU: the device bundle adjustment (vo_bundle_adjust[_batch], map_filters.bundle_adjust / optimize_map) against the numpy
restatement tests/ba_reference.py.

Tolerance rule (tests/ba_reference.py: order_floor, tolerances).  Each parity case runs the numpy LM twice on the CPU, with
the observations as given and in a seeded permutation; the largest difference per quantity (R, t, X, chi2) is that
case's order floor.  The kernel's reduction tree is a third summation order: it has to agree with the first run within
100 x the floor, floored at 1e-12 relative to the quantity's largest magnitude, and take the same number of iterations
and trials.  A case whose two CPU orders take different accept / reject decisions is no parity case; which seeds and
iteration counts that leaves, and why, is stated at R.PARITY_CASES.

Order floors and tolerances as measured on the CPU (pytest -s tests/test_bundle_adjust_reference.py -k order_floor);
tolerances of 1.0e-12 (R), |t|max e-12 and |X|max e-12 are the relative floor of the rule, the others 100 x the order floor:

  case (seed, cams, fixed, points, it)   floor R   floor t   floor X   floor chi2 | tol R    tol t     tol X     tol chi2
  (11,  3,  2,   50,  8)                 6.8e-17   7.0e-16   2.0e-14   2.8e-13    | 1.0e-12  8.0e-13   1.2e-11   3.5e-11
  (12,  3,  2,  400,  8)                 1.7e-17   5.7e-16   3.4e-14   5.7e-13    | 1.0e-12  8.0e-13   1.2e-11   2.9e-10
  (13,  4,  2,  120, 40)                 8.1e-17   6.6e-16   3.3e-14   1.7e-12    | 1.0e-12  1.2e-12   1.2e-11   8.8e-10
  (14,  6,  4,  300, 14)                 6.2e-17   6.7e-16   1.8e-14   1.8e-12    | 1.0e-12  2.0e-12   1.2e-11   3.5e-09
  (15,  6,  5,  300, 40)                 3.5e-17   4.4e-16   1.4e-14   9.6e-12    | 1.0e-12  2.0e-12   1.2e-11   3.2e-09
  (16,  8,  6,  500, 40)                 1.1e-16   3.3e-16   2.1e-14   3.6e-12    | 1.0e-12  2.8e-12   1.2e-11   4.7e-09
  (17, 18, 16,  600, 14)                 4.5e-17   1.9e-16   8.9e-15   1.6e-11    | 1.0e-12  6.8e-12   1.2e-11   1.0e-08
  (18, 18, 16, 3000, 40)                 8.7e-18   4.5e-16   1.8e-14   1.2e-10    | 1.0e-12  6.8e-12   1.2e-11   3.7e-08
  (19, 18, 17,  600, 40)                 1.1e-16   2.9e-16   5.3e-15   1.3e-11    | 1.0e-12  6.8e-12   1.2e-11   1.0e-08
  (20, 14,  2,  300, 40)                 1.1e-16   1.8e-15   1.1e-14   3.6e-12    | 1.0e-12  5.2e-12   1.3e-11   5.6e-09
  (21, 18,  6,  400, 14)                 1.2e-16   1.1e-15   7.1e-15   4.5e-12    | 1.0e-12  6.8e-12   1.2e-11   6.2e-09
  (22, 18,  2,  600, 40)                 1.4e-16   8.9e-16   7.1e-15   1.8e-12    | 1.0e-12  6.8e-12   1.2e-11   1.1e-08
  (23, 18,  2, 1200, 40)                 1.7e-16   1.8e-15   1.6e-14   5.5e-12    | 1.0e-12  6.8e-12   1.2e-11   1.6e-08
  (24, 18,  6,  500, 40)                 1.8e-16   1.8e-15   7.1e-15   7.3e-12    | 1.0e-12  6.8e-12   1.2e-11   9.2e-09
  (25, 18, 16,  800, 40)                 1.5e-16   8.7e-16   9.8e-15   3.6e-11    | 1.0e-12  6.8e-12   1.2e-11   1.4e-08
  gauge-free (t, X divided by |t| of the last camera):
  (51,  2,  1,  200,  8)                 5.7e-16   2.7e-15   7.0e-13   6.8e-13    | 1.0e-12  1.0e-12   7.0e-11   6.8e-11
  (52,  2,  1,  500,  8)                 1.6e-15   4.9e-15   1.8e-12   8.5e-14    | 1.0e-12  1.0e-12   1.8e-10   1.4e-10
  (53,  3,  1,  200,  8)                 9.7e-17   4.7e-16   6.9e-14   1.4e-13    | 1.0e-12  1.0e-12   1.6e-11   1.5e-10
  (54,  3,  1,  500,  8)                 2.9e-16   3.6e-16   1.0e-13   4.6e-13    | 1.0e-12  1.0e-12   1.5e-11   3.7e-10

No seed was replaced.  Seeds 14, 17, 21 and every 3-camera / gauge-free seed tried reach the rounding floor before
iteration 40 and from there on take different accept / reject decisions in two CPU orders; those maps are compared after
14 (3 cameras, gauge-free: 8) iterations, the others after the reference's 40 (R.PARITY_CASES gives the reasoning).  The tests
recompute floor and tolerance at run time; the table is a record."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

CAM = (R.F0, R.CX, R.CY)


def _case_id(c):
    return "seed%d_%dcam_%dfixed_%dpt" % c[:4]


def _compare(problem, iterations, seed, normalise=False, delta=1.0, label=""):
    """The kernel against the first of two CPU summation orders, within the tolerance the two orders give (the rule above)."""
    from visual_odometry_amd import map_filters as mf
    ref, floor, same = R.order_floor_of(problem, iterations, seed, normalise, delta)
    assert same, "not a parity case: two CPU summation orders take different accept / reject decisions"
    tol = R.tolerances(ref, floor, normalise)
    g = mf.bundle_adjust(*problem, *CAM, iterations=iterations, huber_delta=delta)
    qg, qr = R.quantities(g["poses"], g["points"], g["chi2_after"], normalise), R.quantities(ref["poses"], ref["points"], ref["chi2_after"], normalise)
    diff = {k: float(np.abs(qg[k] - qr[k]).max()) for k in qg}
    print("case", label, "obs", len(problem[3]), "chi2", ref["chi2_before"], "->", ref["chi2_after"], "it/trials", g["iterations"], g["trials"],
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


@pytest.mark.parametrize("case", R.PARITY_CASES, ids=_case_id)
def test_parity_with_the_numpy_restatement(ctx, case):
    _compare(R.args(R.case_map(case)), case[5], case[0], label=case)


@pytest.mark.parametrize("case", R.GAUGE_FREE_CASES, ids=_case_id)
def test_initialize_map_shapes_up_to_scale(ctx, case):
    """initialize_map's graph (visual_slam.py:56-87: camera 1 fixed, camera 2 free) and the next frame's (1 fixed, 2 free)"""
    _compare(R.args(R.case_map(case)), case[5], case[0], normalise=True, label=case)


class Cam:
    def __init__(self, cid, R_, t, fixed): self.camera_id, self.R, self.t, self.fixed = cid, R_, t, fixed
    def pose(self):
        T = np.eye(4); T[:3, :3] = self.R; T[:3, 3] = np.asarray(self.t).ravel(); return T


class Pt:
    def __init__(self, pid, p): self.point_id, self.point = pid, p


class Obs:
    def __init__(self, pid, cid, xy): self.point_id, self.camera_id, self.image_coordinates = pid, cid, xy


def _huber_total(sqerr):
    s = np.sqrt(sqerr)
    return float(np.where(s <= 1.0, sqerr, 2 * s - 1).sum())


def test_end_to_end_on_front_end_output(ctx, seq_small, capsys):
    """ImagePair on real frames -> the map initialize_map builds (visual_slam.py:43-87, re-typed) -> optimize_map ->
    the reprojection error of the existing GPU filter."""
    from visual_odometry_amd import FrameGenerator, ImagePair, ORB_create, BFMatcher, map_filters as mf
    from visual_odometry_amd.matcher import NORM_HAMMING
    frames, K = seq_small["frames"], seq_small["K"]
    assert K[0, 0] == K[1, 1]                                                   # one focal length is all g2o's CameraParameters takes
    gen = FrameGenerator(ORB_create(nfeatures=500))
    f1, f2 = gen.make_frame(frames[0]), gen.make_frame(frames[1])
    ip = ImagePair(f1, f2, BFMatcher(NORM_HAMMING, crossCheck=True), K)
    ip.match_features()
    ess = ip.determine_essential_matrix(ip.filtered_matches)
    ip.estimate_camera_movement(ess)
    ip.reconstruct_3d_points(ess)
    capsys.readouterr()
    cams = [Cam(0, np.eye(3), np.zeros(3), True), Cam(1, ip.R.copy(), ip.t.T[0].copy(), False)]
    pts, obs = [], []
    for i, mt in enumerate(ip.matches_with_3d_information):
        pts.append(Pt(2 + i, mt.point))
        obs += [Obs(2 + i, 0, mt.keypoint1), Obs(2 + i, 1, mt.keypoint2)]
    assert len(pts) >= 30
    R1, t1 = cams[1].R.copy(), cams[1].t.copy()
    before = mf.calculate_reprojection_error(cams, pts, obs, K)
    c0, c1 = mf.optimize_map(cams, pts, obs, K)
    after = mf.calculate_reprojection_error(cams, pts, obs, K)
    sq, _ = mf.reprojection_sqerr(*mf._arrays(cams, pts, obs), K, np.inf)
    print(f"{len(pts)} points: reprojection error {before:.3f} -> {after:.3f}; robust chi2 {c0:.3f} -> {c1:.6f}; edges beyond the Huber radius {(sq > 1).sum()}")
    assert after < before and c1 < c0
    assert abs(c1 - _huber_total(sq)) <= 1e-9 * max(c1, 1.0)                    # activeRobustChi2 of the state written back
    if (sq <= 1).all():
        assert abs(c1 - after) <= 1e-9 * max(c1, 1.0)
    assert np.array_equal(cams[0].R, np.eye(3)) and np.array_equal(cams[0].t, np.zeros(3))   # the fixed camera: bit for bit
    assert not np.array_equal(cams[1].R, R1) and cams[1].t.shape == (3,) and not np.array_equal(cams[1].t, t1)
    assert np.abs(cams[1].R @ cams[1].R.T - np.eye(3)).max() < 1e-12


def _mixed_batch():
    shapes = [(61, 6, 4, 120, 0.8), (62, 18, 16, 300, 0.4), (63, 3, 2, 50, 1.0), (64, 18, 2, 200, 0.4), (65, 8, 6, 250, 0.6),
              (66, 2, 1, 80, 1.0), (67, 14, 2, 150, 0.5)]
    return [R.make_map(s, ncam=c, npt=p, nfixed=f, vis=v, min_views=3 if f >= 2 else 2) for s, c, f, p, v in shapes]


def _bytes(r):
    return (r["poses"].tobytes(), r["points"].tobytes(), np.float64(r["chi2_before"]).tobytes(), np.float64(r["chi2_after"]).tobytes(),
            r["iterations"], r["trials"], r["status"])


def test_batch_equals_single_and_calls_are_reproducible(ctx):
    from visual_odometry_amd import map_filters as mf, _lib
    maps = _mixed_batch()
    batch = mf.bundle_adjust_batch([R.args(m) for m in maps], *CAM)
    assert len(batch) == 7 and all(r["status"] == 0 and r["chi2_after"] < r["chi2_before"] for r in batch)
    for m, r in zip(maps, batch):
        assert _bytes(mf.bundle_adjust(*R.args(m), *CAM)) == _bytes(r)          # problem b alone returns the bytes it returns in the batch
    other = _lib.Context(0)
    try:
        mf.bundle_adjust(*R.args(maps[3]), *CAM, iterations=5, ctx=other)        # another context's run in between
    finally:
        other.close()
    again = mf.bundle_adjust_batch([R.args(m) for m in maps], *CAM)
    assert [_bytes(r) for r in again] == [_bytes(r) for r in batch]
    rev = mf.bundle_adjust_batch([R.args(m) for m in maps[::-1]], *CAM)          # nor does a problem's place in the batch matter
    assert [_bytes(r) for r in rev[::-1]] == [_bytes(r) for r in batch]


def test_edges(ctx):
    from visual_odometry_amd import map_filters as mf, _lib
    assert mf.bundle_adjust_batch([], *CAM) == []                               # B = 0
    m = R.make_map(71, ncam=4, npt=40, nfixed=2)
    none = (m["poses"], m["fixed"], m["points"], m["oc"][:0], m["op"][:0], m["xy"][:0])
    g, r = mf.bundle_adjust(*none, *CAM), R.lm(*none)                           # no observations: ten failed factorisations, nothing moves
    assert (g["iterations"], g["trials"], g["chi2_before"], g["chi2_after"]) == (r["iterations"], r["trials"], 0.0, 0.0) == (1, 10, 0.0, 0.0)
    assert np.array_equal(g["points"], m["points"]) and np.array_equal(g["poses"][m["fixed"]], m["poses"][m["fixed"]])
    assert np.abs(g["poses"] - r["poses"]).max() < 1e-15

    s = R.make_map(72, ncam=3, npt=60, nfixed=3)                                # no free camera: structure only
    g, _ = _compare(R.args(s), 8, 72, label="structure only")
    assert np.array_equal(g["poses"], s["poses"])

    keep = m["oc"] != 3                                                         # a free camera without observations: delta = 0
    lone = (m["poses"], m["fixed"], m["points"], m["oc"][keep], m["op"][keep], m["xy"][keep])
    g, _ = _compare(lone, 8, 71, label="free camera without observations")
    assert np.abs(g["poses"][3] - m["poses"][3]).max() < 1e-15

    extra = np.vstack([m["points"], [[1.0, -2.0, 9.0], [-0.0, 3.5, 7.25]]])     # points without observations: their input bytes
    g = mf.bundle_adjust(m["poses"], m["fixed"], extra, m["oc"], m["op"], m["xy"], *CAM)
    assert g["points"][-2:].tobytes() == extra[-2:].tobytes()
    assert g["points"][:-2].tobytes() == mf.bundle_adjust(*R.args(m), *CAM)["points"].tobytes()

    g, _ = _compare(R.args(m), 8, 71, delta=0.0, label="no robust kernel")      # huber_delta <= 0: plain least squares
    assert g["chi2_before"] > mf.bundle_adjust(*R.args(m), *CAM, iterations=0)["chi2_before"]

    # capacity: 17 free cameras, 65 cameras -> that problem unsupported and unchanged, its neighbours solved
    big_free = R.make_map(73, ncam=19, npt=60, nfixed=2, vis=0.4)
    big = R.make_map(74, ncam=65, npt=80, nfixed=60, vis=0.1)
    ok1, ok2 = R.make_map(75, ncam=18, npt=60, nfixed=2, vis=0.4), R.make_map(76, ncam=64, npt=80, nfixed=60, vis=0.1)
    out = mf.bundle_adjust_batch([R.args(x) for x in (ok1, big_free, ok2, big)], *CAM, iterations=5)
    assert [o["status"] for o in out] == [0, _lib.VO_ERR_UNSUPPORTED, 0, _lib.VO_ERR_UNSUPPORTED]
    for o, x in ((out[1], big_free), (out[3], big)):
        assert o["poses"].tobytes() == x["poses"].tobytes() and o["points"].tobytes() == x["points"].tobytes() and o["iterations"] == 0
    for o, x in ((out[0], ok1), (out[2], ok2)):
        assert o["chi2_after"] < o["chi2_before"] and _bytes(o) == _bytes(mf.bundle_adjust(*R.args(x), *CAM, iterations=5))
    with pytest.raises(_lib.VoError) as e:
        mf.bundle_adjust(*R.args(big), *CAM)
    assert e.value.code == _lib.VO_ERR_UNSUPPORTED

    # an index out of range: reported for that problem, which comes back unchanged
    bad_oc = m["oc"].copy(); bad_oc[7] = 4
    bad_op = m["op"].copy(); bad_op[3] = -1
    out = mf.bundle_adjust_batch([(m["poses"], m["fixed"], m["points"], bad_oc, m["op"], m["xy"]), R.args(m),
                                  (m["poses"], m["fixed"], m["points"], m["oc"], bad_op, m["xy"])], *CAM)
    assert [o["status"] for o in out] == [_lib.VO_ERR_INVALID, 0, _lib.VO_ERR_INVALID] and out[0]["points"].tobytes() == m["points"].tobytes()
    with pytest.raises(_lib.VoError) as e:
        mf.bundle_adjust(m["poses"], m["fixed"], m["points"], bad_oc, m["op"], m["xy"], *CAM)
    assert e.value.code == _lib.VO_ERR_INVALID
    with pytest.raises(_lib.VoError):
        mf.bundle_adjust(*R.args(m), *CAM, iterations=1001)

    # NULL arguments
    lib, h = ctx.lib, ctx.handle
    opts = _lib.BaOpts(40, 0, 1.0)
    import ctypes
    one = np.zeros(2, np.int32); one[1] = 1
    chi = np.zeros(2); it = np.zeros(1, np.int32)
    assert lib.vo_bundle_adjust_batch(h, 1, None, None, None, None, None, None, None, None, None, *CAM, ctypes.addressof(opts), None, None, None, None) == _lib.VO_ERR_INVALID
    assert lib.vo_bundle_adjust_batch(h, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, None, None, None, None, None, None, *CAM,
                                      ctypes.addressof(opts), chi.ctypes.data, it.ctypes.data, it.ctypes.data, it.ctypes.data) == _lib.VO_ERR_INVALID
    assert lib.vo_bundle_adjust(h, None, None, 0, None, 0, None, None, None, 0, *CAM, None, chi.ctypes.data, it.ctypes.data, it.ctypes.data) == _lib.VO_ERR_INVALID
    assert lib.vo_bundle_adjust(h, None, None, 1, None, 0, None, None, None, 0, *CAM, ctypes.addressof(opts), None, None, None) == _lib.VO_ERR_INVALID
    assert b"bad arguments" in lib.vo_last_error(h)


def test_outputs_stay_finite(ctx):
    """Finite inputs never produce NaN: an edge behind the camera, a point in a camera's plane, a wild start."""
    from visual_odometry_amd import map_filters as mf
    m = R.make_map(43, ncam=4, npt=60, nfixed=2)
    m["points"][5] = [0.1, 0.2, -3.0]
    m["points"][9, 2] = -m["poses"][2, 2, 3] / m["poses"][2, 2, 2]
    wild = R.make_map(41, ncam=4, npt=60, nfixed=2, pert_r=0.5, pert_t=1.0, pert_x=4.0)
    for x in (m, wild):
        g = mf.bundle_adjust(*R.args(x), *CAM)
        assert np.all(np.isfinite(g["poses"])) and np.all(np.isfinite(g["points"]))
        assert np.isfinite(g["chi2_before"]) and np.isfinite(g["chi2_after"]) and g["chi2_after"] <= g["chi2_before"]
        assert 1 <= g["iterations"] <= 40 and g["iterations"] <= g["trials"] <= 400


def test_object_level_optimize_map(ctx):
    """Duck-typed TrackedCamera / TrackedPoint / Observation in, attributes written back as map.py:175-186 writes them."""
    from visual_odometry_amd import map_filters as mf
    m = R.make_map(81, ncam=5, npt=90, nfixed=2)
    cam_ids = [40, 7, 300, 12, 99]                                              # ids are neither contiguous nor ordered
    cams = [Cam(cam_ids[i], m["poses"][i, :, :3].copy(), m["poses"][i, :, 3].copy(), bool(m["fixed"][i])) for i in range(5)]
    pts = [Pt(1000 + 13 * j, tuple(m["points"][j])) for j in range(90)]
    obs = [Obs(1000 + 13 * int(p), cam_ids[int(c)], tuple(xy)) for c, p, xy in zip(m["oc"], m["op"], m["xy"])]
    K = np.array([[R.F0, 0, R.CX], [0, R.F0, R.CY], [0, 0, 1.0]])
    c0, c1 = mf.optimize_map(cams, pts, obs, K)
    g = mf.bundle_adjust(*R.args(m), *CAM)
    assert (c0, c1) == (g["chi2_before"], g["chi2_after"]) and c1 < c0
    for i, c in enumerate(cams):
        assert isinstance(c.t, np.ndarray) and c.t.shape == (3,) and c.R.shape == (3, 3)
        assert np.array_equal(c.R, g["poses"][i, :, :3]) and np.array_equal(c.t, g["poses"][i, :, 3])
    assert np.array_equal(cams[0].R, m["poses"][0, :, :3]) and np.array_equal(cams[1].t, m["poses"][1, :, 3])
    for j, p in enumerate(pts):
        assert isinstance(p.point, np.ndarray) and p.point.shape == (3,) and np.array_equal(p.point, g["points"][j])
    assert pts[0].point is not pts[1].point and pts[0].point.base is None          # a fresh array per point
    # ... and the map can go straight back in.  Its chi2 is the one just reported up to the rule's relative floor, not to the
    # bit: a free camera's R is turned into a unit quaternion and back on entry (as SE3Quat(R, t) does), which moves it by an ulp
    again = mf.optimize_map(cams, pts, obs, K, iterations=3)
    assert abs(again[0] - c1) <= 1e-12 * c1 and again[1] <= again[0]

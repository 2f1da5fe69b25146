"""GPU: cv2.undistortPoints per call (vo_undistort_points, k_undistort_points) and on the resident keypoints (vo_frames_undistort,
k_undistort_frames) against the numpy checker tests/undistort_reference.py — byte for byte, which is the contract: the kernel and
the checker make the same float64 operations in the same order.

  per call      N in {0, 1, 63, 64, 65, 257} x f32 / f64 x 4, 5, 8 coefficients x R and P absent / present; the input holds the
                principal point, the point chosen to take the icdist < 0 fallback (tests/test_undistort_reference.py shows on
                the CPU that it does) and a NaN row.  A NaN's payload is not defined by IEEE arithmetic, so the NaN row is
                compared as NaN and every other row by its bytes.
  refusals      coefficient counts, fx = 0, null pointers, a bad point type — each followed by a good call on the same context.
  resident      rows staged through set_orb_rows / set_sift_rows (counts 0, 1, 255, 256, 257: either side of the kernel's 256-lane
                block), frames detected from tests/golden/pair_320x240.npz (also behind detect(wait=False)); only kp_xy of the
                named slots changes; the once-per-detection mark.
  downstream    three frames of tests/undistort_cases.py: a front end given the distorted keypoints and the call equals, in
                run_pairs, slam_chain and the map, a front end given the checker's corrected keypoints.
  it helps      the same scene through an ideal pinhole, distorted, and distorted with the call.  On the CPU (oracle,
                tests/test_undistort_cases_reference.py): 60 / 50 / 60 inliers; the corrected coordinates differ from the ideal
                ones by at most delta = 2.57e-3 px (round-trip residual 2.38e-3 px at five times the reference's coefficients
                plus three float32 roundings of 2^-14 px); through the conditioning of the pair's five-point sample (sum of the
                |d[R|t] / d coordinate|, one-sided differences with the oracle) that allows [R|t] to move by 4.8e-4 per entry;
                the oracle's own corrected-against-ideal difference is 3.0e-6.

Each test takes well under a second on an MI355X."""
import numpy as np
import pytest

import undistort_cases as UC
import undistort_reference as U
from test_undistort_reference import FALLBACK_DISTS, FALLBACK_POINT, P34, R_Y

pytestmark = pytest.mark.gpu

K = UC.K
SIZES = (0, 1, 63, 64, 65, 257)
COUNTS = (0, 1, 255, 256, 257)
NAN_ROW = 2


def _points():
    """257 points: the principal point, the fallback point, a NaN row, then points within 250 px of the axis (with k1 = -0.5 only
    those stay inside the model: the rest of the frame would fall back too)."""
    rng = np.random.default_rng(20261022)
    p = np.array([K[0, 2], K[1, 2]]) + rng.uniform(-250, 250, (257, 2))
    p[0] = [K[0, 2], K[1, 2]]
    p[1] = FALLBACK_POINT[0]
    p[NAN_ROW] = [np.nan, 100.0]
    return p


POINTS = _points()


def _same(got, want, nan_rows=()):
    assert got.dtype == want.dtype and got.shape == want.shape
    keep = np.ones(len(want), bool)
    keep[list(nan_rows)] = False
    assert not np.isnan(want[keep]).any()
    assert got[keep].tobytes() == want[keep].tobytes()
    for r in nan_rows:
        assert np.array_equal(np.isnan(got[r]), np.isnan(want[r])) and np.isnan(want[r]).any()


@pytest.fixture(scope="module")
def lib_ctx():
    from visual_odometry_amd import _lib
    ctx = _lib.Context(0)
    yield _lib, ctx
    ctx.close()


def _call(ctx, pts, Kc, d, R=None, P=None, point_type=None, n=None, out=None, pts_ptr=True, out_ptr=True):
    pts = np.ascontiguousarray(pts)
    out = np.full((max(len(pts), 1), 2), 7, pts.dtype) if out is None else out
    Kc = None if Kc is None else np.ascontiguousarray(Kc, np.float64)
    d = None if d is None else np.ascontiguousarray(d, np.float64)
    R = None if R is None else np.ascontiguousarray(R, np.float64)
    P = None if P is None else np.ascontiguousarray(P, np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = ctx.lib.vo_undistort_points(ctx.handle, ptr(pts) if pts_ptr else None, len(pts) if n is None else n,
                                     (0 if pts.dtype == np.float64 else 1) if point_type is None else point_type, ptr(Kc), ptr(d),
                                     0 if d is None else len(d), ptr(R), ptr(P), ptr(out) if out_ptr else None)
    return rc, out


# ------------------------------------------------------------------ per call
@pytest.mark.parametrize("with_P", [False, True], ids=["noP", "P"])
@pytest.mark.parametrize("with_R", [False, True], ids=["noR", "R"])
@pytest.mark.parametrize("nd", [4, 5, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_per_call_equals_the_checker_byte_for_byte(lib_ctx, dtype, nd, with_R, with_P):
    _lib, ctx = lib_ctx
    d = FALLBACK_DISTS[nd]
    R = R_Y if with_R else None
    P = P34[:, :3].copy() if with_P else None
    pts = POINTS.astype(dtype)
    want_all, fb = U.undistort_points(pts, K, d, R, P, return_fallback=True)
    assert fb[1] and not fb[0] and not fb[3:].any()                       # only the chosen point takes the fallback
    for n in SIZES:
        rc, out = _call(ctx, pts[:n], K, d, R, P)
        assert rc == _lib.VO_OK, ctx.last_error()
        if n == 0:
            assert (out == 7).all()                                       # N = 0 touches nothing
            continue
        _same(out[:n], want_all[:n], [NAN_ROW] if n > NAN_ROW else [])
    # the reference's own coefficients, P = K: the form the resident call uses
    rc, out = _call(ctx, pts, K, U.REFERENCE_DIST, None, K)
    assert rc == _lib.VO_OK
    _same(out, U.undistort_points(pts, K, U.REFERENCE_DIST, None, K), [NAN_ROW])
    assert out[0].tolist() == pts[0].tolist()                             # the principal point maps to itself


def test_zero_coefficients_give_plain_normalisation(lib_ctx):
    _lib, ctx = lib_ctx
    pts = np.delete(POINTS, NAN_ROW, axis=0)
    x, y = U.normalise(pts[:, 0].copy(), pts[:, 1].copy(), K)
    for n in (4, 5, 8):
        rc, out = _call(ctx, pts, K, np.zeros(n))
        assert rc == _lib.VO_OK and out.tobytes() == np.stack([x, y], 1).tobytes()


def test_refusals_leave_the_context_usable(lib_ctx):
    _lib, ctx = lib_ctx
    pts = np.delete(POINTS, NAN_ROW, axis=0)[:65]
    d5 = U.REFERENCE_DIST
    want = U.undistort_points(pts, K, d5, None, K)

    def good():
        rc, out = _call(ctx, pts, K, d5, None, K)
        assert rc == _lib.VO_OK and out.tobytes() == want.tobytes()

    good()
    for n in (12, 14):
        assert _call(ctx, pts, K, np.zeros(n))[0] == _lib.VO_ERR_UNSUPPORTED
        good()
    for n in (3, 6, 0, 1, 7, 9, 13):
        assert _call(ctx, pts, K, np.zeros(n))[0] == _lib.VO_ERR_INVALID, n
        good()
    K0 = K.copy(); K0[0, 0] = 0.0
    K1 = K.copy(); K1[1, 1] = 0.0
    refused = [_call(ctx, pts, K0, d5)[0], _call(ctx, pts, K1, d5)[0], _call(ctx, pts, None, d5)[0], _call(ctx, pts, K, None)[0],
               _call(ctx, pts, K, d5, pts_ptr=False)[0], _call(ctx, pts, K, d5, out_ptr=False)[0], _call(ctx, pts, K, d5, n=-1)[0],
               _call(ctx, pts, K, d5, point_type=2)[0]]
    assert refused == [_lib.VO_ERR_INVALID] * len(refused)
    assert ctx.last_error()
    good()
    assert ctx.lib.vo_undistort_points(None, None, 0, 0, None, None, 0, None, None, None) == _lib.VO_ERR_INVALID
    assert ctx.lib.vo_frames_undistort(None, 0, 0, None, None, 0) == _lib.VO_ERR_INVALID
    # the resident call before a batch configuration
    Kc = np.ascontiguousarray(K)
    assert ctx.lib.vo_frames_undistort(ctx.handle, 0, 1, Kc.ctypes.data, d5.ctypes.data, 5) == _lib.VO_ERR_NOT_CONFIGURED
    good()


@pytest.mark.parametrize("shape", ["N2", "N12", "1N2"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_python_entries_return_cv2s_shape_and_the_per_call_bytes(lib_ctx, dtype, shape):
    from visual_odometry_amd import cv2_surface, geometry
    _lib, ctx = lib_ctx
    pts = np.delete(POINTS, NAN_ROW, axis=0)[:65].astype(dtype)
    src = {"N2": pts, "N12": pts.reshape(-1, 1, 2), "1N2": pts.reshape(1, -1, 2)}[shape]
    d = FALLBACK_DISTS[8]
    P4 = P34
    rc, raw = _call(ctx, pts, K, d, R_Y, P4[:, :3].copy())
    assert rc == _lib.VO_OK
    for fn in (lambda *a: geometry.undistortPoints(*a, ctx=ctx), cv2_surface.undistortPoints):
        got = fn(src, K, d, R_Y, P4)                                      # a 3 x 4 P: its left 3 x 3
        assert got.shape == (65, 1, 2) and got.dtype == dtype and got.tobytes() == raw.tobytes()
    none = geometry.undistortPoints(src, K, None, ctx=ctx)
    assert none.tobytes() == geometry.undistortPoints(src, K, np.zeros((1, 5)), ctx=ctx).tobytes() == geometry.undistortPoints(src, K, [], ctx=ctx).tobytes()
    assert none.tobytes() == U.undistort_points(pts, K, None).tobytes()
    assert geometry.undistortPoints(np.zeros((0, 2), dtype), K, d, ctx=ctx).shape == (0, 1, 2)
    for n in (12, 14):
        with pytest.raises(NotImplementedError):
            geometry.undistortPoints(src, K, np.zeros(n), ctx=ctx)
    with pytest.raises(_lib.VoError):
        geometry.undistortPoints(src, K, np.zeros(6), ctx=ctx)
    with pytest.raises(NotImplementedError):                               # solvePnPRansac keeps refusing a lens
        geometry.solvePnPRansac(np.zeros((6, 3)), np.zeros((6, 2)), K, U.REFERENCE_DIST, ctx=ctx)


# ------------------------------------------------------------------ resident, staged rows
FEATURE_KEYS = ("xy", "size", "angle", "response", "octave", "desc", "truncated")


def _features_equal(a, b, but=()):
    for k in FEATURE_KEYS:
        if k in but:
            continue
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def _front_end(detector, frames=3, pairs=1):
    from visual_odometry_amd.frontend import FrontEnd
    if detector == "orb":
        return FrontEnd(64, 64, max_frames=frames, max_pairs=pairs, nfeatures=8, nlevels=1)          # kp_cap 264
    return FrontEnd(32, 32, max_frames=frames, max_pairs=pairs, detector="sift", kp_cap=512)


def _rows(rng, detector, n):
    # SIFT rows stay below the integer matcher's norm bound (|row|^2 <= 2^20), or the slot is flagged and its download refused
    return rng.integers(0, 256, (n, 32), dtype=np.uint8) if detector == "orb" else rng.integers(0, 64, (n, 128), dtype=np.uint8)


@pytest.mark.parametrize("detector", ["orb", "sift"])
def test_resident_staged_rows(detector):
    from visual_odometry_amd import _lib
    fe = _front_end(detector)
    try:
        assert fe.kp_cap >= 257
        put = fe.set_orb_rows if detector == "orb" else fe.set_sift_rows
        rng = np.random.default_rng(5)
        side = {s: (_rows(rng, detector, 40), rng.uniform([0, 0], [UC.W, UC.H], (40, 2)).astype(np.float32)) for s in (0, 2)}
        for s, (rows, xy) in side.items():
            put(s, rows, xy)
        for i, n in enumerate(COUNTS):
            d = UC.DIST if i % 2 == 0 else np.r_[UC.DIST, 0.02, -0.01, 0.005]
            rows = _rows(rng, detector, n)
            xy = rng.uniform([0, 0], [UC.W, UC.H], (n, 2)).astype(np.float32)
            put(1, rows, xy)
            before = [fe.features(s) for s in range(3)]
            assert before[1]["xy"].tobytes() == xy.tobytes() and len(before[1]["xy"]) == n
            fe.undistort(1, 1, K, d)
            after = [fe.features(s) for s in range(3)]
            want = U.undistort_pixels(xy, K, d)
            assert after[1]["xy"].dtype == np.float32 and after[1]["xy"].tobytes() == want.tobytes(), n
            if n:
                assert np.abs(want - xy).max() > 0.1                      # the lens moved them (one point near the axis: 0.6 px): the call did something
            _features_equal(before[1], after[1], but=("xy",))
            _features_equal(before[0], after[0]); _features_equal(before[2], after[2])
            # once per detection: a second call on the slot, alone or inside a range, is refused and changes nothing
            for first, count in ((1, 1), (0, 3), (1, 2)):
                with pytest.raises(_lib.VoError) as e:
                    fe.undistort(first, count, K, d)
                assert e.value.code == _lib.VO_ERR_INVALID
            again = [fe.features(s) for s in range(3)]
            for s in range(3):
                _features_equal(after[s], again[s])
        # restaging the slot allows the call again; the neighbours take it once, in one range
        put(1, side[0][0], side[0][1])
        fe.undistort(0, 3, K, UC.DIST)
        for s in range(3):
            assert fe.features(s)["xy"].tobytes() == U.undistort_pixels(side[0 if s == 1 else s][1], K, UC.DIST).tobytes()
        # refusals of the resident form
        for first, count in ((-1, 1), (2, 2), (3, 1), (0, -1)):
            with pytest.raises(_lib.VoError) as e:
                fe.undistort(first, count, K, UC.DIST)
            assert e.value.code == _lib.VO_ERR_INVALID
        put(0, side[0][0], side[0][1])
        for bad, exc in ((np.zeros(12), NotImplementedError), (np.zeros(3), _lib.VoError)):
            with pytest.raises(exc):
                fe.undistort(0, 1, K, bad)
        K0 = K.copy(); K0[1, 1] = 0
        with pytest.raises(_lib.VoError):
            fe.undistort(0, 1, K0, UC.DIST)
        fe.undistort(0, 0, K, UC.DIST)                                    # an empty range marks nothing
        fe.undistort(0, 1, K, UC.DIST)                                    # ... and none of the refusals marked the slot
        assert fe.features(0)["xy"].tobytes() == U.undistort_pixels(side[0][1], K, UC.DIST).tobytes()
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ resident, detected frames
def test_resident_detected_frames():
    import os
    from visual_odometry_amd import _lib
    from visual_odometry_amd.frontend import FrontEnd
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_320x240.npz"))
    frames, Kg = g["frames"], g["K"]
    d = U.REFERENCE_DIST * 10                                             # a small frame sees little of the lens: make it count
    fe = FrontEnd(240, 320, max_frames=2, max_pairs=1, nfeatures=int(g["nfeatures"]), nlevels=int(g["nlevels"]))
    try:
        fe.upload(frames)
        fe.detect(0, 2)
        before = [fe.features(s) for s in range(2)]
        assert len(before[0]["xy"]) > 100 and len(before[1]["xy"]) > 100
        fe.undistort(0, 2, Kg, d)
        for s in range(2):
            after = fe.features(s)
            want = U.undistort_pixels(before[s]["xy"], Kg, d)
            assert after["xy"].tobytes() == want.tobytes() and np.abs(want - before[s]["xy"]).max() > 0.5
            _features_equal(before[s], after, but=("xy",))
        with pytest.raises(_lib.VoError):
            fe.undistort(1, 1, Kg, d)
        # detecting again gives the slot new keypoints: the call is allowed again, here enqueued behind an asynchronous detection
        fe.detect(0, 2, wait=False)
        fe.undistort(0, 2, Kg, d)
        for s in range(2):
            after = fe.features(s)
            assert after["xy"].tobytes() == U.undistort_pixels(before[s]["xy"], Kg, d).tobytes()
            _features_equal(before[s], after, but=("xy",))
        # an upload alone clears the mark of the slot it writes, not the other's
        fe.upload(frames[1:], first_slot=1)
        with pytest.raises(_lib.VoError):
            fe.undistort(0, 2, Kg, d)
        fe.detect(1, 1)
        fe.undistort(1, 1, Kg, d)
        assert fe.features(1)["xy"].tobytes() == U.undistort_pixels(before[1]["xy"], Kg, d).tobytes()
    finally:
        fe.ctx.close()


# ------------------------------------------------------------------ downstream sees only kp_xy
def _staged(xy_of, undistort):
    fe = _front_end("orb", frames=UC.N_FRAMES, pairs=len(UC.PAIRS))
    fe.ctx.set_poly_solver("opencv300")                                   # the oracle's root finder: the CPU file pinned the scene with it
    for k in range(UC.N_FRAMES):
        fe.set_orb_rows(k, UC.ROWS, xy_of(k))
    if undistort:
        fe.undistort(0, UC.N_FRAMES, K, UC.DIST)
    return fe


def _run(fe, pairs):
    res, X = fe.run_pairs(pairs, K, want_points=True)
    res = res.copy()
    X = [X[p][:, :int(res["n_inl"][p])].copy() for p in range(len(pairs))]
    masks = [fe.pair_matches(p) for p in range(len(pairs))]
    return res, X, masks


def test_downstream_sees_only_the_rewritten_positions(oracle):
    from test_gpu_chain import reference_chain
    # on the CPU: every pair of B is solved and pair 1 localises — the equality below is about something
    ref = reference_chain(oracle, [dict(xy=UC.corrected(k), desc=UC.ROWS) for k in range(UC.N_FRAMES)], UC.PAIRS, K)
    assert ref["status"] == [0, 0] and ref["E_inl"] == [UC.N, UC.N] and ref["n_corr"][1] == UC.N and ref["n_inl"][1] == UC.N
    A = _staged(UC.distorted, True)
    B = _staged(UC.corrected, False)
    try:
        for k in range(UC.N_FRAMES):
            assert A.features(k)["xy"].tobytes() == B.features(k)["xy"].tobytes()
        ra, Xa, ma = _run(A, UC.PAIRS)
        rb, Xb, mb = _run(B, UC.PAIRS)
        assert rb["status"].tolist() == [0, 0] and rb["n_inl"].tolist() == [UC.N, UC.N]
        assert ra.tobytes() == rb.tobytes()
        for p in range(len(UC.PAIRS)):
            assert Xa[p].tobytes() == Xb[p].tobytes() and Xa[p].shape == (4, UC.N)
            assert np.array_equal(ma[p][0], np.arange(UC.N)) and np.array_equal(ma[p][1], np.arange(UC.N))   # the identity permutation
            for a, b in zip(ma[p], mb[p]):
                assert a.tobytes() == b.tobytes()
        oa, ob = A.slam_chain(len(UC.PAIRS), K), B.slam_chain(len(UC.PAIRS), K)
        assert ob["status"].tolist() == [0, 0] and ob["n_inl"][1] > 0 and ob["n_pts"][-1] > 0 and ob["n_cam"][-1] == 3
        assert sorted(oa) == sorted(ob)
        for k in oa:
            assert oa[k].tobytes() == ob[k].tobytes(), k
        mapa, mapb = A.slam_map(0), B.slam_map(0)
        for k in mapa:
            assert mapa[k].tobytes() == mapb[k].tobytes() and len(mapa[k]) > 0, k
    finally:
        A.ctx.close(); B.ctx.close()


# ------------------------------------------------------------------ it helps
def test_the_call_restores_the_pinhole_result(oracle):
    margin, delta = UC.pose_margin(oracle)
    print(f"delta {delta:.3e} px, margin {margin:.3e}")
    assert 1e-5 < margin < 1e-3
    pair = [UC.PAIRS[0]]
    fes = [_staged(UC.ideal, False), _staged(UC.distorted, False), _staged(UC.distorted, True)]
    try:
        (ry, _, my), (ru, _, mu), (rc, _, mc) = (_run(fe, pair) for fe in fes)
        print("inliers: pinhole", int(ry["n_inl"][0]), "distorted", int(ru["n_inl"][0]), "with the call", int(rc["n_inl"][0]))
        assert ry["status"][0] == 0 and rc["status"][0] == 0 and ry["n_inl"][0] == UC.N
        assert mc[0][3].tobytes() == my[0][3].tobytes() and rc["n_inl"][0] == ry["n_inl"][0]        # the inlier mask of the yardstick
        Rt = lambda r: np.hstack([r["R"][0].reshape(3, 3), r["t"][0].reshape(3, 1)])
        diff = np.abs(Rt(rc) - Rt(ry)).max()
        print(f"|[R|t] with the call - pinhole| {diff:.3e}")
        assert diff <= margin
        assert ru["status"][0] != 0 or ru["n_inl"][0] < ry["n_inl"][0]                              # without the call: strictly fewer
        Rtrue, ttrue = UC.relative_pose(0, 1)
        assert np.abs(Rt(rc) - np.hstack([Rtrue, ttrue.reshape(3, 1)])).max() < 1e-4
    finally:
        for fe in fes:
            fe.ctx.close()

"""CPU: the scene of tests/undistort_cases.py does what tests/test_gpu_undistort.py uses it for — shown with the oracle and the
checker alone, so that the device tests are about something.

Figures at SCALE = 5 (pair (0, 1), findEssentialMat's 1 px threshold, 60 matches):
    lens displacement of the keypoints of frame 0      median 9.7 px, largest 35.0 px
    E inliers: pinhole / distorted / corrected          60 / 50 / 60
    round-trip residual on these points                 2.38e-3 px;  delta = residual + 3 * 2^-14 = 2.57e-3 px
    sum |d[R|t] / d coordinate| * delta (the margin)    4.8e-4 per entry of [R|t]
    oracle: corrected against pinhole [R|t]             3.0e-6
(at SCALE 1, 2, 3 the distorted pair keeps 60, 60, 58 inliers: a smooth lens is nearly epipolar-consistent over one baseline)"""
import numpy as np

import undistort_cases as UC
import undistort_reference as U


def test_the_rows_match_one_to_one(oracle):
    q, t, _ = oracle.match_hamming(UC.ROWS, UC.ROWS, 2)
    assert np.array_equal(q, np.arange(UC.N)) and np.array_equal(t, np.arange(UC.N))


def test_the_lens_costs_inliers_and_the_checker_restores_them(oracle):
    d = np.linalg.norm(UC.distorted(0).astype(np.float64) - UC.project64(0), axis=1)
    assert 5 < np.median(d) < 15 and 25 < d.max() < 45
    rc_y, mask_y, Rt_y = UC.oracle_pose(oracle, UC.ideal(0), UC.ideal(1))
    rc_u, mask_u, _ = UC.oracle_pose(oracle, UC.distorted(0), UC.distorted(1))
    rc_c, mask_c, Rt_c = UC.oracle_pose(oracle, UC.corrected(0), UC.corrected(1))
    assert (rc_y, rc_u, rc_c) == (0, 0, 0)
    print("inliers", int(mask_y.sum()), int(mask_u.sum()), int(mask_c.sum()))
    assert mask_y.sum() == UC.N and mask_u.sum() <= UC.N - 8 and np.array_equal(mask_c, mask_y)
    R, t = UC.relative_pose(0, 1)
    assert np.abs(Rt_y - np.hstack([R, t.reshape(3, 1)])).max() < 1e-5          # the yardstick is the true motion
    delta, residual = UC.coordinate_error()
    worst = max(np.abs(UC.corrected(k).astype(np.float64) - UC.ideal(k)).max() for k in range(UC.N_FRAMES))
    print(f"residual {residual:.3e} px, delta {delta:.3e} px, corrected - ideal {worst:.3e} px")
    assert 1e-3 < residual < 3e-3 and worst <= delta
    margin, _ = UC.pose_margin(oracle)
    diff = np.abs(Rt_c - Rt_y).max()
    print(f"margin {margin:.3e}, oracle corrected - pinhole {diff:.3e}")
    assert diff <= margin < 1e-3


def test_the_corrected_frames_form_a_chain_that_localises(oracle):
    from test_gpu_chain import reference_chain
    out = reference_chain(oracle, [dict(xy=UC.corrected(k), desc=UC.ROWS) for k in range(UC.N_FRAMES)], UC.PAIRS, UC.K)
    assert out["status"] == [0, 0] and out["E_inl"] == [UC.N] * 2 and out["n_corr"] == [0, UC.N] and out["n_inl"] == [0, UC.N]
    # the distortion is part of the scene: the distorted keypoints are not the corrected ones
    assert all(np.abs(UC.distorted(k) - UC.corrected(k)).max() > 20 for k in range(UC.N_FRAMES))
    assert UC.corrected(0).tobytes() == U.undistort_points(UC.distorted(0), UC.K, UC.DIST, None, UC.K).tobytes()

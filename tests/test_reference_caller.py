"""CPU: the reference's own VisualSlam (src/visual_slam.py, unmodified, read where it lies at run time) runs on the cv2 / g2o
surfaces, through both drop-in routes, with the project's CPU checkers behind the surface (tests/surface_oracle_backend.py).

The reference checkout is looked for in $VO_REFERENCE_SRC, then in ../reference/src beside this repository; without it the tests
skip.  Nothing of it is copied.  Each route runs in a fresh child process (tests/reference_caller_child.py): the drop-in
directory, then the reference's src, lead sys.path there.

Detector: SIFT + NORM_L2, the reference's own constructor lines; the ORB override was not needed (tests/surface_sequence.py
says why and what was observed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import surface_sequence as SS

pytest.importorskip("PIL")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def _reference_src():
    for d in (os.environ.get("VO_REFERENCE_SRC"), os.path.join(os.path.dirname(ROOT), "reference", "src")):
        if d and os.path.isfile(os.path.join(d, "visual_slam.py")):
            return d
    return None


@pytest.fixture(scope="module")
def image_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("surface_sequence")
    SS.write_jpegs(str(d))
    return str(d)


@pytest.mark.parametrize("route", ["dropin", "cv2_only"])
def test_reference_visual_slam_runs_on_the_surfaces(route, image_dir, oracle):
    ref = _reference_src()
    if ref is None:
        pytest.skip("no reference checkout (set VO_REFERENCE_SRC to its src directory)")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "reference_caller_child.py"), route, ref, image_dir, "oracle", SS.DETECTOR],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]                       # VisualSlam(dir) constructed and run() returned
    out = json.loads(r.stdout.strip().splitlines()[-1])
    # the module that carried ImagePair: this package's through `dropin`, the reference's own through `cv2_only`
    owner = os.path.join(ROOT, "visual_odometry_amd", "dropin") if route == "dropin" else ref
    assert os.path.dirname(out["image_pair_file"]) == os.path.abspath(owner)
    # set_camera_matrix(): the numbers of the reference's test.g2o, to its printed precision
    assert np.allclose(out["reference_K"], [802.832, 565.427, 240.124], rtol=0, atol=5e-4)
    assert not out["hip_loaded"]                                      # the whole run stayed on the CPU checkers
    assert out["n_frames"] == out["n_files"] == SS.N_FRAMES          # every file was processed, and run() left its closing loop
    assert out["pnp_retvals"] == [True] * (SS.N_FRAMES - 2) and out["failures"] == []
    assert out["n_cameras"] == SS.N_FRAMES and out["camera_frames"] == list(range(SS.N_FRAMES))
    assert out["poses_finite"] and out["n_observations"] > 0 and out["n_points"] > 0
    assert out["shown"] == ["matches"] and out["n_viewer_calls"] == SS.N_FRAMES - 1
    poses = np.array(out["poses"])
    assert np.array_equal(poses[0], np.eye(3, 4))                     # the first camera stays fixed at the origin
    assert all(np.linalg.norm(p[:, 3]) > 0 for p in poses[1:])        # the others moved


def test_the_gpu_tests_frame_loop_localises_every_frame_on_the_cpu_checkers(image_dir, oracle):
    """tests/surface_walk.py (the loop tests/test_gpu_surface.py runs on the device) on the same files with the oracle backend behind
    the surface: it reaches one camera per frame, so the GPU test's sequence is long enough for both of its solvePnPRansac calls."""
    import surface_oracle_backend
    import surface_walk as SW
    from visual_odometry_amd import cv2_surface, synth
    keep = cv2_surface.backend
    cv2_surface.backend = surface_oracle_backend.OracleBackend()
    try:
        files = sorted(os.path.join(image_dir, f) for f in os.listdir(image_dir))
        steps, poses = SW.walk(SW.SurfaceApi(), files, synth.camera_matrix(SS.WIDTH, SS.HEIGHT))
        assert len(poses) == SS.N_FRAMES and np.isfinite(np.array(poses)).all()
        assert cv2_surface.backend.pnp_retvals == [True] * (SS.N_FRAMES - 2)
        assert [n for n, _ in steps].count("optimize") == SS.N_FRAMES - 1
    finally:
        cv2_surface.backend = keep

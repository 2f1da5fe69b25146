"""Child process of tests/test_reference_caller.py: runs the reference's unmodified VisualSlam.run() on the cv2 / g2o surfaces.

    python reference_caller_child.py ROUTE REFERENCE_SRC IMAGE_DIR BACKEND DETECTOR

ROUTE: "dropin" (visual_odometry_amd/dropin in front of the reference's src: this package's ImagePair / FrameGenerator / Frame)
or "cv2_only" (visual_odometry_amd/dropin/cv2_only: the reference's own modules, only cv2 and g2o replaced).
BACKEND: "oracle" (tests/surface_oracle_backend.OracleBackend: CPU) or "hip" (the surface's default).
DETECTOR: "sift" (the reference's constructor lines as they are) or "orb" (vs.detector / vs.bf / vs.frame_generator set after
construction).  The reference's source is read where it lies; nothing of it is copied.  Prints one JSON line."""
import contextlib
import io
import json
import os
import sys

import numpy as np


def main():
    route, ref_src, image_dir, backend_name, detector = sys.argv[1:6]
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    dropin = os.path.join(root, "visual_odometry_amd", "dropin")
    first = {"dropin": dropin, "cv2_only": os.path.join(dropin, "cv2_only")}[route]
    sys.path[:0] = [first, ref_src, root, tests]

    from visual_odometry_amd import cv2_surface, synth
    if backend_name == "oracle":
        import surface_oracle_backend
        cv2_surface.backend = surface_oracle_backend.OracleBackend()

    import visual_slam                    # the reference's, unmodified
    import image_pair
    import initials
    out = dict(route=route, image_pair_file=os.path.abspath(image_pair.__file__), hip_loaded_at_import=_hip_loaded())
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        vs = visual_slam.VisualSlam(image_dir)
        vs.set_camera_matrix()
        out["reference_K"] = [float(vs.camera_matrix[0, 0]), float(vs.camera_matrix[0, 2]), float(vs.camera_matrix[1, 2])]
        files = sorted(f for f in os.listdir(image_dir) if f.endswith(".jpg"))
        from PIL import Image
        w, h = Image.open(os.path.join(image_dir, files[0])).size
        vs.camera_matrix = synth.camera_matrix(w, h)
        vs.scale_factor = 1.0
        if detector == "orb":
            vs.detector = initials.cv2.ORB_create()
            vs.bf = initials.cv2.BFMatcher(initials.cv2.NORM_HAMMING, crossCheck=True)
            vs.frame_generator = visual_slam.FrameGenerator(vs.detector)
        vs.run()                          # must return: the waitKey script ends its closing loop
    cams = vs.map.cameras
    out.update(n_files=len(files), n_frames=len(vs.list_of_frames), n_cameras=len(cams),
               camera_frames=[int(c.frame_id) for c in cams],
               poses_finite=bool(all(np.isfinite(c.pose()).all() for c in cams)),
               n_observations=len(vs.map.observations), n_points=len(vs.map.points),
               pnp_retvals=[bool(v) for v in getattr(cv2_surface.backend, "pnp_retvals", [])],
               n_viewer_calls=len(initials.ThreeDimViewer.recorded), shown=sorted(cv2_surface.shown),
               failures=[ln for ln in log.getvalue().splitlines()
                         if ln.startswith(("Position estimation failed", "Failed to estimate", "Error in", "Exception in"))],
               poses=[c.pose()[:3].tolist() for c in cams], hip_loaded=_hip_loaded())
    print(json.dumps(out))


def _hip_loaded():
    from visual_odometry_amd import _lib
    return _lib._lib is not None


if __name__ == "__main__":
    main()

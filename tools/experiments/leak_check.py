"""Device-memory leak check: create / configure / use / destroy a context 30 times and compare hipMemGetInfo.

Every cycle touches each allocation lifetime of vo_api.hip: the context's own buffers, the ORB configuration (small -> large
-> small), the pair buffers, a SIFT batch configuration and the single-image SIFT call, the single-call matcher, and the
growable scratch (JPEG decode, resize, triangulation, the localisation chain, the trajectory gather)."""
import sys, os, ctypes as C, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from visual_odometry_amd import _lib, synth, ingest, geometry
from visual_odometry_amd.detector import SiftDetector
from visual_odometry_amd.frontend import FrontEnd
from visual_odometry_amd.matcher import HammingMatcher
hip = C.CDLL("libamdhip64.so")
def free_mb():
    f = C.c_size_t(); t = C.c_size_t(); hip.hipMemGetInfo(C.byref(f), C.byref(t)); return f.value / 2**20
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
jpeg = open(os.path.join(ROOT, "tests", "golden", "jpeg_gray_q1_saturated_329x267.jpg"), "rb").read()
seq = synth.sequence(3, 640, 480, cache_dir="/tmp")
frames, K = seq["frames"], seq["K"]
rng = np.random.default_rng(0)
P1 = np.hstack([np.eye(3), np.zeros((3, 1))]); P2 = np.hstack([np.eye(3), np.array([[1.0], [0.0], [0.0]])])
x1, x2 = rng.random((2, 200)), rng.random((2, 200))
base = None
for it in range(30):
    c = _lib.Context(0)
    fe = FrontEnd(480, 640, max_frames=3, max_pairs=2, nfeatures=500, ctx=c)
    fe.upload(frames); fe.detect(0, 3); fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
    fe.localize_chain(2, K)
    fe.gather_records(2)
    HammingMatcher(crossCheck=True, ctx=c).match_arrays(np.random.default_rng(it).integers(0, 256, (300, 32), dtype=np.uint8), np.random.default_rng(it + 1).integers(0, 256, (280, 32), dtype=np.uint8))
    FrontEnd(1080, 1920, max_frames=4, max_pairs=2, nfeatures=2000, nlevels=4, ctx=c)           # ORB reconfigure: large ...
    FrontEnd(480, 640, max_frames=3, max_pairs=2, nfeatures=500, ctx=c)                         # ... and small again
    sf = FrontEnd(480, 640, max_frames=3, max_pairs=2, detector="sift", ctx=c)
    sf.upload(frames); sf.detect(0, 3)
    SiftDetector(ctx=c).detectAndCompute(frames[0])
    ingest.imdecode(jpeg, c)
    ingest.resize(frames[0], (320, 240), ingest.INTER_AREA, ctx=c)
    geometry.triangulatePoints(P1, P2, x1, x2, ctx=c)
    del fe, sf
    c.close()
    if it == 2: base = free_mb()
    if it in (2, 15, 29): print("iter", it, "free MB", round(free_mb(), 1))
print("leak MB over 27 create/destroy cycles:", round(base - free_mb(), 2))

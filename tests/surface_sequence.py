"""The sequence tests/test_reference_caller.py and tests/test_gpu_surface.py run the frame loop on: synth.sequence frames as
JPEG files, written with Pillow as tests/test_gpu_jpeg.py writes its files.

Chosen on a CPU by running the reference's unmodified VisualSlam.run() through the oracle backend (SIFT + NORM_L2, the
reference's own constructor lines; synth's default seed, straight flight, JPEG quality 90), 4:3 sizes in steps of 16 columns:
   48 x 36   run() raises (too few SIFT keypoints for an essential matrix)
   64 x 48   6 map points after the first pair; localisation fails before solvePnPRansac is reached
   80 x 60   every solvePnPRansac returns retval True: 4 cameras, 35 points, 61 observations      <- the smallest
   96 x 72 .. 320 x 240   localise as well (54 .. 421 points)
and 4 frames is the fewest the loop needs to call solvePnPRansac twice.  One route takes about 1.2 s there, SIFT included, so
ORB / NORM_HAMMING was not needed."""
import io
import os

N_FRAMES, WIDTH, HEIGHT = 4, 80, 60
JPEG_QUALITY = 90
DETECTOR = "sift"


def jpeg_bytes():
    """[N_FRAMES] JPEG files (grey, baseline) of the sequence, and its camera matrix."""
    from PIL import Image
    from visual_odometry_amd import synth
    seq = synth.sequence(N_FRAMES, WIDTH, HEIGHT, workers=1)
    out = []
    for f in seq["frames"]:
        b = io.BytesIO(); Image.fromarray(f).save(b, "JPEG", quality=JPEG_QUALITY)
        out.append(b.getvalue())
    return out, seq["K"]


def write_jpegs(directory):
    files, K = jpeg_bytes()
    for i, data in enumerate(files):
        with open(os.path.join(directory, "frame_%03d.jpg" % i), "wb") as f:
            f.write(data)
    return K

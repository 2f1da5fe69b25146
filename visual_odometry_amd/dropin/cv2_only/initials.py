"""`from initials import *` for the route that replaces only `cv2` and `g2o`: the names of ../initials.py, re-exported.
With this directory (and not its parent) in front of the reference's src on sys.path, the reference's own image_pair.py,
frame_generator.py and frame.py run on the surface."""
from visual_odometry_amd.dropin.initials import *  # noqa: F401,F403

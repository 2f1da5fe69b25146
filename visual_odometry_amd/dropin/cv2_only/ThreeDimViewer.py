"""The headless viewer of ../ThreeDimViewer.py under the reference's module name."""
from visual_odometry_amd.dropin.ThreeDimViewer import ThreeDimViewer, recorded  # noqa: F401

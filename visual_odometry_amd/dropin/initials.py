"""Drop-in module name for the reference's `from initials import *`: every name src/initials.py:1-12 exports.

  cv2             visual_odometry_amd.cv2_surface, always: running on the device is the point
  g2o             visual_odometry_amd.g2o_surface
  ThreeDimViewer  the headless module beside this file
  gl, plt, go     the real module when it imports; otherwise a placeholder that raises ImportError naming the package at the
                  first attribute use (the in-scope callers never touch them)
  Timer           codetiming's when present, otherwise a no-op decorator / context manager
  np, glob, collections, math, time and the four record schemas

Importing this module loads no HIP library."""
import collections  # noqa: F401
import glob  # noqa: F401
import math  # noqa: F401
import time  # noqa: F401

import numpy as np

import ThreeDimViewer  # noqa: F401  (the sibling of this file: its directory is on sys.path)
from visual_odometry_amd import cv2_surface as cv2  # noqa: F401
from visual_odometry_amd import g2o_surface as g2o  # noqa: F401
from visual_odometry_amd.initials import Feature, Match, Match3D, MatchWithMap  # noqa: F401


class _MissingModule:
    """Stands where a module the in-scope callers never use failed to import."""

    def __init__(self, package):
        self.__dict__["_package"] = package

    def __getattr__(self, name):
        raise ImportError(f"{self._package} is not installed: the drop-in `initials` exports a placeholder for it, "
                          f"and `{name}` was read from the placeholder")


def _optional(module, package):
    import importlib
    try:
        return importlib.import_module(module)
    except ImportError:
        return _MissingModule(package)


gl = _optional("OpenGL.GL", "PyOpenGL (OpenGL.GL)")
plt = _optional("matplotlib.pyplot", "matplotlib")
go = _optional("plotly.graph_objects", "plotly")

try:
    from codetiming import Timer  # noqa: F401
except ImportError:
    class Timer:
        """No-op stand-in for codetiming.Timer: `@Timer(text=...)` and `with Timer(...):` run the code untimed."""

        def __init__(self, *args, **kwargs):
            pass

        def __call__(self, fn):
            return fn

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def start(self):
            pass

        def stop(self):
            return 0.0

np.set_printoptions(precision=4, suppress=True)   # src/initials.py:14

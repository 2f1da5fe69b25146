"""The `g2o` names Map.optimize_map uses (src/map.py:105-179; visual_odometry_template_02/visual_slam.py:413-470), as a graph
collector in front of the device bundle adjustment.

The objects only record what the caller builds.  SparseOptimizer.optimize(n) packs the vertices and edges in insertion order,
calls `cv2_surface.backend.bundle_adjust` (by default map_filters.bundle_adjust, i.e. vo_bundle_adjust) and writes the
estimates back into the vertices, where the caller reads them (estimate().translation(), .rotation(), point estimate()).

What the kernel does not express raises NotImplementedError with the reason: an edge information other than the identity, a
point that is not marginalised, a second camera model, more than VO_BA_MAX_CAMERAS cameras or VO_BA_MAX_FREE free ones.
save(path) writes nothing and returns False: the reference never reads the file back.
Importing this module loads no HIP library.  Parity with a g2o build is unpinned (docs/kernels/k_bundle_adjust.md).
"""
from __future__ import annotations

import numpy as np

from . import cv2_surface

VO_BA_MAX_CAMERAS, VO_BA_MAX_FREE = 64, 16        # include/vo_hip.h


class _Solver:
    def __init__(self, inner=None):
        self.inner = inner


class LinearSolverEigenSE3(_Solver):
    pass


class LinearSolverCholmodSE3(_Solver):
    pass


class LinearSolverDenseSE3(_Solver):
    pass


class BlockSolverSE3(_Solver):
    pass


class OptimizationAlgorithmLevenberg(_Solver):
    pass


class RobustKernelHuber:
    def __init__(self, delta=1.0):
        self._delta = float(delta)

    def set_delta(self, delta):
        self._delta = float(delta)

    def delta(self):
        return self._delta


class CameraParameters:
    """g2o.CameraParameters(focal_length, principal_point, baseline): one focal length, as the reference passes it (:113-117)."""

    def __init__(self, focal_length, principal_point, baseline):
        self.focal_length = float(focal_length)
        self.principal_point = (float(principal_point[0]), float(principal_point[1]))
        self.baseline = float(baseline)
        self._id = None

    def set_id(self, i):
        self._id = int(i)

    def id(self):
        return self._id


class Quaternion:
    """Unit quaternion with g2o's accessors.  From a rotation matrix as Eigen converts it (Shepperd's four branches)."""

    def __init__(self, w, x, y, z):
        self._q = (float(w), float(x), float(y), float(z))

    @classmethod
    def from_matrix(cls, R):
        m = np.asarray(R, np.float64).reshape(3, 3)
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        if tr > 0:
            s = np.sqrt(tr + 1.0); w = 0.5 * s; s = 0.5 / s
            return cls(w, (m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s)
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        v = [0.0, 0.0, 0.0]
        v[i] = 0.5 * s
        s = 0.5 / s
        w = (m[k, j] - m[j, k]) * s
        v[j] = (m[j, i] + m[i, j]) * s
        v[k] = (m[k, i] + m[i, k]) * s
        return cls(w, *v)

    def w(self):
        return self._q[0]

    def x(self):
        return self._q[1]

    def y(self):
        return self._q[2]

    def z(self):
        return self._q[3]

    def coeffs(self):
        return np.array([self._q[1], self._q[2], self._q[3], self._q[0]])


class SE3Quat:
    """g2o.SE3Quat(R, t): t may be a 3-vector or 3x1 (the reference hands both: map.py:125 with cameras from recoverPose's
    3x1 t, solvePnPRansac's 3x1 tvec and optimize_map's own 3-vectors)."""

    def __init__(self, R=None, t=None):
        self._R = np.eye(3) if R is None else np.array(R, np.float64).reshape(3, 3)
        self._t = np.zeros(3) if t is None else np.array(t, np.float64).reshape(3)

    def translation(self):
        return self._t.copy()

    def rotation(self):
        return Quaternion.from_matrix(self._R)

    def matrix(self):
        T = np.eye(4); T[:3, :3] = self._R; T[:3, 3] = self._t
        return T


class _Vertex:
    def __init__(self):
        self._id = None
        self._estimate = None

    def set_id(self, i):
        self._id = int(i)

    def id(self):
        return self._id

    def set_estimate(self, e):
        self._estimate = e

    def estimate(self):
        return self._estimate


class VertexSE3Expmap(_Vertex):
    def __init__(self):
        super().__init__()
        self._fixed = False

    def set_fixed(self, fixed):
        self._fixed = bool(fixed)

    def fixed(self):
        return self._fixed


class VertexPointXYZ(_Vertex):
    def __init__(self):
        super().__init__()
        self._marginalized = False

    def set_marginalized(self, m):
        self._marginalized = bool(m)

    def marginalized(self):
        return self._marginalized

    def set_estimate(self, e):
        self._estimate = np.array(e, np.float64).reshape(3)


VertexSBAPointXYZ = VertexPointXYZ


class EdgeProjectXYZ2UV:
    def __init__(self):
        self._v = {}
        self._measurement = None
        self._information = None
        self._kernel = None
        self._parameter = None

    def set_vertex(self, i, v):
        self._v[int(i)] = v

    def vertex(self, i):
        return self._v[int(i)]

    def set_measurement(self, m):
        self._measurement = np.array(m, np.float64).reshape(2)

    def measurement(self):
        return self._measurement

    def set_information(self, info):
        self._information = np.array(info, np.float64)

    def set_robust_kernel(self, k):
        self._kernel = k

    def set_parameter_id(self, slot, param_id):
        self._parameter = (int(slot), int(param_id))


class SparseOptimizer:
    def __init__(self):
        self._algorithm = None
        self._parameters = {}
        self._vertices = {}          # id -> vertex, insertion ordered
        self._edges = []
        self._verbose = False
        self.last_result = None      # what backend.bundle_adjust returned at the last optimize()

    def set_algorithm(self, a):
        self._algorithm = a

    def add_parameter(self, p):
        self._parameters[p.id()] = p
        return True

    def add_vertex(self, v):
        if v.id() is None or v.id() in self._vertices:
            return False
        self._vertices[v.id()] = v
        return True

    def add_edge(self, e):
        self._edges.append(e)
        return True

    def vertices(self):
        return self._vertices

    def vertex(self, i):
        return self._vertices[i]

    def edges(self):
        return self._edges

    def initialize_optimization(self, level=0):
        return True

    def set_verbose(self, v):
        self._verbose = bool(v)

    def save(self, path):
        """Writes nothing and returns False: the reference saves "test.g2o" (map.py:173) and never reads it."""
        return False

    # ---- the graph as arrays
    def pack(self):
        """(poses [ncam, 3, 4], fixed [ncam], points [npt, 3], obs_cam, obs_pt, obs_xy [nobs, 2], focal, cx, cy, huber_delta,
        camera vertices, point vertices): vertices and edges in insertion order.  Raises NotImplementedError for a graph the
        kernel does not express."""
        cams = [v for v in self._vertices.values() if isinstance(v, VertexSE3Expmap)]
        pts = [v for v in self._vertices.values() if isinstance(v, VertexPointXYZ)]
        if len(cams) + len(pts) != len(self._vertices):
            raise NotImplementedError("g2o_surface: only VertexSE3Expmap and VertexPointXYZ vertices are built")
        if len(self._parameters) != 1:
            raise NotImplementedError(f"g2o_surface: exactly one CameraParameters is built, the graph has {len(self._parameters)}")
        cam_par = next(iter(self._parameters.values()))
        if len(cams) > VO_BA_MAX_CAMERAS:
            raise NotImplementedError(f"g2o_surface: {len(cams)} cameras > VO_BA_MAX_CAMERAS = {VO_BA_MAX_CAMERAS}")
        n_free = sum(1 for c in cams if not c.fixed())
        if n_free > VO_BA_MAX_FREE:
            raise NotImplementedError(f"g2o_surface: {n_free} free cameras > VO_BA_MAX_FREE = {VO_BA_MAX_FREE}")
        for p in pts:
            if not p.marginalized():
                raise NotImplementedError(f"g2o_surface: point vertex {p.id()} is not marginalised; the kernel eliminates every point "
                                          "(Schur complement), as set_marginalized(True) asks of g2o")
        cam_row = {id(v): i for i, v in enumerate(cams)}
        pt_row = {id(v): i for i, v in enumerate(pts)}
        n = len(self._edges)
        oc = np.zeros(n, np.int32); op = np.zeros(n, np.int32); xy = np.zeros((n, 2))
        deltas = set()
        for k, e in enumerate(self._edges):
            if not isinstance(e, EdgeProjectXYZ2UV):
                raise NotImplementedError("g2o_surface: only EdgeProjectXYZ2UV edges are built")
            if e._information is None or e._information.shape != (2, 2) or not np.array_equal(e._information, np.identity(2)):
                raise NotImplementedError("g2o_surface: edge information other than the 2x2 identity is not built")
            if e._parameter is not None and e._parameter[1] != cam_par.id():
                raise NotImplementedError(f"g2o_surface: edge names camera parameter {e._parameter[1]}, which the graph does not hold")
            p, c = e._v.get(0), e._v.get(1)
            if id(p) not in pt_row or id(c) not in cam_row:
                raise NotImplementedError("g2o_surface: an edge joins vertex 0 = a point of the graph to vertex 1 = a camera of the graph")
            op[k], oc[k] = pt_row[id(p)], cam_row[id(c)]
            xy[k] = e._measurement
            deltas.add(e._kernel.delta() if e._kernel is not None else 0.0)
        if len(deltas) > 1:
            raise NotImplementedError("g2o_surface: one robust kernel setting for all edges (the kernel takes one huber_delta)")
        delta = deltas.pop() if deltas else 0.0           # no robust kernel: huber_delta <= 0
        poses = np.zeros((len(cams), 3, 4))
        for i, c in enumerate(cams):
            poses[i, :, :3] = c.estimate()._R; poses[i, :, 3] = c.estimate()._t
        points = np.array([p.estimate() for p in pts], np.float64).reshape(-1, 3)
        fixed = np.array([c.fixed() for c in cams], bool)
        return (poses, fixed, points, oc, op, xy, cam_par.focal_length, cam_par.principal_point[0], cam_par.principal_point[1],
                float(delta), cams, pts)

    def optimize(self, iterations, online=False):
        poses, fixed, points, oc, op, xy, f, cx, cy, delta, cams, pts = self.pack()
        r = cv2_surface.backend.bundle_adjust(poses, fixed, points, oc, op, xy, f, cx, cy, int(iterations), delta)
        self.last_result = r
        new_poses = np.asarray(r["poses"], np.float64).reshape(-1, 3, 4)
        new_points = np.asarray(r["points"], np.float64).reshape(-1, 3)
        for i, c in enumerate(cams):
            c.set_estimate(SE3Quat(new_poses[i, :, :3], new_poses[i, :, 3]))
        for i, p in enumerate(pts):
            p.set_estimate(new_points[i])
        return int(r.get("iterations", iterations))


def __getattr__(name):
    raise AttributeError(f"visual_odometry_amd.g2o_surface carries no g2o.{name}: it holds only the names src/map.py's "
                         "optimize_map and the template's bundle adjustment use")

"""PointCloud container exposing exactly the Open3D surface KinectPy's hot path touches
(SURVEY.md 8b / a22), backed by float32 torch-ROCm tensors (device memory containers only;
every operation is a call into libkinectpx.so through kinectpy_amd.ops).

Reference call sites: utils/io.py:28-41 (points/colors get/set through Vector3dVector),
preprocessing/data.py:46-58 (transform in place, np.asarray(points)), preprocessing/filtering.py:23-24,
floor_removal.py:50,61-73 (select_by_index with (K,1) arrays, segment_plane, `+`), registration.py:8-13.
"""
import copy
import enum

import numpy as np
import torch

from . import _lib as L
from . import ops


class Vector3dVector:
    """o3d.utility.Vector3dVector stand-in: wraps an (N,3) array; np.asarray() gives float64."""

    def __init__(self, data=None):
        if isinstance(data, Vector3dVector):
            self.t = data.t
        elif data is None:
            self.t = torch.empty((0, 3), dtype=torch.float32, device=L.device())
        elif isinstance(data, torch.Tensor):
            self.t = data.to(device=L.device(), dtype=torch.float32).reshape(-1, 3).contiguous()
        else:
            a = np.asarray(data)
            if a.size and (a.ndim != 2 or a.shape[1] != 3):
                raise RuntimeError("Vector3dVector: expected an (N, 3) array")
            self.t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)).to(L.device())

    def __array__(self, dtype=None, copy=None):
        a = self.t.cpu().numpy().astype(np.float64)
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return int(self.t.shape[0])

    def __getitem__(self, i):
        return np.asarray(self)[i]


class Matrix3dVector:
    """o3d.utility.Matrix3dVector stand-in: wraps an (N,3,3) float64 array; np.asarray() gives float64 (N,3,3)."""

    def __init__(self, data=None):
        if isinstance(data, Matrix3dVector):
            self.t = data.t
        elif data is None:
            self.t = torch.empty((0, 3, 3), dtype=torch.float64, device=L.device())
        elif isinstance(data, torch.Tensor):
            self.t = data.to(device=L.device(), dtype=torch.float64).reshape(-1, 3, 3).contiguous()
        else:
            a = np.asarray(data)
            if a.size and (a.ndim != 3 or a.shape[1:] != (3, 3)):
                raise RuntimeError("Matrix3dVector: expected an (N, 3, 3) array")
            self.t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3, 3)).to(L.device())

    def __array__(self, dtype=None, copy=None):
        a = self.t.cpu().numpy()
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return int(self.t.shape[0])

    def __getitem__(self, i):
        return np.asarray(self)[i]


class Vector2iVector:
    def __init__(self, data):
        self.a = np.ascontiguousarray(np.asarray(data), dtype=np.int32).reshape(-1, 2)

    def __array__(self, dtype=None, copy=None):
        return self.a if dtype is None else self.a.astype(dtype)

    def __len__(self):
        return len(self.a)


class KDTreeSearchParamHybrid:
    def __init__(self, radius, max_nn):
        self.radius, self.max_nn = float(radius), int(max_nn)


class KDTreeSearchParamKNN:
    def __init__(self, knn=30):
        self.radius, self.max_nn = 1e150, int(knn)


class KDTreeSearchParamRadius:
    def __init__(self, radius):
        self.radius = float(radius)


def _idx_array(indices):
    """accepts lists, (K,), (K,1) arrays (np.argwhere output, floor_removal.py:50,65-69) and tensors"""
    if isinstance(indices, torch.Tensor):
        return indices.reshape(-1).to(torch.int32)
    return np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.int32)


class OrientedBoundingBox:
    """the members the reference reads: R, extent, get_center(), get_rotation_matrix_from_yxz()"""

    def __init__(self, center=None, R=None, extent=None):
        self.center = np.zeros(3) if center is None else np.asarray(center, dtype=np.float64)
        self.R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
        self.extent = np.zeros(3) if extent is None else np.asarray(extent, dtype=np.float64)

    @classmethod
    def _from_row(cls, row):
        return cls(row[9:12].copy(), row[:9].reshape(3, 3).copy(), row[12:15].copy())

    def get_center(self):
        return self.center

    @staticmethod
    def get_rotation_matrix_from_yxz(rotation):
        """Ry(rotation[0]) @ Rx(rotation[1]) @ Rz(rotation[2]) (utils/normalization.py:40)"""
        a, b, c = (float(v) for v in np.asarray(rotation, dtype=np.float64).reshape(3))
        ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
        Ry = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
        Rx = np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
        Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
        return Ry @ Rx @ Rz

    def __repr__(self):
        return f"OrientedBoundingBox: center: {tuple(self.center)}, extent: {tuple(self.extent)}"


class PointCloud:
    """Covariances (`covariances`, estimate_covariances, generalized ICP) are an fp64 (N,3,3) device tensor `_cov`.  transform()
    rotates them, deepcopy / clone() and `+` carry them; every other method returns a cloud WITHOUT covariances -- unlike Open3D,
    whose select_by_index (and the filters built on it) keeps them.

    State.  Copied on entry: whatever the constructor or a setter (points, colors, normals, covariances) is given as a
    Vector3dVector / Matrix3dVector -- another cloud's property included -- and every host array; a bare torch.Tensor of the stored
    dtype, device and layout is adopted without a copy and written in place from then on.  In place, returning self: transform,
    estimate_normals, estimate_covariances, normalize_normals, the three orient_normals_*, `+=` (and utils.processing's
    normalize_pointcloud).  Every other method that returns a cloud (`+`, copy / deepcopy / clone, select_by_index, the down-samplers
    and outlier filters) returns a new one that shares no storage with this cloud or with the other operand."""
    _cov = None
    # _bounds: the cloud's min / max as a float64[6] DEVICE tensor once some kernel has computed them (the gather that produced the
    # cloud, or the first get_*_bound / remove_floor); dropped whenever the points change
    _bounds = None

    # every assignment of _pts (here, in _make, in utils/processing.py) goes through this setter and drops the cached bounds; in-place
    # writes into the tensor (transform()) drop them themselves
    @property
    def _pts(self):
        return self._pts_t

    @_pts.setter
    def _pts(self, t):
        self._pts_t = t
        self._bounds = None

    def __init__(self, points=None):
        self._pts = _taken(points, Vector3dVector)
        self._col = None
        self._nrm = None
        self._cov = None

    # ---- attributes ---------------------------------------------------------------------------
    @property
    def points(self):
        return Vector3dVector(self._pts)

    @points.setter
    def points(self, v):
        self._pts = _taken(v, Vector3dVector)

    @property
    def colors(self):
        return Vector3dVector(self._col if self._col is not None else None)

    @colors.setter
    def colors(self, v):
        t = _taken(v, Vector3dVector)
        self._col = t if t.shape[0] else None

    @property
    def normals(self):
        return Vector3dVector(self._nrm if self._nrm is not None else None)

    @normals.setter
    def normals(self, v):
        t = _taken(v, Vector3dVector)
        self._nrm = t if t.shape[0] else None

    @property
    def covariances(self):
        return Matrix3dVector(self._cov if self._cov is not None else None)

    @covariances.setter
    def covariances(self, v):
        t = _taken(v, Matrix3dVector)
        self._cov = t if t.shape[0] else None

    def has_covariances(self):
        return self._cov is not None and self._cov.shape[0] == self._pts.shape[0] and self.has_points()

    def has_points(self):
        return self._pts.shape[0] > 0

    def has_colors(self):
        return self._col is not None and self._col.shape[0] == self._pts.shape[0] and self.has_points()

    def has_normals(self):
        return self._nrm is not None and self._nrm.shape[0] == self._pts.shape[0] and self.has_points()

    def __repr__(self):
        return f"PointCloud with {self._pts.shape[0]} points."

    @classmethod
    def _make(cls, pts, col=None, nrm=None, bounds=None):
        pc = cls.__new__(cls)
        pc._pts, pc._col, pc._nrm, pc._bounds = pts, col, nrm, bounds
        return pc

    def _device_bounds(self):
        """float64[6] device tensor (min x, y, z, max x, y, z), computed once per cloud"""
        if self._bounds is None:
            self._bounds = ops.bounds(self._pts)
        return self._bounds

    def __deepcopy__(self, memo):
        pc = PointCloud._make(self._pts.clone(), None if self._col is None else self._col.clone(),
                              None if self._nrm is None else self._nrm.clone())
        pc._cov = None if self._cov is None else self._cov.clone()
        return pc

    __copy__ = lambda self: self.__deepcopy__({})

    def _attrs(self):
        return [self._pts, self._col if self.has_colors() else None, self._nrm if self.has_normals() else None]

    # ---- Open3D methods on the path -----------------------------------------------------------
    def get_min_bound(self):
        if not self.has_points():
            return np.zeros(3)
        return self._device_bounds()[:3].cpu().numpy()

    def get_max_bound(self):
        if not self.has_points():
            return np.zeros(3)
        return self._device_bounds()[3:].cpu().numpy()

    def transform(self, T):
        """in place, returns self (preprocessing/data.py:48)"""
        T = np.asarray(T, dtype=np.float64)
        if T.shape != (4, 4):
            raise RuntimeError("transform: expected a 4x4 matrix")
        if self.has_points():
            self._bounds = None
            ops.transform(self._pts, T, out=self._pts)
            if self.has_normals():
                ops.rotate(self._nrm, T, out=self._nrm)
            if self.has_covariances():
                ops.rotate_covariances(self._cov, T, out=self._cov)
        return self

    def select_by_index(self, indices, invert=False):
        idx = _idx_array(indices)
        if not self.has_points():
            return PointCloud()
        p, c, n = ops.select_by_index(self._attrs(), idx, invert)
        return PointCloud._make(p, c, n)

    def _select(self, idx):
        """select_by_index for an index list produced by this library (ascending, duplicate-free, in range): one gather"""
        (p, c, n), bb = ops.select_by_index(self._attrs(), idx, False, trusted=True, want_bounds=True)
        return PointCloud._make(p, c, n, bb)

    def voxel_down_sample(self, voxel_size):
        if not voxel_size > 0:
            raise RuntimeError("voxel_size <= 0.")
        p, c, n = ops.voxel_downsample(self._pts, float(voxel_size), self._col if self.has_colors() else None,
                                       self._nrm if self.has_normals() else None)
        return PointCloud._make(p, c, n)

    def remove_statistical_outlier(self, nb_neighbors, std_ratio, print_progress=False):
        if nb_neighbors < 1 or std_ratio <= 0:
            raise RuntimeError("Illegal input parameters, the number of neighbors and standard deviation ratio must be positive.")
        if not self.has_points():
            return PointCloud(), np.zeros(0, dtype=np.int32)
        idx, _, _ = ops.sor(self._pts, int(nb_neighbors), float(std_ratio))
        (p, c, n), bb = ops.select_by_index(self._attrs(), idx, False, trusted=True, want_bounds=True)
        return PointCloud._make(p, c, n, bb), idx.cpu().numpy()

    def remove_radius_outlier(self, nb_points, radius, print_progress=False):
        if nb_points < 1 or not radius > 0:
            raise RuntimeError("Illegal input parameters, number of points and radius must be positive")
        if not self.has_points():
            return PointCloud(), np.zeros(0, dtype=np.int32)
        idx = ops.remove_radius_outlier(self._pts, int(nb_points), float(radius))
        (p, c, n), bb = ops.select_by_index(self._attrs(), idx, False, trusted=True, want_bounds=True)
        return PointCloud._make(p, c, n, bb), idx.cpu().numpy()

    def farthest_point_down_sample(self, num_samples, start_index=0):
        """[O3D] FarthestPointDownSample: the points picked by farthest-point sampling, in ascending original order (SelectByIndex's
        mask semantics: a repeated pick -- only duplicates left -- appears once, so the cloud may hold fewer than num_samples)."""
        n = len(self._pts) if self.has_points() else 0
        if num_samples == 0:
            return PointCloud()
        if num_samples == n:
            return copy.deepcopy(self)
        if num_samples > n:
            raise RuntimeError(f"Illegal number of samples: {num_samples}, must <= point size: {n}")
        if not 0 <= start_index < n:
            raise RuntimeError(f"Illegal start index: {start_index}, must <= point size: {n}")
        sel, _ = ops.farthest_point_sample(self._pts, int(num_samples), int(start_index))
        p, c, nrm = ops.select_by_index(self._attrs(), sel)
        return PointCloud._make(p, c, nrm)

    def cluster_dbscan(self, eps, min_points, print_progress=False):
        """labels int32 (N): -1 = noise, clusters 0.. numbered by their smallest core point's index (Open3D's order)"""
        if not self.has_points():
            return np.zeros(0, dtype=np.int32)
        labels, cnt = ops.cluster_dbscan(self._pts, float(eps), int(min_points))
        if int(cnt.cpu()[0]) < 0:
            raise RuntimeError("cluster_dbscan: the union pass did not converge")
        return labels.cpu().numpy()

    def segment_plane(self, distance_threshold, ransac_n, num_iterations, probability=0.99999999, seed=None):
        """seed: the reference's RANSAC is unseeded (floor_removal.py:70); ours draws from Philox with
        the given seed (None -> a fresh random seed, i.e. the reference's behaviour)."""
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
        plane, idx = ops.segment_plane(self._pts, float(distance_threshold), int(ransac_n), int(num_iterations),
                                       float(probability), int(seed))
        return plane, idx.cpu().numpy()

    def estimate_normals(self, search_param=None, fast_normal_computation=True):
        sp = search_param if search_param is not None else KDTreeSearchParamKNN()
        if self.has_points():
            self._nrm = ops.estimate_normals(self._pts, sp.radius, sp.max_nn)       # any max_nn up to KPX_NORMALS_MAX_NN (beyond 128 the fall-back heaps live in the workspace)
        return self

    def _need_normals(self, who):
        if not self.has_normals():
            raise RuntimeError(f"{who}: the cloud has no normals (estimate_normals)")

    def normalize_normals(self):
        """[O3D] normalize_normals, in place -> self: every normal of positive length divided by it (AC17); a zero normal stays"""
        if self.has_points():
            self._need_normals("normalize_normals")
            self._nrm = ops.orient_normals(self._nrm, "normalize")
        return self

    def orient_normals_to_align_with_direction(self, orientation_reference=(0.0, 0.0, 1.0)):
        """[O3D] orient_normals_to_align_with_direction, in place -> self: a normal is flipped when its dot product with the reference
        is negative; a zero normal becomes the reference (AC17)"""
        if self.has_points():
            self._need_normals("orient_normals_to_align_with_direction")
            self._nrm = ops.orient_normals(self._nrm, "direction", orientation_reference)
        return self

    def orient_normals_towards_camera_location(self, camera_location=(0.0, 0.0, 0.0)):
        """[O3D] orient_normals_towards_camera_location, in place -> self: a normal is flipped when it points away from the camera; a
        zero normal becomes the unit vector towards it, (0, 0, 1) for a point at the camera (AC17)"""
        if self.has_points():
            self._need_normals("orient_normals_towards_camera_location")
            self._nrm = ops.orient_normals(self._nrm, "camera", camera_location, self._pts)
        return self

    def orient_normals_consistent_tangent_plane(self, k, lambda_penalty=0.0, cos_alpha_tol=1.0):
        """[O3D] orient_normals_consistent_tangent_plane(k), in place -> self: the signs are propagated from the topmost point along
        the minimum spanning tree, under 1 - |n_a . n_b|, of the Riemannian graph (Euclidean minimum spanning tree plus the k nearest
        neighbours), all on the device with every tie pinned (AC17).  Open3D's lambda_penalty / cos_alpha_tol
        variant is not built: anything but their defaults raises NotImplementedError."""
        if float(lambda_penalty) != 0.0 or float(cos_alpha_tol) != 1.0:
            raise NotImplementedError("orient_normals_consistent_tangent_plane: lambda_penalty and cos_alpha_tol are not built (only their defaults)")
        if self.has_points():
            self._need_normals("orient_normals_consistent_tangent_plane")
            self._nrm = ops.orient_normals_tangent(self._pts, self._nrm, k)[0]
        return self

    def estimate_covariances(self, search_param=None):
        """[O3D] estimate_covariances: per point the covariance of its estimate_normals neighbourhood (None: KDTreeSearchParamKNN(30));
        fewer than 3 neighbours give the identity"""
        sp = search_param if search_param is not None else KDTreeSearchParamKNN(30)
        if self.has_points():
            self._cov = ops.estimate_covariances(self._pts, sp.radius, sp.max_nn)
        return self

    def compute_point_cloud_distance(self, target):
        """[O3D] ComputePointCloudDistance: float64 (N) distance of every point to its nearest point of `target`"""
        if not self.has_points():
            return np.zeros(0, dtype=np.float64)
        if not target.has_points():
            raise RuntimeError("compute_point_cloud_distance: the target cloud has no points")
        _, d2, _ = ops.search_knn(ops.search_index(target._pts), self._pts, 1)
        return np.sqrt(d2[:, 0].cpu().numpy())

    def compute_nearest_neighbor_distance(self):
        """[O3D] ComputeNearestNeighborDistance: float64 (N) distance of every point to its nearest OTHER point -- the second
        entry of a 2-nearest search on the cloud itself (0 for a duplicated point); 0 where fewer than two results exist"""
        if not self.has_points():
            return np.zeros(0, dtype=np.float64)
        _, d2, cnt = ops.search_knn(ops.search_index(self._pts), self._pts, 2)
        d2, cnt = d2.cpu().numpy(), cnt.cpu().numpy()
        return np.where(cnt >= 2, np.sqrt(np.where(cnt >= 2, d2[:, 1], 0.0)), 0.0)

    def _iss_keypoint_indices(self, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
        """ascending int32 device tensor of the ISS keypoints' indices (o3d.geometry.keypoint.compute_iss_keypoints)"""
        if salient_radius < 0 or non_max_radius < 0 or min_neighbors < 0:
            raise RuntimeError("compute_iss_keypoints: radii and min_neighbors must be non-negative")
        return ops.iss_keypoints(self._pts, float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32), int(min_neighbors))

    def get_oriented_bounding_box(self, robust=False):
        """utils/normalization.py:39, 74, 105; utils/processing.py:341"""
        obb, _ = ops.obb_batch(self._pts)
        return OrientedBoundingBox._from_row(obb[0].cpu().numpy())

    def __add__(self, other):
        both_c = self.has_colors() and other.has_colors()
        both_n = self.has_normals() and other.has_normals()
        both_v = self.has_covariances() and other.has_covariances()
        if not self.has_points():
            both_c, both_n, both_v = other.has_colors(), other.has_normals(), other.has_covariances()
        # an empty cloud takes the other's attributes over: as copies, like the concatenations (the sum shares nothing with its operands)
        pc = PointCloud._make(torch.cat([self._pts, other._pts], 0),
                              torch.cat([self._col, other._col], 0) if both_c and self.has_points() else (other._col.clone() if both_c else None),
                              torch.cat([self._nrm, other._nrm], 0) if both_n and self.has_points() else (other._nrm.clone() if both_n else None))
        pc._cov = torch.cat([self._cov, other._cov], 0) if both_v and self.has_points() else (other._cov.clone() if both_v else None)
        return pc

    def __iadd__(self, other):
        """in place -> self; `other` is left as it is and shares nothing with the result"""
        r = self + other
        self._pts, self._col, self._nrm, self._cov, self._bounds = r._pts, r._col, r._nrm, r._cov, None
        return self

    def clone(self):
        return copy.deepcopy(self)


class KDTreeFlann:
    """o3d.geometry.KDTreeFlann over a PointCloud or an (N,3) array: the search index (ops.search_index) is built once per
    set_geometry and never per query.  The three *_vector_3d searches take ONE query point and return Open3D's
    (count, indices, squared distances); search_knn / search_radius / search_hybrid take (M,3) queries -- the library's
    extension -- and return device tensors (ops.search_*).  Rows ascend in (d2, index): on equal distances the lowest index comes
    first (Open3D leaves the order of ties open).  Coordinates are float32 storage: float64 input is rounded on entry.  The index is
    self-contained: it answers for the points as they were at set_geometry, whatever happens to the cloud afterwards."""

    def __init__(self, geometry=None):
        self._index = None
        if geometry is not None:
            self.set_geometry(geometry)

    def set_geometry(self, geometry):
        if isinstance(geometry, PointCloud):
            pts = geometry._pts
        elif isinstance(geometry, Vector3dVector):
            pts = geometry.t
        elif isinstance(geometry, torch.Tensor) or (isinstance(geometry, (np.ndarray, list, tuple)) and len(geometry) >= 0):
            pts = geometry if isinstance(geometry, torch.Tensor) else np.asarray(geometry)
            if pts.dtype == object or pts.ndim != 2 or pts.shape[1] != 3:
                raise TypeError("KDTreeFlann: expected a PointCloud or an (N, 3) array of points")
        else:
            raise TypeError(f"KDTreeFlann: expected a PointCloud or an (N, 3) array of points, not {type(geometry).__name__}")
        self._index = ops.search_index(pts)
        return True

    def _need_index(self):
        if self._index is None:
            raise RuntimeError("KDTreeFlann: no geometry set")
        return self._index

    # ---- batched (the library's extension) ---------------------------------------------------------
    def search_knn(self, queries, knn):
        return ops.search_knn(self._need_index(), queries, knn)

    def search_radius(self, queries, radius):
        return ops.search_radius(self._need_index(), queries, radius)

    def search_hybrid(self, queries, radius, max_nn):
        return ops.search_hybrid(self._need_index(), queries, radius, max_nn)

    # ---- Open3D's single-query calls ----------------------------------------------------------------
    @staticmethod
    def _one(query):
        q = np.asarray(query, dtype=np.float64).reshape(-1)
        if q.shape[0] != 3:
            raise RuntimeError("KDTreeFlann: a query is one 3-D point")
        return q.reshape(1, 3)

    def search_knn_vector_3d(self, query, knn):
        idx, d2, cnt = self.search_knn(self._one(query), knn)
        c = int(cnt[0])
        return c, idx[0, :c].cpu().numpy(), d2[0, :c].cpu().numpy()

    def search_hybrid_vector_3d(self, query, radius, max_nn):
        idx, d2, cnt = self.search_hybrid(self._one(query), radius, max_nn)
        c = int(cnt[0])
        return c, idx[0, :c].cpu().numpy(), d2[0, :c].cpu().numpy()

    def search_radius_vector_3d(self, query, radius):
        off, idx, d2 = self.search_radius(self._one(query), radius)
        return int(off[1]), idx.cpu().numpy(), d2.cpu().numpy()

    def search_vector_3d(self, query, search_param):
        if isinstance(search_param, KDTreeSearchParamKNN):
            return self.search_knn_vector_3d(query, search_param.max_nn)
        if isinstance(search_param, KDTreeSearchParamRadius):
            return self.search_radius_vector_3d(query, search_param.radius)
        if isinstance(search_param, KDTreeSearchParamHybrid):
            return self.search_hybrid_vector_3d(query, search_param.radius, search_param.max_nn)
        raise TypeError("KDTreeFlann.search_vector_3d: expected a KDTreeSearchParamKNN, KDTreeSearchParamRadius or KDTreeSearchParamHybrid")


class ImageFilterType(enum.Enum):
    """[O3D] geometry.ImageFilterType; the values are the KPX_IMAGE_* codes of include/kinectpx.h"""
    Gaussian3 = 0
    Gaussian5 = 1
    Gaussian7 = 2
    Sobel3Dx = 3
    Sobel3Dy = 4


class Image:
    """o3d.geometry.Image stand-in: wraps a host ndarray -- uint8 (H, W, 3) colour, uint16 or float32 (H, W) depth / intensity.
    np.asarray(image) gives the array back.  Image(other_image) copies the array; a contiguous ndarray is wrapped as it is."""

    def __init__(self, data=None):
        a = np.zeros((0, 0), np.uint8) if data is None else (data.data.copy() if isinstance(data, Image) else np.ascontiguousarray(data))
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if not ((a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8) or (a.ndim == 2 and a.dtype in (np.uint8, np.uint16, np.float32))):
            raise RuntimeError(f"Image: unsupported array {a.dtype} {a.shape}: expected uint8 (H, W, 3), or uint16 / float32 (H, W)")
        self.data = a

    height = property(lambda self: self.data.shape[0])
    width = property(lambda self: self.data.shape[1] if self.data.ndim > 1 else 0)
    num_of_channels = property(lambda self: self.data.shape[2] if self.data.ndim == 3 else 1)
    bytes_per_channel = property(lambda self: self.data.dtype.itemsize)

    def is_empty(self):
        return self.data.size == 0

    def __array__(self, dtype=None, copy=None):
        return self.data if dtype is None else self.data.astype(dtype)

    def __repr__(self):
        return f"Image of size {self.width}x{self.height}, with {self.num_of_channels} channels."

    def _float_plane(self, who):
        if self.data.ndim != 2 or self.data.dtype != np.float32 or self.data.size == 0:
            raise RuntimeError(f"[{who}] Unsupported image format: a float32 single-channel image is needed.")
        return self.data

    def filter(self, filter_type):
        """[O3D] Image.filter: Gaussian3 / 5 / 7 and Sobel3Dx / y of a float32 single-channel image (kpx_image_filter: separable,
        border pixel repeated, accumulated in fp64 and rounded once per pass) -> a new host Image"""
        return Image(ops.image_filter(self._float_plane("Filter"), ImageFilterType(filter_type).value).cpu().numpy())

    def create_pyramid(self, num_of_levels, with_gaussian_filter=True):
        """[O3D] Image.create_pyramid: level 0 is the image, level i the 2 x 2 block means of level i - 1 (floor(w / 2) x floor(h / 2)),
        Gaussian3-filtered first when with_gaussian_filter -> list of host Images"""
        level = ops._dev(self._float_plane("CreatePyramid"), torch.float32)
        out = [Image(self.data.copy())]
        for _ in range(1, int(num_of_levels)):
            if level.shape[0] < 2 or level.shape[1] < 2:
                raise RuntimeError("[CreatePyramid] the image is too small for that many levels.")
            level = ops.image_downsample(ops.image_filter(level, ImageFilterType.Gaussian3.value) if with_gaussian_filter else level)
            out.append(Image(level.cpu().numpy()))
        return out

    @staticmethod
    def filter_pyramid(pyramid, filter_type):
        """[O3D] Image.filter_pyramid: every level filtered -> list of host Images"""
        return [Image(level).filter(filter_type) for level in pyramid]


class RGBDImage:
    """o3d.geometry.RGBDImage: a colour (or intensity) image and a float32 depth image of the same size"""

    def __init__(self, color=None, depth=None):
        self.color, self.depth = Image(color), Image(depth)

    @staticmethod
    def create_from_color_and_depth(color, depth, depth_scale=1000.0, depth_trunc=3.0, convert_rgb_to_intensity=True):
        """[O3D] RGBDImage::CreateFromColorAndDepth: depth -> float32 raw / depth_scale, values above depth_trunc -> 0 (both in
        float32); colour -> float32 intensity (0.299 r + 0.587 g + 0.114 b) / 255 when convert_rgb_to_intensity, else unchanged."""
        color, depth = Image(color), Image(depth)
        if color.height != depth.height or color.width != depth.width:
            raise RuntimeError("RGBDImage.create_from_color_and_depth: unsupported image format (colour and depth sizes differ)")
        d = np.asarray(depth).astype(np.float32) / np.float32(depth_scale)
        d[d > np.float32(depth_trunc)] = np.float32(0.0)
        c = np.asarray(color)
        if convert_rgb_to_intensity and c.ndim == 3:
            f = c.astype(np.float32)
            c = ((np.float32(0.2990) * f[:, :, 0] + np.float32(0.5870) * f[:, :, 1]) + np.float32(0.1140) * f[:, :, 2]) / np.float32(255.0)
        elif convert_rgb_to_intensity and c.dtype != np.float32:
            c = c.astype(np.float32) / np.float32(255.0 if c.dtype == np.uint8 else 1.0)
        return RGBDImage(c, d)

    def __repr__(self):
        return f"RGBDImage of size \nColor image : {self.color.width}x{self.color.height}, with {self.color.num_of_channels} channels.\nDepth image : {self.depth.width}x{self.depth.height}, with {self.depth.num_of_channels} channels."


def _off_path(name):
    def f(*a, **k):
        raise NotImplementedError(f"{name} is outside the round-1 hot path of kinectpy_amd (SURVEY.md 8f); "
                                  "there is no CPU fallback")
    return f


class Voxel:
    """o3d.geometry.Voxel: grid_index (3 ints) and color (3 floats)"""

    def __init__(self, grid_index=(0, 0, 0), color=(0.0, 0.0, 0.0)):
        self.grid_index = np.asarray(grid_index, dtype=np.int32).reshape(3).copy()
        self.color = np.asarray(color, dtype=np.float64).reshape(3).copy()

    def __repr__(self):
        return f"Voxel with grid_index: ({self.grid_index[0]}, {self.grid_index[1]}, {self.grid_index[2]}), color: ({self.color[0]:g}, {self.color[1]:g}, {self.color[2]:g})"


def _pinhole(intrinsic):
    """PinholeCameraIntrinsic-like -> (width, height, (fx, fy, cx, cy)); AC10 has no skew and K[2, 2] = 1"""
    K = np.asarray(intrinsic.intrinsic_matrix, dtype=np.float64).reshape(3, 3)
    if K[0, 1] != 0.0 or K[2, 2] != 1.0 or K[1, 0] != 0.0 or K[2, 0] != 0.0 or K[2, 1] != 0.0:
        raise RuntimeError("[VoxelGrid] the intrinsic matrix must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew)")
    return int(intrinsic.width), int(intrinsic.height), (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


class VoxelGrid:
    """[O3D] geometry.VoxelGrid (arithmetic contract AC10): `origin`, `voxel_size` and M voxels kept on the device as
    `_keys` (int64 (M,), gx << 42 | gy << 21 | gz, strictly ascending -- Open3D keeps a hash map, and its get_voxels() comes in the
    map's order) with one float32 colour triple each (`_col`).  Besides Open3D's surface: the batch forms carve_depth_maps /
    carve_silhouettes (raw uint16 frames / uint8 masks of all sensors in one pass), the device accessors voxel_indices / voxel_colors
    and included_mask.  get_voxel_center_coordinate / get_voxel_bounding_points are pure arithmetic: they do not look the voxel up
    (Open3D returns zeros for an absent one).  add_voxel, remove_voxel, the octree conversions and create_from_triangle_mesh are off
    the path and raise."""
    AXIS_BITS = ops.VOXELGRID_AXIS_BITS
    AXIS_CELLS = 1 << AXIS_BITS

    def __init__(self, other=None):
        self.origin = np.zeros(3)
        self.voxel_size = 0.0
        self._keys = self._col = None
        if other is not None:
            self.origin, self.voxel_size = np.array(other.origin, dtype=np.float64).reshape(3), float(other.voxel_size)
            if other._keys is not None:
                self._keys, self._col = other._keys.clone(), other._col.clone()

    @classmethod
    def _make(cls, keys, col, origin, voxel_size):
        g = cls()
        g._keys, g._col = keys, col
        g.origin, g.voxel_size = np.asarray(origin, dtype=np.float64).reshape(3).copy(), float(voxel_size)
        return g

    def __deepcopy__(self, memo):
        return VoxelGrid(self)

    __copy__ = lambda self: self.__deepcopy__({})

    def _count(self):
        return 0 if self._keys is None else int(self._keys.shape[0])

    # ---- constructors -------------------------------------------------------------------------
    @staticmethod
    def create_from_point_cloud(input, voxel_size):
        """origin = min_bound - voxel_size / 2; colour of a voxel = mean colour of its points (zeros without colours)"""
        if not voxel_size > 0:
            raise RuntimeError("[VoxelGrid] voxel_size <= 0.")
        if not input.has_points():
            return VoxelGrid._make(None, None, np.zeros(3) - float(voxel_size) * 0.5, voxel_size)
        keys, col, origin = ops.voxelgrid_from_cloud(input._pts, float(voxel_size), input._col if input.has_colors() else None)
        return VoxelGrid._make(keys, col, origin, voxel_size)

    @staticmethod
    def create_from_point_cloud_within_bounds(input, voxel_size, min_bound, max_bound):
        """origin = min_bound; points beyond max_bound are indexed like any other, as Open3D does"""
        if not voxel_size > 0:
            raise RuntimeError("[VoxelGrid] voxel_size <= 0.")
        lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in (min_bound, max_bound))
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise RuntimeError("[VoxelGrid] min_bound and max_bound must be finite")
        if float(voxel_size) * float(np.iinfo(np.int32).max) < (hi - lo).max():
            raise RuntimeError("[VoxelGrid] voxel_size is too small.")
        if not input.has_points():
            return VoxelGrid._make(None, None, lo, voxel_size)
        keys, col, origin = ops.voxelgrid_from_cloud(input._pts, float(voxel_size), input._col if input.has_colors() else None, origin=lo)
        return VoxelGrid._make(keys, col, origin, voxel_size)

    @staticmethod
    def create_dense(origin, color, voxel_size, width, height, depth):
        """all round(extent / voxel_size) cells per axis (half away from zero, as std::round), every voxel with `color`"""
        if not voxel_size > 0:
            raise RuntimeError("[VoxelGrid] voxel_size <= 0.")
        dims = []
        for extent in (width, height, depth):
            q = float(extent) / float(voxel_size)
            if not np.isfinite(q) or q < -0.5:
                raise RuntimeError("[VoxelGrid] create_dense: width, height and depth must be finite and non-negative")
            n = np.floor(abs(q))
            dims.append(int(n) + (1 if abs(q) - n >= 0.5 else 0))
        if max(dims) > VoxelGrid.AXIS_CELLS or dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
            raise RuntimeError(f"[VoxelGrid] create_dense: at most 2^{VoxelGrid.AXIS_BITS} cells per axis and 2^31 - 1 voxels ({dims[0]} x {dims[1]} x {dims[2]})")
        org = np.asarray(origin, dtype=np.float64).reshape(3)
        if dims[0] * dims[1] * dims[2] == 0:
            return VoxelGrid._make(None, None, org, voxel_size)
        keys, col = ops.voxelgrid_dense(dims, np.asarray(color, dtype=np.float64).reshape(3))
        return VoxelGrid._make(keys, col, org, voxel_size)

    create_from_triangle_mesh = staticmethod(_off_path("VoxelGrid.create_from_triangle_mesh"))
    create_from_triangle_mesh_within_bounds = staticmethod(_off_path("VoxelGrid.create_from_triangle_mesh_within_bounds"))
    create_from_octree = _off_path("VoxelGrid.create_from_octree")
    to_octree = _off_path("VoxelGrid.to_octree")
    add_voxel = _off_path("VoxelGrid.add_voxel")
    remove_voxel = _off_path("VoxelGrid.remove_voxel")

    # ---- state --------------------------------------------------------------------------------
    def has_voxels(self):
        return self._count() > 0

    def has_colors(self):
        return True                     # [O3D]: always (a grid built without colours holds zeros)

    def is_empty(self):
        return not self.has_voxels()

    def clear(self):
        self.origin, self.voxel_size, self._keys, self._col = np.zeros(3), 0.0, None, None
        return self

    def __repr__(self):
        return f"VoxelGrid with {self._count()} voxels."

    @property
    def voxel_indices(self):
        """int32 (M, 3) device tensor, ascending (gx, gy, gz)"""
        if self._keys is None:
            return torch.empty((0, 3), dtype=torch.int32, device=L.device())
        mask = self.AXIS_CELLS - 1
        k = self._keys
        return torch.stack([k >> (2 * self.AXIS_BITS), (k >> self.AXIS_BITS) & mask, k & mask], 1).to(torch.int32)

    @property
    def voxel_colors(self):
        """float32 (M, 3) device tensor, in the order of voxel_indices"""
        return torch.empty((0, 3), dtype=torch.float32, device=L.device()) if self._col is None else self._col

    def get_voxels(self):
        """host list of Voxel, ascending (gx, gy, gz)"""
        if not self.has_voxels():
            return []
        idx, col = self.voxel_indices.cpu().numpy(), self._col.cpu().numpy().astype(np.float64)
        return [Voxel(i, c) for i, c in zip(idx, col)]

    # ---- index arithmetic (host, fp64) --------------------------------------------------------
    def get_voxel(self, point):
        p = np.asarray(point, dtype=np.float64).reshape(3)
        return np.floor((p - self.origin) / self.voxel_size).astype(np.int32)

    def get_voxel_center_coordinate(self, idx):
        g = np.asarray(idx, dtype=np.float64).reshape(3)
        return self.origin + (g + 0.5) * self.voxel_size

    def get_voxel_bounding_points(self, index):
        c, r = self.get_voxel_center_coordinate(index), self.voxel_size * 0.5
        return [c + np.array(s) * r for s in ((-1, -1, -1), (-1, -1, 1), (1, -1, -1), (1, -1, 1), (-1, 1, -1), (-1, 1, 1), (1, 1, -1), (1, 1, 1))]

    def _index_range(self):
        idx = self.voxel_indices
        return idx.min(0).values.cpu().numpy().astype(np.float64), idx.max(0).values.cpu().numpy().astype(np.float64)

    def get_min_bound(self):
        if not self.has_voxels():
            return self.origin.copy()
        return self.origin + self._index_range()[0] * self.voxel_size

    def get_max_bound(self):
        if not self.has_voxels():
            return self.origin.copy()
        return self.origin + (self._index_range()[1] + 1.0) * self.voxel_size

    def get_center(self):
        return (self.get_min_bound() + self.get_max_bound()) * 0.5

    # ---- inclusion ----------------------------------------------------------------------------
    def included_mask(self, points):
        """device bool tensor: does each point (a PointCloud, Vector3dVector, (N, 3) float32 / float64 tensor or array) lie in a voxel"""
        if isinstance(points, PointCloud):
            points = points._pts
        elif isinstance(points, Vector3dVector):
            points = points.t
        elif not isinstance(points, torch.Tensor):
            points = np.asarray(points)
            points = np.ascontiguousarray(points if points.dtype == np.float32 else points.astype(np.float64)).reshape(-1, 3)
        if not self.voxel_size > 0:
            raise RuntimeError("[VoxelGrid] voxel_size <= 0.")
        keys = self._keys if self._keys is not None else torch.empty(0, dtype=torch.int64, device=L.device())
        return ops.voxelgrid_included(keys, self.origin, self.voxel_size, points).to(torch.bool)

    def check_if_included(self, queries):
        return [bool(b) for b in self.included_mask(queries).cpu().tolist()]

    # ---- carving ------------------------------------------------------------------------------
    def _carve(self, mode, images, width, height, K, extrinsics, keep_outside, keep_unmeasured=False, depth_scale=1.0, depth_trunc=0.0):
        if self.has_voxels():
            self._keys, self._col = ops.voxelgrid_carve(self._keys, self._col, self.origin, self.voxel_size, mode, images, width, height, K, extrinsics,
                                                        keep_outside, keep_unmeasured, depth_scale, depth_trunc)
        return self

    def _carve_image(self, who, mode, image, camera_params, keep_outside, keep_unmeasured):
        width, height, K = _pinhole(camera_params.intrinsic)
        a = np.asarray(image)
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if a.ndim != 2 or a.dtype != np.float32:
            raise RuntimeError(f"[VoxelGrid] {who}: Unsupported image format (one channel of float32 expected).")
        if a.shape != (height, width):
            raise RuntimeError(f"[VoxelGrid] provided {who} dimensions are not compatible with the provided camera_parameters")
        if width < 2 or height < 2:
            raise RuntimeError(f"[VoxelGrid] {who}: images need width, height >= 2")
        E = np.asarray(camera_params.extrinsic, dtype=np.float64).reshape(1, 4, 4)
        if not self.has_voxels():
            return self
        return self._carve(mode, [torch.as_tensor(np.ascontiguousarray(a)).to(L.device())], width, height, K, E, keep_outside, keep_unmeasured)

    def carve_depth_map(self, depth_map, camera_params, keep_voxels_outside_image=False, keep_unmeasured=False):
        """[O3D] carve_depth_map: a voxel stays when one of its 8 corners projects into the image at a pixel with 0 < depth <= z (or
        outside it, with keep_voxels_outside_image).  keep_unmeasured (extension): a corner on a pixel without depth keeps too."""
        return self._carve_image("depth_map", "depth", depth_map, camera_params, keep_voxels_outside_image, keep_unmeasured)

    def carve_silhouette(self, silhouette_mask, camera_params, keep_voxels_outside_image=False):
        """[O3D] carve_silhouette: a voxel stays when one of its 8 corners projects onto the mask (sample > 0)"""
        return self._carve_image("silhouette_mask", "silhouette", silhouette_mask, camera_params, keep_voxels_outside_image, False)

    def _frames(self, who, frames, dtypes, count, width, height):
        if isinstance(frames, torch.Tensor):
            t = frames.view(torch.uint8) if frames.dtype == torch.bool else frames
        else:
            a = np.ascontiguousarray(frames)
            t = torch.as_tensor(a.view(np.uint8) if a.dtype == np.bool_ else a)
        if t.dtype not in dtypes or t.numel() != count * width * height:
            raise RuntimeError(f"[VoxelGrid] {who}: Unsupported image format.")
        if width < 2 or height < 2:
            raise RuntimeError(f"[VoxelGrid] {who}: images need width, height >= 2")
        return t.reshape(count, width * height)

    def carve_depth_maps(self, depths, intrinsic, extrinsics, keep_voxels_outside_image=False, depth_scale=1000.0, depth_trunc=3.0,
                         keep_unmeasured=False):
        """The batch form: S raw uint16 depth frames ((S, H W) or (S, H, W), host or device) and S extrinsics (world -> camera) carve
        the grid in one pass; depth_scale / depth_trunc as in RGBDImage.create_from_color_and_depth, applied in the kernel.
        Bit-identical to S carve_depth_map() calls with the converted float32 images, in any order."""
        width, height, K = _pinhole(intrinsic)
        E = np.asarray(extrinsics, dtype=np.float64).reshape(-1, 4, 4)
        t = self._frames("carve_depth_maps", depths, (torch.uint16,), len(E), width, height)
        if not self.has_voxels():
            return self
        return self._carve("depth", list(t.to(L.device())), width, height, K, E, keep_voxels_outside_image, keep_unmeasured, depth_scale, depth_trunc)

    def carve_silhouettes(self, masks, intrinsic, extrinsics, keep_voxels_outside_image=False):
        """The batch form of carve_silhouette: S uint8 or bool masks (nonzero = inside), one pass"""
        width, height, K = _pinhole(intrinsic)
        E = np.asarray(extrinsics, dtype=np.float64).reshape(-1, 4, 4)
        t = self._frames("carve_silhouettes", masks, (torch.uint8,), len(E), width, height)
        if not self.has_voxels():
            return self
        return self._carve("silhouette", list(t.to(L.device())), width, height, K, E, keep_voxels_outside_image)


class Vector3iVector:
    """o3d.utility.Vector3iVector stand-in: wraps a (T, 3) int32 array (a triangle list); np.asarray() gives int32.  Host data
    stays on the host until a TriangleMesh takes it."""

    def __init__(self, data=None):
        if isinstance(data, Vector3iVector):
            self.t = data.t
        elif data is None:
            self.t = torch.empty((0, 3), dtype=torch.int32)
        elif isinstance(data, torch.Tensor):
            self.t = data.to(dtype=torch.int32).reshape(-1, 3).contiguous()
        else:
            a = np.asarray(data)
            if a.size and (a.ndim != 2 or a.shape[1] != 3):
                raise RuntimeError("Vector3iVector: expected a (T, 3) array")
            self.t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 3))

    def __array__(self, dtype=None, copy=None):
        a = self.t.cpu().numpy()
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return int(self.t.shape[0])

    def __getitem__(self, i):
        return np.asarray(self)[i]


def _taken(v, wrap, device=None):
    """The tensor a constructor or setter of PointCloud / TriangleMesh stores for `v`.  A wrapper -- what another
    geometry's property hands out -- is copied, so no two geometries share storage (once: a wrapper of host triangles that moving to
    `device` has copied already is not copied again); a host array becomes a new device tensor anyway; a bare torch.Tensor is
    ADOPTED: when it already has the dtype, device and layout the object keeps, the object works in it, in place, without a copy."""
    t = wrap(v).t
    if device is not None:
        t = t.to(device)
    return t.clone() if isinstance(v, (Vector3dVector, Matrix3dVector, Vector3iVector)) and t is v.t else t


class FilterScope(enum.Enum):
    """[O3D] geometry.FilterScope: the arrays a TriangleMesh.filter_smooth_* call filters"""
    All = 0
    Color = 1
    Normal = 2
    Vertex = 3


class TriangleMesh:
    """[O3D] geometry.TriangleMesh, the part a fused surface needs: float32 (V, 3) vertices, int32 (T, 3) triangles and the optional
    vertex colours, vertex normals and triangle normals, all device tensors; normals and area are arithmetic contract AC12
    (kpx_mesh_normals, kpx_mesh_surface_area).  The clean-up path is arithmetic contract AC13, all on the device:
    adjacency (compute_adjacency_list), edges (get_non_manifold_edges, is_edge_manifold), cluster_connected_triangles, ordered removal
    (remove_triangles_by_mask / _by_index, remove_vertices_by_mask / _by_index, remove_unreferenced_vertices,
    remove_degenerate_triangles, select_by_index), smoothing (filter_smooth_simple / _laplacian / _taubin) and sample_points_uniformly.
    The checks are arithmetic contract AC15: get_non_manifold_vertices / is_vertex_manifold,
    get_self_intersecting_triangles / is_self_intersecting / is_intersecting (a triangle-triangle search over RaycastingScene's box
    hierarchy), is_orientable / orient_triangles, get_volume and euler_poincare_characteristic; watertightness is
    ops.mesh_is_watertight(vertices, triangles) on the mesh's arrays.
    Not built: remove_duplicated_vertices, remove_duplicated_triangles, the simplification methods, is_watertight as a method (the
    clean-up suite holds the class to not having it), sample_points_poisson_disk, crop, is_bounding_box_intersecting.

    State.  Copied on entry: whatever the constructor or a setter (vertices, triangles, vertex_colors, vertex_normals,
    triangle_normals) is given as a Vector3dVector / Vector3iVector -- another mesh's property included -- and every host array; a
    bare torch.Tensor of the stored dtype, device and layout is adopted without a copy and written in place from then on.  In place,
    returning self: transform, compute_triangle_normals, compute_vertex_normals, compute_adjacency_list and the remove_* family;
    orient_triangles rewrites the triangles in place and returns whether it could; sample_points_uniformly(use_triangle_normal=True)
    fills missing triangle normals.  copy / deepcopy, select_by_index and filter_smooth_* return a new mesh, sample_points_uniformly a
    new cloud, that share no storage with this mesh.  Cached answers (the bounds, the adjacency list) are dropped by whatever changes
    the arrays they were computed from."""
    _bounds = None
    _adj = None               # (offsets, neighbours) device tensors: compute_adjacency_list's CSR
    _adj_sets = None          # the same as Python sets, built on first use of adjacency_list

    def __init__(self, vertices=None, triangles=None):
        self._vert = _taken(vertices, Vector3dVector)
        self._tri = _taken(triangles, Vector3iVector, L.device())
        self._vcol = self._vnrm = self._tnrm = None

    @classmethod
    def _make(cls, vert, tri, vcol=None, vnrm=None, tnrm=None):
        m = cls.__new__(cls)
        m._vert, m._tri, m._vcol, m._vnrm, m._tnrm = vert, tri, vcol, vnrm, tnrm
        return m

    # ---- attributes ---------------------------------------------------------------------------
    @property
    def vertices(self):
        return Vector3dVector(self._vert)

    @vertices.setter
    def vertices(self, v):
        self._vert, self._bounds = _taken(v, Vector3dVector), None

    @property
    def triangles(self):
        return Vector3iVector(self._tri)

    @triangles.setter
    def triangles(self, v):
        self._tri = _taken(v, Vector3iVector, L.device())
        self._adj = self._adj_sets = None

    def _optional(name):
        def get(self):
            t = getattr(self, name)
            return Vector3dVector(t if t is not None else None)

        def put(self, v):
            t = _taken(v, Vector3dVector)
            setattr(self, name, t if t.shape[0] else None)
        return property(get, put)

    vertex_colors, vertex_normals, triangle_normals = _optional("_vcol"), _optional("_vnrm"), _optional("_tnrm")
    del _optional

    def has_vertices(self):
        return self._vert.shape[0] > 0

    def has_triangles(self):
        return self.has_vertices() and self._tri.shape[0] > 0

    def has_vertex_colors(self):
        return self.has_vertices() and self._vcol is not None and self._vcol.shape[0] == self._vert.shape[0]

    def has_vertex_normals(self):
        return self.has_vertices() and self._vnrm is not None and self._vnrm.shape[0] == self._vert.shape[0]

    def has_triangle_normals(self):
        return self.has_triangles() and self._tnrm is not None and self._tnrm.shape[0] == self._tri.shape[0]

    def is_empty(self):
        return not self.has_vertices()

    def __repr__(self):
        return f"TriangleMesh with {self._vert.shape[0]} points and {self._tri.shape[0]} triangles."

    def __deepcopy__(self, memo):
        c = lambda t: None if t is None else t.clone()
        return TriangleMesh._make(self._vert.clone(), self._tri.clone(), c(self._vcol), c(self._vnrm), c(self._tnrm))

    __copy__ = lambda self: self.__deepcopy__({})

    # ---- Open3D methods -------------------------------------------------------------------------
    def compute_triangle_normals(self, normalized=True):
        self._tnrm, _ = ops.mesh_normals(self._vert, self._tri, normalized, want_vertex=False)
        return self

    def compute_vertex_normals(self, normalized=True):
        """also fills the triangle normals, as Open3D does"""
        self._tnrm, self._vnrm = ops.mesh_normals(self._vert, self._tri, normalized)
        return self

    def get_surface_area(self):
        return ops.mesh_surface_area(self._vert, self._tri)

    def _device_bounds(self):
        if self._bounds is None:
            self._bounds = ops.bounds(self._vert)
        return self._bounds

    def get_min_bound(self):
        if not self.has_vertices():
            return np.zeros(3)
        return self._device_bounds()[:3].cpu().numpy()

    def get_max_bound(self):
        if not self.has_vertices():
            return np.zeros(3)
        return self._device_bounds()[3:].cpu().numpy()

    def transform(self, T):
        """in place, returns self: the vertices through T, vertex and triangle normals through its rotation"""
        T = np.asarray(T, dtype=np.float64)
        if T.shape != (4, 4):
            raise RuntimeError("transform: expected a 4x4 matrix")
        if self.has_vertices():
            self._bounds = None
            ops.transform(self._vert, T, out=self._vert)
            if self.has_vertex_normals():
                ops.rotate(self._vnrm, T, out=self._vnrm)
            if self.has_triangle_normals():
                ops.rotate(self._tnrm, T, out=self._tnrm)
        return self

    # ---- clean-up (AC13) ------------------------------------------------------------------------
    def compute_adjacency_list(self):
        """[O3D] ComputeAdjacencyList: N(v) as CSR on the device (ops.mesh_adjacency); adjacency_list turns it into sets on the host"""
        self._adj, self._adj_sets = ops.mesh_adjacency(self._vert, self._tri), None
        return self

    def has_adjacency_list(self):
        return self.has_vertices() and self._adj is not None and self._adj[0].shape[0] == self._vert.shape[0] + 1

    @property
    def adjacency_list(self):
        """a list of V Python sets, as in Open3D; empty before compute_adjacency_list()"""
        if not self.has_adjacency_list():
            return []
        if self._adj_sets is None:
            off, nb = (t.cpu().numpy() for t in self._adj)
            self._adj_sets = [set(nb[off[v]:off[v + 1]].tolist()) for v in range(len(off) - 1)]
        return self._adj_sets

    def get_non_manifold_edges(self, allow_boundary_edges=True):
        """-> Vector2iVector of ascending (min, max) vertex pairs"""
        return Vector2iVector(ops.mesh_non_manifold_edges(self._vert, self._tri, allow_boundary_edges).cpu().numpy())

    def is_edge_manifold(self, allow_boundary_edges=True):
        return ops.mesh_non_manifold_edges(self._vert, self._tri, allow_boundary_edges).shape[0] == 0

    def cluster_connected_triangles(self):
        """-> (triangle_clusters int32 (T,), cluster_n_triangles int32 (C,), cluster_area float64 (C,)) device tensors; clusters are
        numbered by their smallest triangle, as Open3D's search from ascending seeds numbers them"""
        return ops.mesh_cluster_triangles(self._vert, self._tri)

    # ---- checks (AC15) ---------------------------------------------------------------------------
    def get_non_manifold_vertices(self):
        """-> int32 array, ascending: the vertices whose triangles do not form one fan (or one open fan) around them.  A vertex that
        no triangle names once is not reported (Open3D reads an empty map there)."""
        return ops.mesh_non_manifold_vertices(self._vert, self._tri).cpu().numpy()

    def is_vertex_manifold(self):
        return ops.mesh_non_manifold_vertices(self._vert, self._tri).shape[0] == 0

    def get_self_intersecting_triangles(self):
        """-> Vector2iVector of (t0, t1), t0 < t1, ascending: the intersecting pairs that share no vertex index"""
        return Vector2iVector(ops.mesh_self_intersections(self._vert, self._tri).cpu().numpy())

    def is_self_intersecting(self):
        return ops.mesh_is_self_intersecting(self._vert, self._tri)

    def is_intersecting(self, other):
        """whether some triangle of this mesh meets some triangle of `other` (no shared-vertex exemption)"""
        if not isinstance(other, TriangleMesh):
            raise RuntimeError(f"is_intersecting: expected a TriangleMesh, got {type(other).__name__}")
        if not self.has_triangles() or not other.has_triangles():
            return False
        return ops.rayscene_triangles_meet(ops.rayscene_build(other._vert, other._tri), self._vert, self._tri)

    def is_orientable(self):
        return ops.mesh_orientation(self._vert, self._tri)[0]

    def orient_triangles(self):
        """-> whether the mesh is orientable.  If so the triangles are rewritten in place: in every connected component the smallest
        triangle keeps its winding, the others are flipped ((t0, t1, t2) -> (t0, t2, t1), a stored triangle normal negated) where
        they contradict it; vertex normals are not touched.  Otherwise the mesh stays bit for bit as it was."""
        tn = self._tnrm if self.has_triangle_normals() else None
        ok, _, tri, tn = ops.mesh_orientation(self._vert, self._tri, True, tn)
        if ok:
            self._tri = tri
            if tn is not None:
                self._tnrm = tn
        return ok

    def get_volume(self):
        """the volume a watertight, orientable mesh encloses; raises RuntimeError for any other mesh, as Open3D does"""
        if not ops.mesh_is_watertight(self._vert, self._tri):
            raise RuntimeError("get_volume: the mesh is not watertight")
        if not self.is_orientable():
            raise RuntimeError("get_volume: the mesh is not orientable")
        return ops.mesh_volume(self._vert, self._tri)

    def euler_poincare_characteristic(self):
        """V - E + F with E the number of distinct undirected edges"""
        return self._vert.shape[0] - ops.mesh_edge_count(self._vert, self._tri) + self._tri.shape[0]

    def _set_triangles(self, tri, tnrm):
        self._tri, self._tnrm, self._adj, self._adj_sets = tri, tnrm, None, None
        return self

    def _remove_triangles(self, flags):
        tn = self._tnrm if self.has_triangle_normals() else None
        return self._set_triangles(*ops.mesh_select_triangles(self._tri, flags, True, tn))

    def remove_triangles_by_mask(self, triangle_mask):
        """True removes the triangle; the triangle normals follow.  In place, returns self."""
        return self._remove_triangles(ops._mesh_flag_bytes("remove_triangles_by_mask", triangle_mask, self._tri.shape[0]))

    def remove_triangles_by_index(self, triangle_indices):
        return self._remove_triangles(ops.mesh_flags("indices", None, 0, triangle_indices, self._tri.shape[0]))

    def remove_degenerate_triangles(self):
        return self._remove_triangles(ops.mesh_flags("degenerate", self._tri, self._vert.shape[0]))

    def _select_vertices(self, flags, invert, into=None):
        m = self if into is None else into
        col = self._vcol if self.has_vertex_colors() else None
        nrm = self._vnrm if self.has_vertex_normals() else None
        tn = self._tnrm if self.has_triangle_normals() else None
        m._vert, m._vcol, m._vnrm, tri, tn = ops.mesh_select_vertices(self._vert, self._tri, flags, invert, col, nrm, tn)
        m._bounds = None
        return m._set_triangles(tri, tn)

    def remove_vertices_by_mask(self, vertex_mask):
        """True removes the vertex and every triangle that names it; the kept vertices keep their order and are renumbered by rank,
        colours, vertex normals and triangle normals follow.  In place, returns self."""
        return self._select_vertices(ops._mesh_flag_bytes("remove_vertices_by_mask", vertex_mask, self._vert.shape[0]), True)

    def remove_vertices_by_index(self, vertex_indices):
        return self._select_vertices(ops.mesh_flags("indices", None, 0, vertex_indices, self._vert.shape[0]), True)

    def remove_unreferenced_vertices(self):
        return self._select_vertices(ops.mesh_flags("referenced", self._tri, self._vert.shape[0]), False)

    def select_by_index(self, indices, cleanup=True):
        """a new mesh of the named vertices, IN VERTEX ORDER (duplicates count once; Open3D keeps the list's order), with the triangles
        whose three corners are named; cleanup drops the vertices those triangles leave unreferenced"""
        m = self._select_vertices(ops.mesh_flags("indices", None, 0, indices, self._vert.shape[0]), False, TriangleMesh.__new__(TriangleMesh))
        return m.remove_unreferenced_vertices() if cleanup else m

    def _smooth(self, method, number_of_iterations, lambda_filter, mu, filter_scope):
        scope = FilterScope(filter_scope)
        on = (scope in (FilterScope.All, FilterScope.Vertex), scope in (FilterScope.All, FilterScope.Normal), scope in (FilterScope.All, FilterScope.Color))
        nrm = self._vnrm if self.has_vertex_normals() else None
        col = self._vcol if self.has_vertex_colors() else None
        v, n, c = ops.mesh_smooth(self._vert, self._tri, method, number_of_iterations, lambda_filter, mu, nrm, col, on)
        return TriangleMesh._make(v, self._tri.clone(), c, n)              # mesh_smooth's outputs share no storage with its inputs

    def filter_smooth_simple(self, number_of_iterations=1, filter_scope=FilterScope.All):
        """a new mesh (same triangles, no triangle normals): every vertex value becomes the mean of itself and its neighbours'"""
        return self._smooth("simple", number_of_iterations, 0.0, 0.0, filter_scope)

    def filter_smooth_laplacian(self, number_of_iterations=1, lambda_filter=0.5, filter_scope=FilterScope.All):
        return self._smooth("laplacian", number_of_iterations, lambda_filter, 0.0, filter_scope)

    def filter_smooth_taubin(self, number_of_iterations=1, lambda_filter=0.5, mu=-0.53, filter_scope=FilterScope.All):
        """each iteration is a Laplacian step with lambda_filter, then one with mu (negative: it undoes the shrinkage)"""
        return self._smooth("taubin", number_of_iterations, lambda_filter, mu, filter_scope)

    def sample_points_uniformly(self, number_of_points=100, use_triangle_normal=False, seed=0):
        """-> PointCloud of number_of_points points, ordered by triangle, each triangle's share by its area; colours are interpolated
        when the mesh has them; normals are interpolated vertex normals, or with use_triangle_normal the triangle's own (computed
        first if absent, as Open3D does).  Seeded by Philox, not mt19937: the points inside a triangle differ from Open3D's."""
        if use_triangle_normal and self.has_triangles() and not self.has_triangle_normals():
            self.compute_triangle_normals(True)
        vn = self._vnrm if self.has_vertex_normals() and not use_triangle_normal else None
        tn = self._tnrm if use_triangle_normal and self.has_triangle_normals() else None
        col = self._vcol if self.has_vertex_colors() else None
        pts, c, n = ops.mesh_sample_points(self._vert, self._tri, number_of_points, seed, col, vn, tn)
        return PointCloud._make(pts, c, n)


class RaycastingScene:
    """[O3D] t.geometry.RaycastingScene on the device: ray casts, occlusion tests, intersection counts and closest points on the
    triangle meshes added to the scene (arithmetic contract AC14; kpx_rayscene_*).  Queries take arrays whose last
    dimension is 6 (rays: origin, direction; directions are not normalised, t_hit is in units of |d|) or 3 (points); leading
    dimensions are preserved.  Results are NumPy arrays in Open3D's dtypes -- the uint32 ids are the device's int32 viewed, so -1 reads
    as INVALID_ID -- or, with device=True, the device tensors of ops.rayscene_*.  The index is built on the first query and rebuilt
    after a later add_triangles, both from the copies add_triangles took: the scene answers for every geometry as it was when it was
    handed over, whatever happens to the mesh or the tensors afterwards.  Nothing works in place on a scene.
    Shape and dtype errors raise before the device is touched.
    Deviations: compute_occupancy / compute_signed_distance cast ONE ray per point (nsamples = 1 only) in the fixed direction
    (1, 0.375, 0.3125) -- marching-cubes meshes are full of axis-aligned edges, which a ray along +x would graze; a ray through an edge
    shared by two triangles counts both.  Not built: list_intersections, nsamples > 1, line sets, t.geometry tensors."""
    INVALID_ID = 0xFFFFFFFF
    OCCUPANCY_DIRECTION = (1.0, 0.375, 0.3125)

    def __init__(self):
        self._geoms = []              # (vertices, triangles): host arrays or device tensors, copies made by add_triangles
        self._scene = None

    # ---- geometries ---------------------------------------------------------------------------
    def add_triangles(self, vertex_positions, triangle_indices=None):
        """(vertex_positions float (V, 3), triangle_indices integer (T, 3)), or one TriangleMesh -> the geometry id.  The scene keeps
        a copy made here, of host arrays, of device tensors and of a mesh's arrays alike: what the caller does to them afterwards
        (TriangleMesh.transform works in place) does not reach the scene, whenever its index is built or rebuilt."""
        if isinstance(vertex_positions, TriangleMesh):
            if triangle_indices is not None:
                raise RuntimeError("RaycastingScene.add_triangles: a TriangleMesh brings its own triangles")
            pair = (vertex_positions._vert.clone(), vertex_positions._tri.clone())
        else:
            v, t = vertex_positions, triangle_indices
            if t is None:
                raise RuntimeError("RaycastingScene.add_triangles: triangle_indices is missing")
            if not (isinstance(v, torch.Tensor) and isinstance(t, torch.Tensor)):
                v, t = np.asarray(v), np.asarray(t)
                if v.dtype not in (np.float32, np.float64):
                    raise RuntimeError(f"RaycastingScene.add_triangles: vertex_positions must be float32 or float64, got {v.dtype}")
                if t.dtype.kind not in "iu":
                    raise RuntimeError(f"RaycastingScene.add_triangles: triangle_indices must be integers, got {t.dtype}")
            elif not v.dtype.is_floating_point or t.dtype.is_floating_point:
                raise RuntimeError("RaycastingScene.add_triangles: vertex_positions must be floating point, triangle_indices integers")
            if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
                raise RuntimeError(f"RaycastingScene.add_triangles: expected (V, 3) vertices and (T, 3) triangles, got {tuple(v.shape)} and {tuple(t.shape)}")
            if isinstance(v, np.ndarray):
                if t.size and (int(t.min()) < 0 or int(t.max()) >= v.shape[0]):
                    raise RuntimeError(f"RaycastingScene.add_triangles: triangle index out of range [0, {v.shape[0]})")
                with np.errstate(over="ignore"):
                    v = v.astype(np.float32)
                if not np.isfinite(v).all():
                    raise RuntimeError("RaycastingScene.add_triangles: a vertex coordinate is not finite (after rounding to float32)")
                t = t.astype(np.int32)
            else:
                v, t = v.detach().clone(), t.detach().clone()
            pair = (v, t)
        self._geoms.append(pair)
        self._scene = None
        return len(self._geoms) - 1

    def _built(self):
        if self._scene is None:
            dev = L.device()
            verts, tris, ids, base = [], [], [], 0
            for g, (v, t) in enumerate(self._geoms):
                v = ops._dev(v, torch.float32).reshape(-1, 3)
                t = ops._dev(t, torch.int32).reshape(-1, 3)
                ops._mesh_index_check("RaycastingScene", t, v.shape[0])
                verts.append(v)
                tris.append(t + base)
                ids.append(torch.stack([torch.full((t.shape[0],), g, dtype=torch.int32, device=dev),
                                        torch.arange(t.shape[0], dtype=torch.int32, device=dev)], 1))
                base += v.shape[0]
            if not verts:
                verts, tris, ids = [torch.zeros((0, 3), dtype=torch.float32, device=dev)], [torch.zeros((0, 3), dtype=torch.int32, device=dev)], \
                    [torch.zeros((0, 2), dtype=torch.int32, device=dev)]
            self._scene = ops.rayscene_build(torch.cat(verts), torch.cat(tris), torch.cat(ids))
        return self._scene

    def _n_triangles(self):
        return sum(int(t.shape[0]) for _, t in self._geoms)

    # ---- arguments ----------------------------------------------------------------------------
    @staticmethod
    def _query(who, a, width):
        """-> (array or tensor whose last dimension is `width`, its leading shape); raises on any other shape or a non-float dtype"""
        if isinstance(a, torch.Tensor):
            ok = a.dtype in (torch.float32, torch.float64)
        else:
            a = np.asarray(a)
            ok = a.dtype in (np.float32, np.float64)
        if not ok:
            raise RuntimeError(f"RaycastingScene.{who}: expected float32 or float64, got {a.dtype}")
        if a.ndim < 1 or a.shape[-1] != width:
            raise RuntimeError(f"RaycastingScene.{who}: the last dimension must be {width}, got shape {tuple(a.shape)}")
        if isinstance(a, np.ndarray):
            with np.errstate(over="ignore"):
                a = np.ascontiguousarray(a, dtype=np.float32)
        return a, tuple(a.shape[:-1])

    @staticmethod
    def _nsamples(who, nsamples):
        if int(nsamples) != 1:
            raise NotImplementedError(f"RaycastingScene.{who}: only nsamples = 1 is built")

    @staticmethod
    def _shaped(t, lead):
        return t.reshape(lead + tuple(t.shape[1:]))

    # ---- queries ------------------------------------------------------------------------------
    def cast_rays(self, rays, nthreads=0, device=False):
        """-> dict: t_hit float32 (+inf: miss), geometry_ids and primitive_ids uint32 (INVALID_ID: miss), primitive_uvs float32 (..., 2),
        primitive_normals float32 (..., 3) (zeros on a miss)"""
        rays, lead = self._query("cast_rays", rays, 6)
        out = ops.rayscene_cast(self._built(), rays)
        out = {k: self._shaped(v, lead) for k, v in out.items()}
        if device:
            return out
        res = {k: out[k].cpu().numpy() for k in ("t_hit", "geometry_ids", "primitive_ids", "primitive_uvs", "primitive_normals")}
        res["geometry_ids"], res["primitive_ids"] = res["geometry_ids"].view(np.uint32), res["primitive_ids"].view(np.uint32)
        return res

    def test_occlusions(self, rays, tnear=0.0, tfar=float("inf"), nthreads=0, device=False):
        """-> bool (...): some hit has tnear <= t <= tfar"""
        rays, lead = self._query("test_occlusions", rays, 6)
        if float(tnear) != float(tnear) or float(tfar) != float(tfar):
            raise RuntimeError("RaycastingScene.test_occlusions: tnear / tfar is not a number")
        out = self._shaped(ops.rayscene_occluded(self._built(), rays, tnear, tfar), lead)
        return out if device else out.cpu().numpy() != 0

    def count_intersections(self, rays, nthreads=0, device=False):
        """-> int32 (...): the number of triangles the ray hits; a ray through an edge that two triangles share counts both"""
        rays, lead = self._query("count_intersections", rays, 6)
        out = self._shaped(ops.rayscene_count(self._built(), rays), lead)
        return out if device else out.cpu().numpy()

    def _closest(self, who, query_points):
        q, lead = self._query(who, query_points, 3)
        if self._n_triangles() == 0:
            raise RuntimeError(f"RaycastingScene.{who}: the scene holds no triangle")
        return {k: self._shaped(v, lead) for k, v in ops.rayscene_closest(self._built(), q).items()}, q, lead

    def compute_closest_points(self, query_points, nthreads=0, device=False):
        """-> dict: points float32 (..., 3), geometry_ids and primitive_ids uint32"""
        out, _, _ = self._closest("compute_closest_points", query_points)
        if device:
            return out
        return {"points": out["points"].cpu().numpy(), "geometry_ids": out["geometry_ids"].cpu().numpy().view(np.uint32),
                "primitive_ids": out["primitive_ids"].cpu().numpy().view(np.uint32)}

    def compute_distance(self, query_points, nthreads=0, device=False):
        """-> float32 (...): the distance to the closest point of the scene"""
        out, _, _ = self._closest("compute_distance", query_points)
        return out["distance"] if device else out["distance"].cpu().numpy()

    def _occupied(self, q, lead):
        """int32 device tensor (...): 1 where the ray from q in OCCUPANCY_DIRECTION hits an odd number of triangles"""
        q = ops._dev(q, torch.float32).reshape(-1, 3)
        d = torch.tensor(self.OCCUPANCY_DIRECTION, dtype=torch.float32, device=q.device).expand(q.shape[0], 3)
        return self._shaped(ops.rayscene_count(self._built(), torch.cat([q, d], 1)) & 1, lead)

    def compute_occupancy(self, query_points, nthreads=0, nsamples=1, device=False):
        """-> float32 (...): 1 inside a closed surface, 0 outside (one ray per point, see the class's deviations)"""
        self._nsamples("compute_occupancy", nsamples)
        q, lead = self._query("compute_occupancy", query_points, 3)
        out = self._occupied(q, lead).to(torch.float32)
        return out if device else out.cpu().numpy()

    def compute_signed_distance(self, query_points, nthreads=0, nsamples=1, device=False):
        """-> float32 (...): compute_distance, negative where compute_occupancy is 1"""
        self._nsamples("compute_signed_distance", nsamples)
        out, q, lead = self._closest("compute_signed_distance", query_points)
        d = out["distance"]
        d = torch.where(self._occupied(q, lead) != 0, -d, d)
        return d if device else d.cpu().numpy()

    # ---- rays of a camera (host, fp64) ---------------------------------------------------------
    @staticmethod
    def create_rays_pinhole(*args, pixel_center=0.5, **kwargs):
        """(intrinsic_matrix 3x3, extrinsic_matrix 4x4 world -> camera, width_px, height_px), or (fov_deg, center, eye, up, width_px,
        height_px) -> float32 (H, W, 6).  Pixel (y, x): origin -(R^T t), direction R^T ((x + c - cx) / fx, (y + c - cy) / fy, 1) with
        c = pixel_center.  The default 0.5 is Open3D's; with 0.0 the ray goes through the centre of pixel (x, y) of this library's depth
        images (pixel u covers [u - 0.5, u + 0.5)), and because its camera-frame z is 1, t_hit is the depth."""
        fov = "fov_deg" in kwargs or (len(args) > 0 and np.ndim(args[0]) == 0)
        names = ("fov_deg", "center", "eye", "up", "width_px", "height_px") if fov else ("intrinsic_matrix", "extrinsic_matrix", "width_px", "height_px")
        if len(args) > len(names) or any(k not in names[len(args):] for k in kwargs) or len(args) + len(kwargs) != len(names):
            raise RuntimeError(f"RaycastingScene.create_rays_pinhole: expected {names}")
        a = dict(zip(names, args), **kwargs)
        W, H = int(a["width_px"]), int(a["height_px"])
        if W < 0 or H < 0:
            raise RuntimeError("RaycastingScene.create_rays_pinhole: negative image size")
        if fov:
            fov_deg = float(a["fov_deg"])
            if not 0.0 < fov_deg < 180.0:
                raise RuntimeError("RaycastingScene.create_rays_pinhole: fov_deg must lie in (0, 180)")
            center, eye, up = (np.asarray(a[k], dtype=np.float64).reshape(3) for k in ("center", "eye", "up"))
            fx = fy = 0.5 * W / np.tan(0.5 * np.deg2rad(fov_deg))
            cx, cy = 0.5 * W, 0.5 * H
            norm = lambda v: v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            z = norm(center - eye)
            x = norm(np.cross(z, up))
            R = np.stack([x, np.cross(z, x), z])
            t = -(R @ eye)
        else:
            K = np.asarray(a["intrinsic_matrix"], dtype=np.float64)
            E = np.asarray(a["extrinsic_matrix"], dtype=np.float64)
            if K.shape != (3, 3) or E.shape != (4, 4):
                raise RuntimeError("RaycastingScene.create_rays_pinhole: expected a 3x3 intrinsic and a 4x4 extrinsic matrix")
            fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
            R, t = E[:3, :3], E[:3, 3]
        c = float(pixel_center)
        a_ = ((np.arange(W, dtype=np.float64) + c) - cx) / fx                     # (W,)
        b_ = ((np.arange(H, dtype=np.float64) + c) - cy) / fy                     # (H,)
        rays = np.empty((H, W, 6), dtype=np.float64)
        for k in range(3):
            rays[:, :, k] = -((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2])
            rays[:, :, 3 + k] = (R[0, k] * a_[None, :] + R[1, k] * b_[:, None]) + R[2, k]
        return rays.astype(np.float32)

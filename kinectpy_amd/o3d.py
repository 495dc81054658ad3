"""Open3D-shaped namespace over the kinectpx hot path, so that KinectPy code written as
`import open3d as o3d` keeps working with `from kinectpy_amd import o3d` for the calls on the
path.  Anything off the path (visualisation)
raises NotImplementedError loudly instead of silently computing on the CPU.
"""
import types

import numpy as np

from . import ops
from .geometry import (Image, ImageFilterType, KDTreeFlann, KDTreeSearchParamHybrid, KDTreeSearchParamKNN, KDTreeSearchParamRadius, Matrix3dVector,
                       OrientedBoundingBox, PointCloud, RaycastingScene, RGBDImage, TriangleMesh, FilterScope, Vector2iVector, Vector3dVector, Vector3iVector, Voxel,
                       VoxelGrid, _off_path)
from . import integration as _integration
from . import odometry as _odometry
from . import mesh_io
from . import pcd_io
from . import posegraph


class ICPConvergenceCriteria:
    def __init__(self, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
        self.relative_fitness, self.relative_rmse, self.max_iteration = relative_fitness, relative_rmse, max_iteration


class RegistrationResult:
    def __init__(self, transformation=None, fitness=0.0, inlier_rmse=0.0, correspondence_set=None):
        self.transformation = np.eye(4) if transformation is None else transformation
        self.fitness, self.inlier_rmse = fitness, inlier_rmse
        self.correspondence_set = correspondence_set if correspondence_set is not None else np.zeros((0, 2), np.int32)

    def __repr__(self):
        return (f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, "
                f"and correspondence_set size of {len(self.correspondence_set)}")


class TransformationEstimationPointToPoint:
    mode = "p2p"

    def __init__(self, with_scaling=False):
        if with_scaling:
            raise NotImplementedError("with_scaling=True is not on the KinectPy path (registration.py:53 passes False)")
        self.with_scaling = False

    def compute_transformation(self, source, target, corres):
        """manual_pointcloud_registration.py:90-91: Umeyama/Kabsch on picked pairs"""
        return ops.kabsch(source._pts, target._pts, np.asarray(corres, dtype=np.int32))


class RobustKernel:
    """o3d.pipelines.registration.RobustKernel: `.weight(residual)` is what a residual row of the normal equations is multiplied
    with (J^T w J, J^T w r) -- the same formulas, operation by operation, as RobustLoss::weight on the device (kpx_icpdefs.h).
    `.kind` names the loss for ops (ops.LOSS_KINDS); `.k` is None for the losses without a parameter.  Open3D does not check k;
    here it must be positive."""
    kind = None
    k = None

    def weight(self, residual):
        raise NotImplementedError


class L2Loss(RobustKernel):
    """o3d.pipelines.registration.L2Loss: the plain least-squares loss (weight 1 for every residual)"""
    kind = "l2"

    def weight(self, residual):
        r = np.asarray(residual, dtype=np.float64)
        return np.ones_like(r)[()]


class L1Loss(RobustKernel):
    """w = 1 / |r|  (infinite at r == 0: such a row is left out of the normal equations, where Open3D yields NaN)"""
    kind = "l1"

    def weight(self, residual):
        r = np.asarray(residual, dtype=np.float64)
        with np.errstate(divide="ignore"):
            return (1.0 / np.abs(r))[()]


class _LossWithK(RobustKernel):
    def __init__(self, k):
        self.k = float(k)
        if not self.k > 0.0:
            raise ValueError(f"{type(self).__name__}: k must be positive")


class HuberLoss(_LossWithK):
    """w = k / max(|r|, k)"""
    kind = "huber"

    def weight(self, residual):
        r = np.asarray(residual, dtype=np.float64)
        return (self.k / np.maximum(np.abs(r), self.k))[()]


class CauchyLoss(_LossWithK):
    """w = 1 / (1 + (r / k)^2)"""
    kind = "cauchy"

    def weight(self, residual):
        q = np.asarray(residual, dtype=np.float64) / self.k
        return (1.0 / (1.0 + q * q))[()]


class GMLoss(_LossWithK):
    """Geman-McClure: w = k / (k + r^2)^2"""
    kind = "gm"

    def weight(self, residual):
        r = np.asarray(residual, dtype=np.float64)
        d = self.k + r * r
        return (self.k / (d * d))[()]


class TukeyLoss(_LossWithK):
    """w = (1 - min(1, |r| / k)^2)^2"""
    kind = "tukey"

    def weight(self, residual):
        r = np.asarray(residual, dtype=np.float64)
        q = np.minimum(1.0, np.abs(r) / self.k)
        u = 1.0 - q * q
        return (u * u)[()]


def _kernel(kernel, who, error=TypeError):
    """the `kernel` argument of an estimation: None (L2) or one of the losses above"""
    if kernel is not None and not isinstance(kernel, RobustKernel):
        raise error(f"{who}: kernel must be one of L2Loss, L1Loss, HuberLoss, CauchyLoss, GMLoss, TukeyLoss, not {kernel!r}")
    return kernel


class TransformationEstimationPointToPlane:
    mode = "p2plane"

    def __init__(self, kernel=None):
        self.kernel = _kernel(kernel, "TransformationEstimationPointToPlane")


class TransformationEstimationForColoredICP:
    mode = "colored"

    def __init__(self, lambda_geometric=0.968, kernel=None):
        self.lambda_geometric = float(lambda_geometric)
        self.kernel = _kernel(kernel, "TransformationEstimationForColoredICP")


def registration_colored_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """preprocessing/registration.py:107-113"""
    est = estimation_method if estimation_method is not None else TransformationEstimationForColoredICP()
    crit = criteria if criteria is not None else ICPConvergenceCriteria()
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    if not target.has_normals():
        raise RuntimeError("TransformationEstimationPointToPlane and TransformationEstimationColoredICP "
                           "require pre-computed normal vectors for target PointCloud.")
    if not (source.has_colors() and target.has_colors()):
        raise RuntimeError("ColoredICP requires colored point clouds.")
    r = ops.colored_icp(source._pts, source._col, target._pts, target._col, target._nrm, float(max_correspondence_distance), init,
                        est.lambda_geometric, crit.max_iteration, crit.relative_fitness, crit.relative_rmse, loss=est.kernel)
    return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], None)


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """manual_pointcloud_registration.py:96-98, preprocessing/registration.py:78-84"""
    est = estimation_method if estimation_method is not None else TransformationEstimationPointToPoint()
    crit = criteria if criteria is not None else ICPConvergenceCriteria()
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    tn = None
    if est.mode == "p2plane":
        if not target.has_normals():
            raise RuntimeError("TransformationEstimationPointToPlane and TransformationEstimationColoredICP "
                               "require pre-computed normal vectors for target PointCloud.")
        tn = target._nrm
    r = ops.icp(source._pts, target._pts, float(max_correspondence_distance), init, est.mode, tn, crit.max_iteration,
                crit.relative_fitness, crit.relative_rmse, want_corr=True, loss=getattr(est, "kernel", None))
    idx, d2 = r["idx"].cpu().numpy(), r["d2"].cpu().numpy()
    ok = d2 < float(max_correspondence_distance) ** 2
    corr = np.stack([np.flatnonzero(ok).astype(np.int32), idx[ok]], 1)
    return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], corr)


def evaluate_registration(source, target, max_correspondence_distance, transformation=None):
    """[O3D] evaluate_registration: fitness / inlier_rmse / correspondence_set of `transformation` as given (no ICP)"""
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    T = np.eye(4) if transformation is None else np.array(transformation, dtype=np.float64).reshape(4, 4)
    r = ops.registration_eval(source._pts, target._pts, float(max_correspondence_distance), T, want_corr=True)
    idx, d2 = r["idx"].cpu().numpy(), r["d2"].cpu().numpy()
    ok = d2 < float(max_correspondence_distance) ** 2
    corr = np.stack([np.flatnonzero(ok).astype(np.int32), idx[ok]], 1)
    return RegistrationResult(T, r["fitness"], r["inlier_rmse"], corr)


def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation):
    """[O3D] GetInformationMatrixFromPointClouds: sum G^T G, G = [-[t]x | I3], over the matched target points -> (6, 6) float64"""
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    return ops.registration_eval(source._pts, target._pts, float(max_correspondence_distance), transformation)["information"]


class TransformationEstimationForGeneralizedICP:
    """[O3D] plane-to-plane ICP (Segal et al.), with any of the robust kernels above"""
    mode = "gicp"

    def __init__(self, epsilon=1e-3, kernel=None):
        self.epsilon, self.kernel = float(epsilon), _kernel(kernel, "TransformationEstimationForGeneralizedICP", NotImplementedError)


def _gicp_covariances(cloud, epsilon):
    """[O3D] InitializePointCloudForGeneralizedICP, without touching `cloud`: its covariances as they are; else from its normals;
    else from normals estimated with KDTreeSearchParamKNN(20)"""
    if cloud.has_covariances():
        return cloud._cov
    nrm = cloud._nrm if cloud.has_normals() else ops.estimate_normals(cloud._pts, KDTreeSearchParamKNN(20).radius, 20)
    return ops.gicp_covariances(nrm, epsilon)


def registration_generalized_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """[O3D] registration_generalized_icp: the registration_icp loop with TransformationEstimationForGeneralizedICP as the update.
    Source and target are left as they are (covariances are built on copies, as Open3D does)."""
    est = estimation_method if estimation_method is not None else TransformationEstimationForGeneralizedICP()
    crit = criteria if criteria is not None else ICPConvergenceCriteria()
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    r = ops.generalized_icp(source._pts, _gicp_covariances(source, est.epsilon), target._pts, _gicp_covariances(target, est.epsilon),
                            float(max_correspondence_distance), init, crit.max_iteration, crit.relative_fitness, crit.relative_rmse,
                            want_corr=True, loss=est.kernel)
    idx, d2 = r["idx"].cpu().numpy(), r["d2"].cpu().numpy()
    ok = d2 < float(max_correspondence_distance) ** 2
    corr = np.stack([np.flatnonzero(ok).astype(np.int32), idx[ok]], 1)
    return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], corr)


class Feature:
    """o3d.pipelines.registration.Feature: `.data` is (33, N) float64 like Open3D's; the device copy is (N, 33)."""

    def __init__(self, dev):
        self._dev = dev

    @property
    def data(self):
        return self._dev.cpu().numpy().T.copy()

    def dimension(self):
        return 33

    def num(self):
        return int(self._dev.shape[0])

    def select_by_index(self, indices, invert=False):
        """[O3D] Feature.select_by_index: the columns of `.data` named by `indices` (duplicates once, ascending -- Open3D selects
        through a mask), or every other column with invert=True; an index outside [0, num) raises"""
        import torch
        n = self.num()
        idx = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices).reshape(-1).astype(np.int64))
        idx = idx.reshape(-1).to(device=self._dev.device, dtype=torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise RuntimeError(f"Feature.select_by_index: index out of range [0, {n})")
        mask = torch.zeros(n, dtype=torch.bool, device=self._dev.device)
        mask[idx] = True
        return Feature(self._dev[~mask if invert else mask].contiguous())


class CorrespondenceCheckerBasedOnEdgeLength:
    def __init__(self, similarity_threshold=0.9):
        self.similarity_threshold = float(similarity_threshold)


class CorrespondenceCheckerBasedOnDistance:
    def __init__(self, distance_threshold):
        self.distance_threshold = float(distance_threshold)


class RANSACConvergenceCriteria:
    def __init__(self, max_iteration=100000, confidence=0.999):
        self.max_iteration, self.confidence = int(max_iteration), float(confidence)


def compute_fpfh_feature(input, search_param):
    """preprocessing/registration.py:15-20"""
    if not input.has_normals():
        raise RuntimeError("Failed because input point cloud has no normal.")
    return Feature(ops.fpfh(input._pts, input._nrm, search_param.radius, search_param.max_nn))


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                                  max_correspondence_distance, estimation_method=None, ransac_n=3,
                                                  checkers=(), criteria=None, seed=None):
    """preprocessing/registration.py:50-57.  Open3D's RANSAC is unseeded and runs its iterations in an OpenMP
    loop; ours draws from Philox with `seed` (None -> fresh random seed) and replays the iterations in order."""
    crit, edge, seed = _ransac_arguments(max_correspondence_distance, estimation_method, checkers, criteria, seed)
    # the correspondences depend only on the two feature sets: execute_global_registration calls this 15 times with the
    # same features (registration.py:46-57), so they are computed once and kept on the source Feature
    key = (id(target_feature), bool(mutual_filter), int(ransac_n))
    cached = getattr(source_feature, "_corr_cache", None)
    if cached is not None and cached[0] == key and cached[2] is target_feature:
        corres = cached[1]
    else:
        corres = ops.feature_correspondences(source_feature._dev, target_feature._dev, bool(mutual_filter), int(ransac_n))
        source_feature._corr_cache = (key, corres, target_feature)
    r = ops.ransac_corres(source._pts, target._pts, corres, float(max_correspondence_distance), int(ransac_n), edge,
                          crit.max_iteration, crit.confidence, seed)
    return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], corres)


def _ransac_arguments(max_correspondence_distance, estimation_method, checkers, criteria, seed):
    """the restrictions the two RANSAC entry points share -> (criteria, edge similarity, seed)"""
    crit = criteria if criteria is not None else RANSACConvergenceCriteria()
    est = estimation_method if estimation_method is not None else TransformationEstimationPointToPoint()
    if est.mode != "p2p":
        raise NotImplementedError("feature-matching RANSAC is used with TransformationEstimationPointToPoint(False) by KinectPy")
    edge, dist_thr = 0.0, float(max_correspondence_distance)
    for c in checkers:
        if isinstance(c, CorrespondenceCheckerBasedOnEdgeLength):
            edge = c.similarity_threshold
        elif isinstance(c, CorrespondenceCheckerBasedOnDistance):
            dist_thr = c.distance_threshold
    if dist_thr != float(max_correspondence_distance):
        raise NotImplementedError("distance checker threshold must equal max_correspondence_distance (as in KinectPy)")
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    return crit, edge, seed


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, estimation_method=None, ransac_n=3,
                                                checkers=(), criteria=None, seed=None):
    """[O3D] registration_ransac_based_on_correspondence: the RANSAC of the feature variant over the correspondences as given
    ((C, 2) source / target indices), with the same restrictions and the same `seed` keyword.  `correspondence_set` is, as in
    Open3D, the evaluation's: every source point with a target point within max_correspondence_distance under the result."""
    crit, edge, seed = _ransac_arguments(max_correspondence_distance, estimation_method, checkers, criteria, seed)
    corres = np.ascontiguousarray(np.asarray(corres, dtype=np.int32).reshape(-1, 2))
    r = ops.ransac_corres(source._pts, target._pts, corres, float(max_correspondence_distance), int(ransac_n), edge,
                          crit.max_iteration, crit.confidence, seed)
    if not max_correspondence_distance > 0:
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"])
    inliers = evaluate_registration(source, target, max_correspondence_distance, r["transformation"]).correspondence_set
    return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], inliers)


class FastGlobalRegistrationOption:
    """[O3D] FastGlobalRegistrationOption, Open3D's defaults"""

    def __init__(self, division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
                 iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, tuple_test=True):
        self.division_factor, self.use_absolute_scale, self.decrease_mu = float(division_factor), bool(use_absolute_scale), bool(decrease_mu)
        self.maximum_correspondence_distance, self.iteration_number = float(maximum_correspondence_distance), int(iteration_number)
        self.tuple_scale, self.maximum_tuple_count, self.tuple_test = float(tuple_scale), int(maximum_tuple_count), bool(tuple_test)

    def __repr__(self):
        return ("FastGlobalRegistrationOption(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in (
            "division_factor", "use_absolute_scale", "decrease_mu", "maximum_correspondence_distance", "iteration_number", "tuple_scale",
            "maximum_tuple_count", "tuple_test")) + ")")


def _fgr_result(source, target, corres, opt):
    """optimise over `corres`, then Open3D's evaluation of the result at maximum_correspondence_distance"""
    if opt.maximum_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    r = ops.fgr_optimize(source._pts, target._pts, corres, opt.division_factor, opt.use_absolute_scale, opt.decrease_mu,
                         opt.maximum_correspondence_distance, opt.iteration_number)
    return evaluate_registration(source, target, opt.maximum_correspondence_distance, r["transformation"])


def registration_fgr_based_on_correspondence(source, target, corres, option=None):
    """[O3D] registration_fgr_based_on_correspondence: Fast Global Registration over the correspondences as given ((C, 2) source /
    target indices); no tuple test, as in Open3D."""
    opt = option if option is not None else FastGlobalRegistrationOption()
    return _fgr_result(source, target, np.ascontiguousarray(np.asarray(corres, dtype=np.int32).reshape(-1, 2)), opt)


def registration_fgr_based_on_feature_matching(source, target, source_feature, target_feature, option=None, seed=None):
    """[O3D] registration_fgr_based_on_feature_matching: mutual nearest neighbours of the features (no one-way fall-back), the tuple
    test, then the optimisation.  Open3D draws the tuple test's triples from rand() seeded by the clock; ours draws from Philox
    with `seed` (None -> fresh random seed)."""
    opt = option if option is not None else FastGlobalRegistrationOption()
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    corres = ops.feature_correspondences(source_feature._dev, target_feature._dev, True, ransac_n=0)
    if opt.tuple_test and len(corres):
        corres = ops.fgr_tuple_test(source._pts, target._pts, corres, opt.tuple_scale, opt.maximum_tuple_count, seed)
    return _fgr_result(source, target, corres, opt)


def compute_iss_keypoints(input, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """[O3D] geometry.keypoint.compute_iss_keypoints (Zhong 2009): the points whose neighbourhood covariance has three well
    separated eigenvalues and whose smallest eigenvalue is a maximum within non_max_radius, as a PointCloud (colours and normals
    follow) in ascending order of their index in `input` -- Open3D's order is whatever its OpenMP loop produced.  Either radius 0:
    both are taken from the cloud's resolution (6 x and 4 x the mean nearest-neighbour distance)."""
    if not input.has_points():
        return PointCloud()
    return input._select(input._iss_keypoint_indices(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors))


class PinholeCameraIntrinsic:
    """[O3D] camera.PinholeCameraIntrinsic(width, height, fx, fy, cx, cy) (or (width, height, intrinsic_matrix))"""

    def __init__(self, width=-1, height=-1, fx=None, fy=None, cx=None, cy=None):
        self.width, self.height = int(width), int(height)
        if fx is not None and np.ndim(fx) == 2:
            self.intrinsic_matrix = np.array(fx, dtype=np.float64).reshape(3, 3)
        else:
            self.intrinsic_matrix = np.eye(3)
            if fx is not None:
                self.set_intrinsics(width, height, fx, fy, cx, cy)

    def set_intrinsics(self, width, height, fx, fy, cx, cy):
        self.width, self.height = int(width), int(height)
        self.intrinsic_matrix = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)

    def get_focal_length(self):
        return float(self.intrinsic_matrix[0, 0]), float(self.intrinsic_matrix[1, 1])

    def get_principal_point(self):
        return float(self.intrinsic_matrix[0, 2]), float(self.intrinsic_matrix[1, 2])

    def get_skew(self):
        return float(self.intrinsic_matrix[0, 1])

    def is_valid(self):
        return self.width > 0 and self.height > 0

    def __repr__(self):
        return f"PinholeCameraIntrinsic with width = {self.width} and height = {self.height}.\nAccess intrinsics with intrinsic_matrix."


class PinholeCameraParameters:
    """[O3D] camera.PinholeCameraParameters: `intrinsic` (PinholeCameraIntrinsic) and `extrinsic` (4x4 float64, world -> camera)"""

    def __init__(self, intrinsic=None, extrinsic=None):
        self.intrinsic = PinholeCameraIntrinsic() if intrinsic is None else intrinsic
        self.extrinsic = np.eye(4) if extrinsic is None else extrinsic

    extrinsic = property(lambda self: self._extrinsic)

    @extrinsic.setter
    def extrinsic(self, E):
        E = np.array(E, dtype=np.float64)
        if E.shape != (4, 4):
            raise RuntimeError("PinholeCameraParameters: extrinsic must be a 4x4 matrix")
        self._extrinsic = E

    def __repr__(self):
        return "PinholeCameraParameters class.\nAccess its data via intrinsic and extrinsic."


geometry = types.SimpleNamespace(PointCloud=PointCloud, OrientedBoundingBox=OrientedBoundingBox, KDTreeSearchParamHybrid=KDTreeSearchParamHybrid,
                                 KDTreeSearchParamKNN=KDTreeSearchParamKNN, KDTreeSearchParamRadius=KDTreeSearchParamRadius, KDTreeFlann=KDTreeFlann,
                                 Image=Image, ImageFilterType=ImageFilterType, RGBDImage=RGBDImage, Voxel=Voxel, VoxelGrid=VoxelGrid,
                                 TriangleMesh=TriangleMesh, FilterScope=FilterScope,
                                 keypoint=types.SimpleNamespace(compute_iss_keypoints=compute_iss_keypoints))
# [O3D] o3d.t.geometry: only the mesh-query class; it takes NumPy arrays (or a legacy TriangleMesh), not t.geometry tensors
t = types.SimpleNamespace(geometry=types.SimpleNamespace(RaycastingScene=RaycastingScene))
camera = types.SimpleNamespace(PinholeCameraIntrinsic=PinholeCameraIntrinsic, PinholeCameraParameters=PinholeCameraParameters)
utility = types.SimpleNamespace(Vector3dVector=Vector3dVector, Vector2iVector=Vector2iVector, Vector3iVector=Vector3iVector,
                                Matrix3dVector=Matrix3dVector)
io = types.SimpleNamespace(read_point_cloud=pcd_io.read_point_cloud, write_point_cloud=pcd_io.write_point_cloud,
                           read_triangle_mesh=mesh_io.read_triangle_mesh, write_triangle_mesh=mesh_io.write_triangle_mesh)
pipelines = types.SimpleNamespace(integration=types.SimpleNamespace(
    TSDFVolumeColorType=_integration.TSDFVolumeColorType,
    UniformTSDFVolume=_integration.UniformTSDFVolume,
    ScalableTSDFVolume=_integration.ScalableTSDFVolume,
), odometry=types.SimpleNamespace(
    OdometryOption=_odometry.OdometryOption,
    RGBDOdometryJacobian=_odometry.RGBDOdometryJacobian,
    RGBDOdometryJacobianFromColorTerm=_odometry.RGBDOdometryJacobianFromColorTerm,
    RGBDOdometryJacobianFromHybridTerm=_odometry.RGBDOdometryJacobianFromHybridTerm,
    compute_rgbd_odometry=_odometry.compute_rgbd_odometry,
    compute_rgbd_odometry_batch=_odometry.compute_rgbd_odometry_batch,
    compute_correspondence=_odometry.compute_correspondence,
), registration=types.SimpleNamespace(
    registration_icp=registration_icp,
    ICPConvergenceCriteria=ICPConvergenceCriteria,
    RegistrationResult=RegistrationResult,
    TransformationEstimationPointToPoint=TransformationEstimationPointToPoint,
    TransformationEstimationPointToPlane=TransformationEstimationPointToPlane,
    compute_fpfh_feature=compute_fpfh_feature,
    registration_ransac_based_on_feature_matching=registration_ransac_based_on_feature_matching,
    registration_ransac_based_on_correspondence=registration_ransac_based_on_correspondence,
    FastGlobalRegistrationOption=FastGlobalRegistrationOption,
    registration_fgr_based_on_feature_matching=registration_fgr_based_on_feature_matching,
    registration_fgr_based_on_correspondence=registration_fgr_based_on_correspondence,
    Feature=Feature,
    CorrespondenceCheckerBasedOnEdgeLength=CorrespondenceCheckerBasedOnEdgeLength,
    CorrespondenceCheckerBasedOnDistance=CorrespondenceCheckerBasedOnDistance,
    RANSACConvergenceCriteria=RANSACConvergenceCriteria,
    registration_colored_icp=registration_colored_icp,
    TransformationEstimationForColoredICP=TransformationEstimationForColoredICP,
    registration_generalized_icp=registration_generalized_icp,
    RobustKernel=RobustKernel,
    L2Loss=L2Loss,
    L1Loss=L1Loss,
    HuberLoss=HuberLoss,
    CauchyLoss=CauchyLoss,
    GMLoss=GMLoss,
    TukeyLoss=TukeyLoss,
    TransformationEstimationForGeneralizedICP=TransformationEstimationForGeneralizedICP,
    evaluate_registration=evaluate_registration,
    get_information_matrix_from_point_clouds=get_information_matrix_from_point_clouds,
    PoseGraphNode=posegraph.PoseGraphNode,
    PoseGraphEdge=posegraph.PoseGraphEdge,
    PoseGraph=posegraph.PoseGraph,
    GlobalOptimizationConvergenceCriteria=posegraph.GlobalOptimizationConvergenceCriteria,
    GlobalOptimizationOption=posegraph.GlobalOptimizationOption,
    GlobalOptimizationLevenbergMarquardt=posegraph.GlobalOptimizationLevenbergMarquardt,
    GlobalOptimizationGaussNewton=posegraph.GlobalOptimizationGaussNewton,
    global_optimization=posegraph.global_optimization,
))
visualization = types.SimpleNamespace(VisualizerWithEditing=_off_path("VisualizerWithEditing"),
                                      draw_geometries=_off_path("draw_geometries"))

"""[O3D] pipelines.odometry: RGB-D odometry between two frames of ONE sensor (Steinbruecker 2011 colour term, Park 2017 hybrid term),
arithmetic contract AC11 of DESIGN.md.  The whole multiscale chain and the information matrix run on the device in one chain of
launches (kpx_rgbd_odometry); the host reads (success, transformation, information) once.  Values are in data units: a rig that
records millimetres passes e.g. OdometryOption(depth_diff_max=30, depth_min=0, depth_max=4000)."""
import numpy as np

from . import ops
from .geometry import _pinhole


class OdometryOption:
    """[O3D] OdometryOption; iteration_number_per_pyramid_level[0] belongs to the coarsest level.  The older names max_depth_diff,
    min_depth and max_depth are accepted and exposed as well."""

    def __init__(self, iteration_number_per_pyramid_level=None, depth_diff_max=None, depth_min=None, depth_max=None, *, max_depth_diff=None,
                 min_depth=None, max_depth=None):
        def pick(new, old, default, name):
            if new is not None and old is not None:
                raise TypeError(f"OdometryOption: {name} given under both of its names")
            return float(default if new is None and old is None else (new if new is not None else old))
        its = [20, 10, 5] if iteration_number_per_pyramid_level is None else [int(i) for i in iteration_number_per_pyramid_level]
        if not 1 <= len(its) <= ops.ODOMETRY_MAX_LEVELS or any(i < 0 for i in its):
            raise RuntimeError(f"OdometryOption: 1 to {ops.ODOMETRY_MAX_LEVELS} pyramid levels with iteration counts >= 0")
        self.iteration_number_per_pyramid_level = its
        self.depth_diff_max = pick(depth_diff_max, max_depth_diff, 0.03, "depth_diff_max")
        self.depth_min = pick(depth_min, min_depth, 0.0, "depth_min")
        self.depth_max = pick(depth_max, max_depth, 4.0, "depth_max")

    max_depth_diff = property(lambda self: self.depth_diff_max, lambda self, v: setattr(self, "depth_diff_max", float(v)))
    min_depth = property(lambda self: self.depth_min, lambda self, v: setattr(self, "depth_min", float(v)))
    max_depth = property(lambda self: self.depth_max, lambda self, v: setattr(self, "depth_max", float(v)))

    def __repr__(self):
        return (f"OdometryOption class.\niteration_number_per_pyramid_level = {self.iteration_number_per_pyramid_level}\n"
                f"depth_diff_max = {self.depth_diff_max:g}\ndepth_min = {self.depth_min:g}\ndepth_max = {self.depth_max:g}")


class RGBDOdometryJacobian:
    kind = None

    def __repr__(self):
        return type(self).__name__


class RGBDOdometryJacobianFromColorTerm(RGBDOdometryJacobian):
    """photo-consistency rows only (Steinbruecker, Sturm, Cremers 2011)"""
    kind = "color"


class RGBDOdometryJacobianFromHybridTerm(RGBDOdometryJacobian):
    """photo-consistency and depth rows, weights sqrt(1 - 0.968) and sqrt(0.968) (Park, Zhou, Koltun 2017)"""
    kind = "hybrid"


def _jacobian_kind(jacobian):
    jacobian = RGBDOdometryJacobianFromHybridTerm() if jacobian is None else jacobian
    if getattr(jacobian, "kind", None) not in ops.ODOMETRY_JACOBIANS:
        raise TypeError("odometry: jacobian must be RGBDOdometryJacobianFromColorTerm() or RGBDOdometryJacobianFromHybridTerm()")
    return jacobian.kind


def _failed():
    return False, np.eye(4), np.eye(6)


def _pair_ok(source, target, width, height):
    """[O3D] CheckRGBDImagePair: float32 single-channel intensity and float32 depth, all of the intrinsic's size"""
    for im in (source.color, source.depth, target.color, target.depth):
        a = np.asarray(im)
        if a.dtype != np.float32 or a.ndim != 2 or a.shape != (height, width) or a.size == 0:
            return False
    return True


def compute_rgbd_odometry(rgbd_source, rgbd_target, pinhole_camera_intrinsic, odo_init=None, jacobian=None, option=None):
    """[O3D] compute_rgbd_odometry -> (success, transformation (4, 4) float64 source -> target camera, information (6, 6) float64).
    Images that are not float32 intensity + float32 depth of the intrinsic's size, and a solve that fails (no correspondence or a
    singular system in any iteration), give (False, identity, identity)."""
    option = OdometryOption() if option is None else option
    kind = _jacobian_kind(jacobian)
    width, height, K = _pinhole(pinhole_camera_intrinsic)
    T0 = np.eye(4) if odo_init is None else np.asarray(odo_init, dtype=np.float64)
    if T0.shape != (4, 4):
        raise RuntimeError("compute_rgbd_odometry: odo_init must be a 4x4 matrix")
    if not _pair_ok(rgbd_source, rgbd_target, width, height):
        return _failed()
    ok, T, info, _ = ops.rgbd_odometry(np.asarray(rgbd_source.depth)[None], np.asarray(rgbd_source.color)[None], np.asarray(rgbd_target.depth)[None],
                                       np.asarray(rgbd_target.color)[None], width, height, K, T0[None], kind, option.iteration_number_per_pyramid_level,
                                       option.depth_diff_max, option.depth_min, option.depth_max)
    return (True, T[0], info[0]) if ok[0] else _failed()


def compute_rgbd_odometry_batch(depths_s, colors_s, depths_t, colors_t, intrinsic, odo_inits=None, jacobian=None, option=None, depth_scale=1000.0,
                                depth_trunc=3.0, masks_s=None, masks_t=None):
    """Extension: P pairs of RAW frames in one chain of launches (pair = grid.y).  depths_*: uint16 (P, H W) or (P, H, W); colors_*:
    uint8 (P, H W, 3) or (P, H, W, 3); host arrays or device tensors.  The RGBDImage.create_from_color_and_depth conversion
    (depth_scale, depth_trunc, rgb -> intensity) is done in the kernel, bit-identical to the host path; masks_* (uint8 / bool (P, H W),
    optional): a nonzero pixel loses its depth.  -> (success bool (P,), transformation (P, 4, 4), information (P, 6, 6)), each pair
    bit-identical to its own compute_rgbd_odometry call; a failed pair holds the identities."""
    option = OdometryOption() if option is None else option
    kind = _jacobian_kind(jacobian)
    width, height, K = _pinhole(intrinsic)
    ok, T, info, _ = ops.rgbd_odometry(depths_s, colors_s, depths_t, colors_t, width, height, K, odo_inits, kind, option.iteration_number_per_pyramid_level,
                                       option.depth_diff_max, option.depth_min, option.depth_max, raw=True, depth_scale=depth_scale,
                                       depth_trunc=depth_trunc, mask_s=masks_s, mask_t=masks_t)
    return ok, T, info


def compute_correspondence(intrinsic_matrix, extrinsic, depth_s, depth_t, option=None):
    """[O3D] ComputeCorrespondence (exposed by newer Open3D): int32 (n, 4) rows (u_s, v_s, u_t, v_t), ascending in (v_t, u_t), of two
    float32 depth images whose missing measurements are NaN.  Several source pixels on one target pixel: the smallest float32 z'
    wins, equal ones the smallest source index."""
    option = OdometryOption() if option is None else option
    return ops.odometry_correspondence(np.asarray(depth_s), np.asarray(depth_t), np.asarray(intrinsic_matrix, dtype=np.float64), extrinsic,
                                       option.depth_diff_max).cpu().numpy()

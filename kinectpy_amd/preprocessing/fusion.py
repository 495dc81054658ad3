"""Volumetric fusion of one frame set: every sensor's depth image integrated into one TSDF volume in the master's frame with the
calibrated sensor -> master transforms, then the surface cloud extracted (o3d.pipelines.integration on the rig's own arrays).  An
alternative to DataProcessor's transform + vstack + voxel_down_sample + remove_statistical_outlier fuse; the frame step is
unchanged.  remove_free_space_points is the rig's space-carving filter: it drops the points of a fused cloud that lie where some
sensor sees through (flying pixels), which the density filters keep."""
import numpy as np
import torch

from ..geometry import RaycastingScene, VoxelGrid
from ..integration import ScalableTSDFVolume, TSDFVolumeColorType, UniformTSDFVolume
from ..utils import synth


class _Intrinsic:
    def __init__(self, width, height, fx, fy, cx, cy):
        self.width, self.height = int(width), int(height)
        self.intrinsic_matrix = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _undistorted_frames(who, rig, depth, rgb, intrinsic):
    """the frames of a rig of distorted lenses as its common pinhole camera sees them -> depth (S, H' W'), rgb (S, H' W', 3) or None,
    the PinholeCameraIntrinsic"""
    if intrinsic is not None:
        raise ValueError(f"{who}: give either intrinsic (pinhole frames) or rig (frames as the lenses took them), not both")
    target = rig.common_pinhole()
    n = int(depth.shape[0])
    depth = rig.undistort_depths(depth, pinhole=target).reshape(n, -1)
    if rgb is not None:
        rgb = rig.undistort_colors(rgb, pinhole=target, camera="depth", interpolation="nearest").reshape(n, -1, 3)
    return depth, rgb, target.to_pinhole()


def fuse_depth_tsdf(depth, rgb, intrinsic, sensor_to_master, length, resolution, origin, sdf_trunc=None, depth_scale=1.0, depth_trunc=6000.0, mesh=False,
                    min_cluster_triangles=0, taubin_iterations=0, scalable=False, volume_unit_resolution=16, depth_sampling_stride=4, rig=None):
    """depth: uint16 (S, H W) raw frames (synth.sensor_ring's layout; host or device); rgb: uint8 (S, H W, 3) or None (no colours);
    intrinsic: a PinholeCameraIntrinsic, or None for the Kinect's (synth.FX, FY, CX, CY at synth.W x synth.H); sensor_to_master:
    the S - 1 transforms of the sub sensors (sensor 0 is the master, identity).  The world frame is the master's: sensor s is
    integrated with the extrinsic inv(sensor_to_master[s]) (host float64).  sdf_trunc defaults to 4 voxels.  One integrate_frames
    call and one extraction -> PointCloud with normals (and colours when rgb is given); mesh=True: the surface as a TriangleMesh
    (extract_triangle_mesh) with vertex normals computed instead.  The mesh's clean-up, both off by default: min_cluster_triangles > 0
    drops every connected component of fewer triangles (the specks flying pixels leave) and then the vertices nothing names;
    taubin_iterations > 0 smooths with filter_smooth_taubin's defaults before the normals are computed.  scalable=True: a
    ScalableTSDFVolume of voxel length `length / resolution` with volume_unit_resolution and depth_sampling_stride instead of the
    uniform volume; `origin` is not used (the blocks sit on the world lattice); everything after the volume is the same.
    rig: a calibration.SensorRig of the S sensors for frames as the lenses took them (`intrinsic` must then be None): depth, and rgb
    already registered into the depth grid (SensorRig.register_colors), are undistorted to rig.common_pinhole() first, both with
    nearest sampling -- depth values are copied, and bilinear would blend the registered colours' zero holes."""
    if rig is not None:
        depth, rgb, intrinsic = _undistorted_frames("fuse_depth_tsdf", rig, depth, rgb, intrinsic)
    if intrinsic is None:
        intrinsic = _Intrinsic(synth.W, synth.H, synth.FX, synth.FY, synth.CX, synth.CY)
    n = int(depth.shape[0])
    if len(sensor_to_master) != n - 1:
        raise RuntimeError(f"fuse_depth_tsdf: {n} sensors need {n - 1} sensor -> master transforms, got {len(sensor_to_master)}")
    extr = [np.eye(4)] + [np.linalg.inv(np.asarray(T, dtype=np.float64).reshape(4, 4)) for T in sensor_to_master]
    if sdf_trunc is None:
        sdf_trunc = 4.0 * float(length) / int(resolution)
    color_type = TSDFVolumeColorType.RGB8 if rgb is not None else TSDFVolumeColorType.NoColor
    if scalable:
        vol = ScalableTSDFVolume(float(length) / int(resolution), sdf_trunc, color_type, volume_unit_resolution, depth_sampling_stride)
    else:
        vol = UniformTSDFVolume(length, resolution, sdf_trunc, color_type, origin)
    vol.integrate_frames(depth, rgb, intrinsic, np.stack(extr), depth_scale, depth_trunc)
    if mesh:
        m = vol.extract_triangle_mesh()
        if min_cluster_triangles > 0 and m.has_triangles():
            cluster, n_triangles, _ = m.cluster_connected_triangles()
            m.remove_triangles_by_mask(n_triangles[cluster.long()] < int(min_cluster_triangles)).remove_unreferenced_vertices()
        if taubin_iterations > 0:
            m = m.filter_smooth_taubin(int(taubin_iterations))
        return m.compute_vertex_normals()
    return vol.extract_point_cloud()


def remove_free_space_points(pcd, depth, intrinsic, sensor_to_master, voxel_size, keep_unmeasured=True, depth_scale=1.0, depth_trunc=6000.0, rig=None):
    """pcd: the fused cloud in the master's frame; depth, intrinsic, sensor_to_master, depth_scale, depth_trunc as in fuse_depth_tsdf.
    The cloud's VoxelGrid (voxel_size) is carved by every sensor's depth map in one pass (carve_depth_maps with
    keep_voxels_outside_image=True: a sensor that does not see a voxel says nothing about it); a point is kept when its voxel
    survived.  keep_unmeasured=True: a pixel without depth is no evidence of free space (Open3D's rule, False, carves its whole
    ray).  rig: as in fuse_depth_tsdf (the depth frames as the lenses took them, `intrinsic` None).
    -> (PointCloud of the kept points, their indices in pcd: ascending int32 device tensor)"""
    if rig is not None:
        depth, _, intrinsic = _undistorted_frames("remove_free_space_points", rig, depth, None, intrinsic)
    if intrinsic is None:
        intrinsic = _Intrinsic(synth.W, synth.H, synth.FX, synth.FY, synth.CX, synth.CY)
    n = int(depth.shape[0])
    if len(sensor_to_master) != n - 1:
        raise RuntimeError(f"remove_free_space_points: {n} sensors need {n - 1} sensor -> master transforms, got {len(sensor_to_master)}")
    extr = [np.eye(4)] + [np.linalg.inv(np.asarray(T, dtype=np.float64).reshape(4, 4)) for T in sensor_to_master]
    grid = VoxelGrid.create_from_point_cloud(pcd, voxel_size)
    grid.carve_depth_maps(depth, intrinsic, np.stack(extr), True, depth_scale, depth_trunc, keep_unmeasured)
    kept = torch.nonzero(grid.included_mask(pcd)).reshape(-1).to(torch.int32)
    if not pcd.has_points() or kept.numel() == 0:
        return type(pcd)(), kept
    return pcd._select(kept), kept


def render_mesh_depth(mesh, intrinsic, sensor_to_master, width=None, height=None):
    """the depth images the sensors of fuse_depth_tsdf would take of `mesh` (a TriangleMesh in the master's frame): intrinsic and
    sensor_to_master as there (sensor 0 is the master), width x height default to the intrinsic's.  All sensors' rays go through one
    RaycastingScene.cast_rays: pixel (y, x) of sensor s casts the ray through its centre (create_rays_pinhole with pixel_center=0.0
    and the extrinsic inv(sensor_to_master[s])), whose camera-frame z is 1, so t_hit is the depth along the optical axis -- in the
    mesh's unit, not divided by a depth scale.  -> float32 (S, H, W) host array, 0 where the ray misses, as in a depth image."""
    if intrinsic is None:
        intrinsic = _Intrinsic(synth.W, synth.H, synth.FX, synth.FY, synth.CX, synth.CY)
    W = int(intrinsic.width if width is None else width)
    H = int(intrinsic.height if height is None else height)
    if W <= 0 or H <= 0:
        raise RuntimeError(f"render_mesh_depth: bad image size {W} x {H}")
    extr = [np.eye(4)] + [np.linalg.inv(np.asarray(T, dtype=np.float64).reshape(4, 4)) for T in sensor_to_master]
    rays = np.stack([RaycastingScene.create_rays_pinhole(intrinsic.intrinsic_matrix, E, W, H, pixel_center=0.0) for E in extr])
    scene = RaycastingScene()
    scene.add_triangles(mesh)
    t = scene.cast_rays(rays)["t_hit"]
    return np.where(np.isfinite(t), t, np.float32(0.0)).astype(np.float32)


def orient_normals_to_sensors(pcds, sensor_to_master):
    """pcds: one PointCloud with normals per sensor, each already in the master's frame (sensor 0 is the master); sensor_to_master
    as in fuse_depth_tsdf (the S - 1 transforms of the sub sensors; S transforms, the master's first, are accepted too).  Every
    cloud's normals are oriented, in place, towards its own sensor's centre T[:3, 3] (orient_normals_towards_camera_location) --
    before the clouds are fused and the sensor of origin is lost.  -> pcds"""
    n = len(pcds)
    Ts = [np.asarray(T, dtype=np.float64).reshape(4, 4) for T in sensor_to_master]
    if len(Ts) == n - 1:
        Ts = [np.eye(4)] + Ts
    if len(Ts) != n:
        raise RuntimeError(f"orient_normals_to_sensors: {n} sensors need {n - 1} sensor -> master transforms, got {len(sensor_to_master)}")
    for pcd, T in zip(pcds, Ts):
        pcd.orient_normals_towards_camera_location(T[:3, 3])
    return pcds

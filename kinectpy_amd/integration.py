"""o3d.pipelines.integration over the kinectpx hot path: a uniform truncated-signed-distance volume in device memory that depth
images are integrated into (kpx_tsdf_integrate, arithmetic contract AC9 of DESIGN.md) and surface clouds are extracted from.
The batch form `integrate_frames` takes the rig's uint16 depth frames as they are and updates the volume for all of them in one
pass; extract_triangle_mesh is marching cubes over the same volume (AC12).  The hashed ScalableTSDFVolume is off the path and raises."""
import enum

import numpy as np
import torch

from . import _lib as L
from . import ops
from .geometry import PointCloud, TriangleMesh


class TSDFVolumeColorType(enum.Enum):
    NoColor = 0
    RGB8 = 1
    Gray32 = 2


def _intrinsic4(intrinsic):
    """PinholeCameraIntrinsic-like (width, height, intrinsic_matrix) -> (width, height, (fx, fy, cx, cy))"""
    K = np.asarray(intrinsic.intrinsic_matrix, dtype=np.float64)
    return int(intrinsic.width), int(intrinsic.height), (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


class UniformTSDFVolume:
    """[O3D] UniformTSDFVolume(length, resolution, sdf_trunc, color_type, origin): resolution^3 voxels of length / resolution,
    voxel (x, y, z) centred at origin + (index + 0.5) voxel_length.  `_vol` is the float32 (resolution^3, 2) {tsdf, weight} device
    tensor, `_col` the float32 (resolution^3, 3) colours of an RGB8 volume."""

    def __init__(self, length, resolution, sdf_trunc, color_type, origin=(0.0, 0.0, 0.0)):
        color_type = TSDFVolumeColorType(color_type)
        if color_type is TSDFVolumeColorType.Gray32:
            raise NotImplementedError("UniformTSDFVolume: Gray32 volumes are not built (NoColor and RGB8 are)")
        self.length, self.resolution, self.sdf_trunc, self.color_type = float(length), int(resolution), float(sdf_trunc), color_type
        if not (1 <= self.resolution <= 1024) or not self.length > 0.0 or not self.sdf_trunc > 0.0:
            raise RuntimeError("UniformTSDFVolume: resolution must be in [1, 1024], length and sdf_trunc positive")
        self.voxel_length = self.length / self.resolution
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3).copy()
        n = self.resolution ** 3
        self._vol = torch.zeros((n, 2), dtype=torch.float32, device=L.device())
        self._col = torch.zeros((n, 3), dtype=torch.float32, device=L.device()) if color_type is TSDFVolumeColorType.RGB8 else None

    def reset(self):
        ops.tsdf_reset(self._vol, self._col)

    def _integrate(self, depths, colors, width, height, K, extrinsics, depth_scale=1.0, depth_trunc=0.0):
        ops.tsdf_integrate(self._vol, self._col, self.resolution, self.voxel_length, self.origin, self.sdf_trunc, depths,
                           colors if self._col is not None else None, width, height, K, extrinsics, depth_scale, depth_trunc)

    def integrate(self, image, intrinsic, extrinsic):
        """[O3D] integrate(RGBDImage, PinholeCameraIntrinsic, extrinsic world -> camera)"""
        width, height, K = _intrinsic4(intrinsic)
        depth, color = np.asarray(image.depth), np.asarray(image.color)
        bad = depth.ndim != 2 or depth.dtype != np.float32 or depth.shape != (height, width)
        if self._col is not None:
            bad = bad or color.ndim != 3 or color.dtype != np.uint8 or color.shape[:2] != (height, width)
        elif color.size:
            bad = bad or color.shape[:2] != (height, width)
        if bad:
            raise RuntimeError("[UniformTSDFVolume::Integrate] Unsupported image format.")
        dev = self._vol.device
        self._integrate([torch.as_tensor(depth).to(dev)], [torch.as_tensor(color).to(dev)] if self._col is not None else None, width, height, K,
                        np.asarray(extrinsic, dtype=np.float64).reshape(1, 4, 4))

    def integrate_frames(self, depths, colors, intrinsic, extrinsics, depth_scale=1000.0, depth_trunc=3.0):
        """The batch form: S raw uint16 depth frames ((S, H W) or (S, H, W), host or device), their uint8 colours ((S, H W, 3);
        None for a NoColor volume) and S extrinsics, integrated in ascending order in one pass over the volume; depth_scale and
        depth_trunc as in RGBDImage.create_from_color_and_depth, applied in the kernel.  Bit-identical to S integrate() calls."""
        width, height, K = _intrinsic4(intrinsic)
        E = np.asarray(extrinsics, dtype=np.float64).reshape(-1, 4, 4)
        dev = self._vol.device
        as_dev = lambda x, dt: x.to(dev) if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)
        depths = as_dev(depths, np.uint16)
        if depths.dtype != torch.uint16 or depths.numel() != len(E) * width * height:
            raise RuntimeError("[UniformTSDFVolume::Integrate] Unsupported image format.")
        depths = depths.reshape(len(E), -1)
        if self._col is not None:
            if colors is None:
                raise RuntimeError("[UniformTSDFVolume::Integrate] Unsupported image format.")
            colors = as_dev(colors, np.uint8)
            if colors.dtype != torch.uint8 or colors.numel() != 3 * depths.numel():
                raise RuntimeError("[UniformTSDFVolume::Integrate] Unsupported image format.")
            colors = colors.reshape(len(E), -1)
        self._integrate(list(depths), list(colors) if self._col is not None else None, width, height, K, E, depth_scale, depth_trunc)

    def extract_point_cloud(self):
        """[O3D] extract_point_cloud: zero crossings along +x / +y / +z with normals (and colours of an RGB8 volume)"""
        pts, nrm, col = ops.tsdf_extract(self._vol, self._col, self.resolution, self.voxel_length, self.origin, "surface")
        return PointCloud._make(pts, col, nrm)

    def extract_voxel_point_cloud(self):
        """[O3D] extract_voxel_point_cloud: the centres of the valid voxels, grey = (tsdf + 1) / 2"""
        pts, _, col = ops.tsdf_extract(self._vol, self._col, self.resolution, self.voxel_length, self.origin, "voxels")
        return PointCloud._make(pts, col, None)

    def extract_triangle_mesh(self):
        """[O3D] extract_triangle_mesh: marching cubes over the active cubes (AC12) -> TriangleMesh with vertex colours from an RGB8
        volume and without normals; vertices ascend in (linear voxel index, axis)"""
        if getattr(self, "_vol", None) is None:
            raise NotImplementedError("UniformTSDFVolume.extract_triangle_mesh: needs a volume in device memory -- no CPU fallback")
        vert, col, tri = ops.tsdf_extract_mesh(self._vol, self._col, self.resolution, self.voxel_length, self.origin)
        return TriangleMesh._make(vert, tri, col)

    def __repr__(self):
        return f"UniformTSDFVolume with {self.color_type.name}, resolution {self.resolution}, voxel_length {self.voxel_length:g}."


def ScalableTSDFVolume(*a, **k):
    from .o3d import _off_path
    return _off_path("ScalableTSDFVolume")(*a, **k)

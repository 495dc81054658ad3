"""o3d.pipelines.integration over the kinectpx hot path: a uniform truncated-signed-distance volume in device memory that depth
images are integrated into (kpx_tsdf_integrate, arithmetic contract AC9 of DESIGN.md) and surface clouds are extracted from.
The batch form `integrate_frames` takes the rig's uint16 depth frames as they are and updates the volume for all of them in one
pass; extract_triangle_mesh is marching cubes over the same volume (AC12).  ScalableTSDFVolume keeps blocks of voxels where the
surface is (kpx_tsdf_blocks_*, AC16) with the same integration and extractions."""
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


class ScalableTSDFVolume:
    """[O3D] ScalableTSDFVolume(voxel_length, sdf_trunc, color_type, volume_unit_resolution=16, depth_sampling_stride=4): blocks
    ("volume units") of volume_unit_resolution^3 voxels on the world lattice, allocated where the band of +-sdf_trunc round a depth
    image's sampled pixels falls (arithmetic contract AC16).  Block (bx, by, bz) spans [b ul, (b + 1) ul) per axis with ul =
    voxel_length volume_unit_resolution; an image updates the blocks it touches and no others (Open3D's rule).  `_pool` is the
    append-only float32 (capacity, R^3, 2) {tsdf, weight} device tensor, `_col` the (capacity, R^3, 3) colours of an RGB8 volume,
    `_keys` / `_slots` the sorted index (packed block keys ascending, the pool slot of each).  The pool doubles when it is full.
    Outputs ascend in (block index, voxel index inside the block, axis) whatever the history of allocation -- Open3D walks a hash map.
    Extensions: integrate_frames, volume_unit_count, volume_unit_indices, unit_arrays, _set_units."""

    def __init__(self, voxel_length, sdf_trunc, color_type, volume_unit_resolution=16, depth_sampling_stride=4, _capacity=256):
        color_type = TSDFVolumeColorType(color_type)
        if color_type is TSDFVolumeColorType.Gray32:
            raise NotImplementedError("ScalableTSDFVolume: Gray32 volumes are not built (NoColor and RGB8 are)")
        self.voxel_length, self.sdf_trunc, self.color_type = float(voxel_length), float(sdf_trunc), color_type
        self.volume_unit_resolution, self.depth_sampling_stride = int(volume_unit_resolution), int(depth_sampling_stride)
        if not (1 <= self.volume_unit_resolution <= 32) or self.depth_sampling_stride < 1:
            raise RuntimeError("ScalableTSDFVolume: volume_unit_resolution must be in [1, 32], depth_sampling_stride at least 1")
        if not self.voxel_length > 0.0 or not self.sdf_trunc > 0.0:
            raise RuntimeError("ScalableTSDFVolume: voxel_length and sdf_trunc must be positive")
        self.volume_unit_length = self.voxel_length * self.volume_unit_resolution
        if self.sdf_trunc > self.volume_unit_length:
            raise RuntimeError("ScalableTSDFVolume: sdf_trunc must not exceed voxel_length * volume_unit_resolution")
        if not torch.cuda.is_available():
            raise NotImplementedError("ScalableTSDFVolume: the blocks live in device memory and no ROCm device is visible -- no CPU fallback")
        self._r3 = self.volume_unit_resolution ** 3
        self._capacity0 = max(int(_capacity), 1)
        self._alloc(self._capacity0)
        self._keys = self._slots = None

    def _alloc(self, capacity):
        dev = L.device()
        self._pool = torch.zeros((capacity, self._r3, 2), dtype=torch.float32, device=dev)
        self._col = torch.zeros((capacity, self._r3, 3), dtype=torch.float32, device=dev) if self.color_type is TSDFVolumeColorType.RGB8 else None

    def reset(self):
        self._alloc(self._capacity0)
        self._keys = self._slots = None

    def volume_unit_count(self):
        return 0 if self._keys is None else int(self._keys.numel())

    def volume_unit_indices(self):
        """int32 (B, 3) block indices, ascending in (bx, by, bz)"""
        if self._keys is None:
            return np.zeros((0, 3), dtype=np.int32)
        k = self._keys.cpu().numpy()
        return np.stack([((k >> s) & 0x1FFFFF) - (1 << 20) for s in (42, 21, 0)], 1).astype(np.int32)

    def unit_arrays(self):
        """(float32 (B, R^3, 2) {tsdf, weight}, float32 (B, R^3, 3) colours or None), blocks in volume_unit_indices() order, voxel
        (x, y, z) of a block at (x R + y) R + z"""
        if self._keys is None:
            return np.zeros((0, self._r3, 2), dtype=np.float32), None if self._col is None else np.zeros((0, self._r3, 3), dtype=np.float32)
        order = self._slots.long()
        return self._pool[order].cpu().numpy(), None if self._col is None else self._col[order].cpu().numpy()

    def _set_units(self, indices, tsdf_weight, colors=None):
        """replace the whole content: indices int (B, 3) in any order, tsdf_weight float32 (B, R^3, 2), colors float32 (B, R^3, 3)"""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
        tw = np.ascontiguousarray(tsdf_weight, dtype=np.float32).reshape(len(idx), self._r3, 2)
        if len(idx) and (idx.min() < -(1 << 20) or idx.max() >= (1 << 20)):
            raise RuntimeError("ScalableTSDFVolume: block indices must lie in [-2^20, 2^20)")
        keys = (idx[:, 0] + (1 << 20)) << 42 | (idx[:, 1] + (1 << 20)) << 21 | (idx[:, 2] + (1 << 20))
        order = np.argsort(keys, kind="stable")
        if len(np.unique(keys)) != len(keys):
            raise RuntimeError("ScalableTSDFVolume: a block index is given twice")
        self._alloc(max(len(idx), 1))
        self._keys = self._slots = None
        if len(idx) == 0:
            return
        dev = self._pool.device
        self._pool[:len(idx)].copy_(torch.from_numpy(tw[order]))
        if self._col is not None:
            self._col[:len(idx)].copy_(torch.from_numpy(np.ascontiguousarray(colors, dtype=np.float32).reshape(len(idx), self._r3, 3)[order]))
        self._keys = torch.from_numpy(keys[order]).to(dev)
        self._slots = torch.arange(len(idx), dtype=torch.int32, device=dev)

    def _grow(self, need):
        capacity = self._pool.shape[0]
        if need <= capacity:
            return
        old_pool, old_col, held = self._pool, self._col, self.volume_unit_count()
        self._alloc(max(2 * capacity, need))
        self._pool[:held].copy_(old_pool[:held])
        if old_col is not None:
            self._col[:held].copy_(old_col[:held])

    def _integrate(self, depths, colors, width, height, K, extrinsics, depth_scale=1.0, depth_trunc=0.0):
        E = np.asarray(extrinsics, dtype=np.float64).reshape(-1, 4, 4)
        R, stride, ul = self.volume_unit_resolution, self.depth_sampling_stride, self.volume_unit_length
        for first in range(0, len(E), 8):                      # KPX_TSDF_MAX_SENSORS images per touch: one host read each
            d, e = depths[first:first + 8], E[first:first + 8]
            c = colors[first:first + 8] if self._col is not None else None
            poses = np.stack([np.linalg.inv(x) for x in e])
            touched, new, ws = ops.tsdf_blocks_touch(self._keys, self._slots, d, width, height, K, poses, stride, ul, self.sdf_trunc, depth_scale,
                                                     depth_trunc)
            if new:
                self._grow(self.volume_unit_count() + new)
                self._keys, self._slots = ops.tsdf_blocks_insert(self._keys, self._slots, new, self._pool, self._col, R,
                                                                 (len(d), width, height, stride, ul, self.sdf_trunc), ws)
            if touched:
                ops.tsdf_blocks_integrate(self._pool, self._col, R, self.voxel_length, self.sdf_trunc, touched, d, c, width, height, K, e, stride, ws,
                                          depth_scale, depth_trunc)

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
            raise RuntimeError("[ScalableTSDFVolume::Integrate] Unsupported image format.")
        dev = self._pool.device
        host = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(dev).reshape(-1)
        self._integrate([host(depth)], [host(color)] if self._col is not None else None,
                        width, height, K, np.asarray(extrinsic, dtype=np.float64).reshape(1, 4, 4))

    def integrate_frames(self, depths, colors, intrinsic, extrinsics, depth_scale=1000.0, depth_trunc=3.0):
        """The batch form (an extension), arguments and image checks as UniformTSDFVolume.integrate_frames: S raw uint16 depth
        frames, their uint8 colours (None for a NoColor volume) and S extrinsics.  Bit-identical to S integrate() calls in ascending
        order; every eight images share one touch, one insertion and one pass over the blocks they touch."""
        width, height, K = _intrinsic4(intrinsic)
        E = np.asarray(extrinsics, dtype=np.float64).reshape(-1, 4, 4)
        dev = self._pool.device
        as_dev = lambda x, dt: x.to(dev) if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)
        depths = as_dev(depths, np.uint16)
        if depths.dtype != torch.uint16 or depths.numel() != len(E) * width * height:
            raise RuntimeError("[ScalableTSDFVolume::Integrate] Unsupported image format.")
        depths = depths.reshape(len(E), -1).contiguous()
        if self._col is not None:
            if colors is None:
                raise RuntimeError("[ScalableTSDFVolume::Integrate] Unsupported image format.")
            colors = as_dev(colors, np.uint8)
            if colors.dtype != torch.uint8 or colors.numel() != 3 * depths.numel():
                raise RuntimeError("[ScalableTSDFVolume::Integrate] Unsupported image format.")
            colors = colors.reshape(len(E), -1).contiguous()
        self._integrate(list(depths), list(colors) if self._col is not None else None, width, height, K, E, depth_scale, depth_trunc)

    def extract_point_cloud(self):
        """[O3D] extract_point_cloud: zero crossings along +x / +y / +z (the neighbour may lie in the next block) with normals"""
        pts, nrm, col = ops.tsdf_blocks_extract(self._keys, self._slots, self._pool, self._col, self.volume_unit_resolution, self.voxel_length, "surface")
        return PointCloud._make(pts, col, nrm)

    def extract_voxel_point_cloud(self):
        """[O3D] extract_voxel_point_cloud: the centres of the valid voxels, grey = (tsdf + 1) / 2"""
        pts, _, col = ops.tsdf_blocks_extract(self._keys, self._slots, self._pool, self._col, self.volume_unit_resolution, self.voxel_length, "voxels")
        return PointCloud._make(pts, col, None)

    def extract_triangle_mesh(self):
        """[O3D] extract_triangle_mesh: marching cubes with a cube at every voxel of every block; corners by global voxel index"""
        vert, col, tri = ops.tsdf_blocks_extract_mesh(self._keys, self._slots, self._pool, self._col, self.volume_unit_resolution, self.voxel_length)
        return TriangleMesh._make(vert, tri, col)

    def __repr__(self):
        return (f"ScalableTSDFVolume with {self.color_type.name}, voxel_length {self.voxel_length:g}, sdf_trunc {self.sdf_trunc:g}, "
                f"{self.volume_unit_count()} volume units of {self.volume_unit_resolution}^3.")

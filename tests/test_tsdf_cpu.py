"""CPU suite of the TSDF integration (AC9): the NumPy restatement tests/tsdf_ref.py against analytic scenes, and the host surface
(RGBDImage, PinholeCameraIntrinsic, errors, ABI).  Nothing here touches a device."""
import ctypes as C
import ctypes.util
import os
import re

import numpy as np
import pytest

import tsdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kpx_tsdf_workspace_bytes", "kpx_tsdf_integrate", "kpx_tsdf_extract_count", "kpx_tsdf_extract_fill")


def test_the_restatements_fma_is_the_c_librarys():
    """tsdf_ref.fma (error-free product and sum, rounding to odd) against libm's fma: random operands, products that cancel against
    the addend to the last bits, and sums that sit on rounding ties"""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype, libm.fma.argtypes = C.c_double, [C.c_double] * 3
    rng = np.random.default_rng(5)
    a = rng.normal(size=6000) * 10.0 ** rng.integers(-3, 4, 6000)
    b = rng.normal(size=6000) * 10.0 ** rng.integers(-3, 4, 6000)
    c = rng.normal(size=6000) * 10.0 ** rng.integers(-3, 4, 6000)
    c[2000:4000] = -(a[2000:4000] * b[2000:4000]) * (1.0 + rng.integers(-3, 4, 2000) * 2.0 ** -52)         # cancellation
    k = rng.integers(1, 1 << 26, 2000).astype(np.float64)
    a[4000:], b[4000:], c[4000:] = 1.0 + k * 2.0 ** -26, 1.0 + rng.integers(1, 1 << 26, 2000) * 2.0 ** -26, 2.0 ** rng.integers(-60, 60, 2000)
    got = R.fma(a, b, c)
    want = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


W8, H8, F8, CX8, CY8 = 80, 72, 63.0, 40.0, 36.0           # synth.small_xy(8)'s camera


@pytest.mark.parametrize("res,npts", [(16, 256), (33, 1089)])
def test_fronto_parallel_plane(res, npts):
    """a plane at constant depth 1510.3 seen by the identity camera: one point per (x, y) column, all from z edges, all within
    0.05 voxel of the plane (measured: 0.0018 voxel at resolution 16, 0.0017 at 33; a missing half-voxel offset gives 0.5)"""
    vol = R.Volume(1000.0, res, 4.0 * 1000.0 / res, origin=(-500.0, -500.0, 1000.0))
    depth = np.full(W8 * H8, 1510.3, np.float32)
    R.integrate(vol, depth, None, (F8, F8, CX8, CY8), W8, H8, np.eye(4))
    lin, axis = R.crossings(vol)
    pts, nrm, col = R.extract_point_cloud(vol)
    assert len(pts) == npts and col is None
    assert np.all(axis == 2)
    assert len(np.unique(lin // res)) == npts                                   # one per column
    err = np.abs(pts[:, 2].astype(np.float64) - float(np.float32(1510.3))) / vol.vl
    print("plane: worst distance", err.max(), "voxel")
    assert err.max() <= 0.05
    assert np.all(nrm[:, 2] < -0.99)                                            # towards the camera


def _sphere_depth(w, h, f, cx, cy, centre, radius):
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u)], -1).reshape(-1, 3)       # camera z == ray parameter
    A, B, Cq = (d * d).sum(1), -2.0 * (d @ centre), centre @ centre - radius * radius
    disc = B * B - 4.0 * A * Cq
    t = np.where(disc >= 0, (-B - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * A), 0.0)
    return t.astype(np.float32)


def test_analytic_sphere_normals_face_the_camera():
    """a sphere of radius 300 at (0, 0, 1500), ray-cast on a 160 x 144 camera, resolution 32 over an 800 volume: every point whose
    whole normal stencil (the 48 taps) has weight > 0 has a normal with a positive dot product with the direction to the camera.
    Measured: 513 such points of 824, worst angle between normal and radial direction 9.2 degrees (median 1.6), worst distance
    from the sphere 0.18 voxel."""
    w, h, f, cx, cy = 160, 144, 126.0, 80.0, 72.0
    centre, radius = np.array([0.0, 0.0, 1500.0]), 300.0
    depth = _sphere_depth(w, h, f, cx, cy, centre, radius)
    vol = R.Volume(800.0, 32, 100.0, origin=(-400.0, -400.0, 1100.0))
    R.integrate(vol, depth, None, (f, f, cx, cy), w, h, np.eye(4))
    pts, nrm, _ = R.extract_point_cloud(vol)
    assert len(pts) > 300
    p = pts.astype(np.float64)
    # the stencil of a point: the 2x2x2 cells around p +- gap e_k
    q = p - vol.origin
    full = np.ones(len(p), bool)
    wgt = vol.w.reshape(32, 32, 32)
    for k in range(3):
        for sgn in (-1.0, 1.0):
            qq = q.copy()
            qq[:, k] += sgn * 0.99 * vol.vl
            i0 = np.floor(qq / vol.vl - 0.5).astype(int)
            for t in range(8):
                i = i0 + np.array([t >> 2, (t >> 1) & 1, t & 1])
                inside = np.all((i >= 0) & (i < 32), 1)
                ii = np.clip(i, 0, 31)
                full &= inside & (wgt[ii[:, 0], ii[:, 1], ii[:, 2]] > 0)
    assert full.sum() > 100
    to_cam = -p / np.linalg.norm(p, axis=1, keepdims=True)
    dots = (nrm.astype(np.float64) * to_cam).sum(1)
    radial = (p - centre) / np.linalg.norm(p - centre, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip((nrm.astype(np.float64) * radial).sum(1), -1, 1)))
    print("sphere:", full.sum(), "of", len(p), "full stencils; worst angle", ang[full].max(), "median", np.median(ang[full]),
          "worst distance", (np.abs(np.linalg.norm(p - centre, axis=1) - radius) / vol.vl)[full].max(), "voxel")
    assert np.all(dots[full] > 0.0)


def test_rgbd_image_scale_truncation_and_intensity():
    from kinectpy_amd import o3d
    rng = np.random.default_rng(0)
    color = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    depth = rng.integers(0, 6000, (6, 5), dtype=np.uint16)
    im = o3d.geometry.RGBDImage.create_from_color_and_depth(o3d.geometry.Image(color), o3d.geometry.Image(depth))
    d = np.asarray(im.depth)
    want = depth.astype(np.float32) / np.float32(1000.0)
    want[want > np.float32(3.0)] = 0
    assert d.dtype == np.float32 and np.array_equal(d, want) and (d == 0).sum() > (depth == 0).sum()
    assert np.array_equal(d, R.depth_from_u16(depth, 1000.0, 3.0))
    c = np.asarray(im.color)
    f = color.astype(np.float32)
    assert c.dtype == np.float32 and c.shape == (6, 5)
    assert np.array_equal(c, (np.float32(0.299) * f[..., 0] + np.float32(0.587) * f[..., 1] + np.float32(0.114) * f[..., 2]) / np.float32(255))
    im = o3d.geometry.RGBDImage.create_from_color_and_depth(color, depth, depth_scale=1.0, depth_trunc=4000.0, convert_rgb_to_intensity=False)
    assert np.asarray(im.color).dtype == np.uint8 and np.array_equal(np.asarray(im.color), color)
    assert np.array_equal(np.asarray(im.depth), np.where(depth > 4000, 0, depth).astype(np.float32))
    assert (im.depth.width, im.depth.height, im.depth.num_of_channels, im.depth.bytes_per_channel) == (5, 6, 1, 4)
    assert (im.color.width, im.color.height, im.color.num_of_channels, im.color.bytes_per_channel) == (5, 6, 3, 1)
    with pytest.raises(RuntimeError):
        o3d.geometry.RGBDImage.create_from_color_and_depth(color, depth[:5])
    with pytest.raises(RuntimeError):
        o3d.geometry.Image(np.zeros((4, 4), np.float64))


def test_pinhole_intrinsic_accessors():
    from kinectpy_amd import o3d
    k = o3d.camera.PinholeCameraIntrinsic(80, 72, 63.0, 62.0, 40.0, 36.0)
    assert (k.width, k.height) == (80, 72) and k.get_focal_length() == (63.0, 62.0) and k.get_principal_point() == (40.0, 36.0)
    assert np.array_equal(k.intrinsic_matrix, [[63.0, 0, 40.0], [0, 62.0, 36.0], [0, 0, 1]]) and k.is_valid() and k.get_skew() == 0.0
    k2 = o3d.camera.PinholeCameraIntrinsic(80, 72, k.intrinsic_matrix)
    assert k2.get_focal_length() == (63.0, 62.0)


def test_stated_errors_without_a_device():
    from kinectpy_amd import integration, o3d
    ns = o3d.pipelines.integration
    assert {t.name for t in ns.TSDFVolumeColorType} == {"NoColor", "RGB8", "Gray32"}
    with pytest.raises(NotImplementedError, match="Gray32"):
        ns.UniformTSDFVolume(1.0, 8, 0.1, ns.TSDFVolumeColorType.Gray32)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ns.ScalableTSDFVolume(0.01, 0.04, ns.TSDFVolumeColorType.RGB8)
    with pytest.raises(NotImplementedError, match="extract_triangle_mesh"):
        ns.UniformTSDFVolume.extract_triangle_mesh(None)
    # the image checks come before any device work: a volume shell is enough
    k = o3d.camera.PinholeCameraIntrinsic(5, 6, 4.0, 4.0, 2.5, 3.0)
    for col_vol, color, depth in ((None, np.zeros((6, 5, 3), np.uint8), np.zeros((6, 5), np.uint16)),            # depth not float
                                  (None, np.zeros((6, 5, 3), np.uint8), np.zeros((5, 6), np.float32)),           # size differs from the intrinsic
                                  (None, np.zeros((5, 5, 3), np.uint8), np.zeros((6, 5), np.float32)),           # colour size differs
                                  (object(), np.zeros((6, 5), np.float32), np.zeros((6, 5), np.float32))):       # RGB8 volume, intensity image
        shell = object.__new__(integration.UniformTSDFVolume)
        shell._col = col_vol
        with pytest.raises(RuntimeError, match="Unsupported image format"):
            shell.integrate(o3d.geometry.RGBDImage(color, depth), k, np.eye(4))


def test_abi_symbols_and_workspace():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kinectpx.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in _lib.SIGNATURES and hasattr(lib, s), s
    sizes = [lib.kpx_tsdf_workspace_bytes(r) for r in range(1, 1025)]
    assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[63] >= 8 * (64 ** 3 // R.COUNT_BLOCK + 1)
    assert lib.kpx_tsdf_workspace_bytes(0) == 0 and lib.kpx_tsdf_workspace_bytes(1025) == 0
    # argument checks come before the device is touched
    z = np.zeros(16)
    zp = z.ctypes.data_as(C.c_void_p)
    assert lib.kpx_tsdf_integrate(C.c_void_p(4096), None, 2000, 1.0, zp, 1.0, 0, None, 0, 1.0, 1.0, None, 8, 8, zp, None, None) == -1
    assert b"resolution" in lib.kpx_last_error()
    assert lib.kpx_tsdf_integrate(C.c_void_p(4096), None, 8, 1.0, zp, -1.0, 0, None, 0, 1.0, 1.0, None, 8, 8, zp, None, None) == -1
    assert b"sdf_trunc" in lib.kpx_last_error()
    assert lib.kpx_tsdf_extract_count(C.c_void_p(4096), 8, 7, C.c_void_p(4096), C.c_void_p(4096), 4096, None) == -1 and b"mode" in lib.kpx_last_error()
    assert lib.kpx_tsdf_extract_count(C.c_void_p(4096), 64, 0, C.c_void_p(4096), C.c_void_p(4096), 64, None) == -2 and b"workspace" in lib.kpx_last_error()

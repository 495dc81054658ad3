"""CPU suite of the occupancy grids (AC10): the NumPy restatement tests/voxelgrid_ref.py on scenes whose answers are known -- by exact
rational arithmetic or by hand -- and the host surface (constructors' errors, index arithmetic, PinholeCameraParameters, off-path
methods, ABI).  Nothing here touches a device."""
import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import voxelgrid_ref as R
import voxelgrid_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kpx_voxelgrid_from_cloud_workspace_bytes", "kpx_voxelgrid_from_cloud", "kpx_voxelgrid_dense", "kpx_voxelgrid_carve_workspace_bytes",
           "kpx_voxelgrid_carve", "kpx_voxelgrid_included")


# ---- the rule in exact rational arithmetic, for integer scenes with the identity extrinsic ------------------------------------------
def exact_survivors(idx, image, K4, mode, keep_outside, keep_unmeasured=False):
    fx, fy, cx, cy = (Fraction(k) for k in K4)
    H, W = image.shape
    out = []
    for g in idx:
        kept = False
        for s in itertools.product((0, 1), repeat=3):
            x, y, z = (int(g[k]) + s[k] for k in range(3))
            within = False
            if z != 0:                                       # z == 0 divides to an infinity or a NaN: not within
                u, v = (fx * x + cx * z) / z, (fy * y + cy * z) / z
                within = 0 <= u <= W - 1 and 0 <= v <= H - 1
            if not within:
                kept |= bool(keep_outside)
                continue
            ui, vi = max(min(int(u), W - 2), 0), max(min(int(v), H - 2), 0)
            pu, pv = u - ui, v - vi
            a = lambda r, c: Fraction(float(image[r, c]))
            d = (a(vi, ui) * (1 - pv) + a(vi + 1, ui) * pv) * (1 - pu) + (a(vi, ui + 1) * (1 - pv) + a(vi + 1, ui + 1) * pv) * pu
            if d > 0:
                kept |= mode == "silhouette" or z >= d
            else:
                kept |= bool(keep_unmeasured)
        out.append(kept)
    return np.array(out, bool)


DENSE4 = R.create_dense((0.0, 0.0, 0.0), (0.5, 0.25, 1.0), 1.0, 4.0, 4.0, 4.0)
CAM9 = (4.0, 4.0, 4.0, 4.0)                  # 9 x 9 pixels: a corner (x, y, z) is inside the image iff 0 <= x <= z and 0 <= y <= z


def test_dense_grid_and_constant_depth():
    idx, col, origin = DENSE4
    assert idx.shape == (64, 3) and np.array_equal(idx, sorted(map(tuple, idx))) and np.array_equal(idx[1], (0, 0, 1)) and np.array_equal(idx[-1], (3, 3, 3))
    assert col.dtype == np.float32 and np.array_equal(col, np.tile(np.float32([0.5, 0.25, 1.0]), (64, 1)))
    depth = np.full((9, 9), 2.0, np.float32)
    for keep_outside in (False, True):
        got = R.carve(idx, origin, 1.0, depth, CAM9, np.eye(4), "depth", keep_outside)
        assert np.array_equal(got, exact_survivors(idx, depth, CAM9, "depth", keep_outside)), keep_outside
        if not keep_outside:
            # by hand: the corner (gx, gy, gz + 1) is the one most inside the image and farthest: z >= 2 and x, y <= z
            hand = (idx[:, 2] >= 1) & (idx[:, 0] <= idx[:, 2] + 1) & (idx[:, 1] <= idx[:, 2] + 1)
            assert np.array_equal(got, hand) and 0 < got.sum() < 64
        else:
            assert got[idx[:, 2] == 0].all()            # corners at z == 0 divide by zero: outside the image, kept
            assert got.sum() > exact_survivors(idx, depth, CAM9, "depth", False).sum()


def test_silhouette_of_a_centred_square():
    idx, _, origin = DENSE4
    mask = np.zeros((9, 9), np.float32)
    mask[3:6, 3:6] = 1.0
    got = R.carve(idx, origin, 1.0, mask, CAM9, np.eye(4), "silhouette", False)
    assert np.array_equal(got, exact_survivors(idx, mask, CAM9, "silhouette", False))
    # the bilinear sample is positive strictly between the pixels 2 and 6: the frustum -1/2 < x / z, y / z < 1/2, open.  The corner
    # nearest the axis is (gx, gy) (indices are >= 0) at the far face z = gz + 1
    hand = (2 * idx[:, 0] < idx[:, 2] + 1) & (2 * idx[:, 1] < idx[:, 2] + 1)
    assert np.array_equal(got, hand) and got.sum() == hand.sum() > 0
    # per column (gx, gy): the survivors are the voxels from some depth on
    for gx, gy in itertools.product(range(4), repeat=2):
        col = got[(idx[:, 0] == gx) & (idx[:, 1] == gy)]
        assert np.array_equal(col, np.sort(col))


def test_a_voxel_behind_the_camera_documents_the_missing_sign_test():
    idx, origin = np.array([[0, 0, 0]]), (0.0, 0.0, -2.0)             # x, y in [0, 1], z in [-2, -1]
    E, ones = np.eye(4), np.ones((9, 9), np.float32)
    u, v, z = R.project(R.corners(idx, origin, 1.0), CAM9, E)
    assert (z < 0).all() and set(u.ravel()) == {4.0, 2.0, 0.0}          # mirrored through the principal point, inside the image
    for depth in (np.full((9, 9), 0.5, np.float32), np.full((9, 9), 100.0, np.float32)):
        assert not R.carve(idx, origin, 1.0, depth, CAM9, E, "depth", False).any()          # z < 0 < d: never z >= d
        assert not R.carve(idx, origin, 1.0, depth, CAM9, E, "depth", True).any()           # and it IS within, so outside does not apply
    assert R.carve(idx, origin, 1.0, ones, CAM9, E, "silhouette", False).all()
    left = ones.copy()
    left[:, :5] = 0.0                                                    # the mirrored projection (u <= 4) lands off the mask
    assert not R.carve(idx, origin, 1.0, left, CAM9, E, "silhouette", False).any()
    assert np.array_equal(R.carve(idx, origin, 1.0, left, CAM9, E, "depth", False, keep_unmeasured=True), [True])


def test_edge_decisions_with_exact_numbers():
    idx = np.array([[0, 0, 0]])
    seen = {}
    for name, origin, image, mode, survives in S.edge_scenes():
        u, v, z = R.project(R.corners(idx, origin, 1.0), S.K4, np.eye(4))
        assert ((v >= 0) & (v <= S.H - 1)).all(), name
        seen[name] = u.ravel()
        got = R.carve(idx, origin, 1.0, image, S.K4, np.eye(4), mode, False)
        assert bool(got[0]) == survives, name
    assert sorted(seen["u == 0 is within"]) == [-12.0, -12.0, -8.0, -8.0, -2.0, -2.0, 0.0, 0.0]
    assert seen["below u == 0 is not"].max() == -2.0 * S.EPS4
    assert sorted(set(seen["u == W - 1 is within"])) == [16.0, 18.0, 24.0, 28.0]
    assert seen["one ulp beyond u == W - 1 is not"].min() == np.nextafter(16.0, np.inf)


def test_unmeasured_pixels_and_nan():
    idx, origin = np.array([[0, 0, 0]]), (0.0, 0.0, 1.0)
    hole = np.zeros((S.H, S.W), np.float32)
    assert not R.carve(idx, origin, 1.0, hole, S.K4, np.eye(4), "depth", False).any()               # Open3D's rule: no depth carves
    assert R.carve(idx, origin, 1.0, hole, S.K4, np.eye(4), "depth", False, keep_unmeasured=True).all()
    nan = np.full((S.H, S.W), np.nan, np.float32)
    assert not R.carve(idx, origin, 1.0, nan, S.K4, np.eye(4), "silhouette", True).any()             # within, and NaN > 0 is false
    within, _ = R.sample(hole, np.array([np.nan, np.inf, -0.0, 16.0]), np.array([1.0, 1.0, 8.0, 8.0]))
    assert list(within) == [False, False, True, True]


def test_grid_of_a_cloud_by_hand():
    pts = np.float32([[0.0, 0.0, 0.0], [0.4, 0.0, 0.0], [0.6, 0.0, 0.0], [2.0, 1.0, 0.0], [0.1, 0.1, 0.1]])
    col = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5], [1, 1, 1]])
    idx, c, origin = R.create_from_point_cloud(pts, 1.0, col)
    assert np.array_equal(origin, [-0.5, -0.5, -0.5])
    assert np.array_equal(idx, [[0, 0, 0], [1, 0, 0], [2, 1, 0]])                 # floor(x + 0.5): 0.4 -> 0, 0.6 -> 1
    assert c.dtype == np.float32 and np.array_equal(c, np.float32([[2.0 / 3.0, 2.0 / 3.0, 1.0 / 3.0], [0, 0, 1], [0.5, 0.5, 0.5]]))          # (float)(sum / 3)
    idx2, c2, origin2 = R.create_from_point_cloud(pts, 1.0, None, origin=(-1.0, -1.0, -1.0))
    assert np.array_equal(idx2, [[1, 1, 1], [3, 2, 1]]) and not c2.any() and np.array_equal(origin2, [-1, -1, -1])
    with pytest.raises(ValueError, match="too small"):
        R.create_from_point_cloud(pts, 1e-7)
    with pytest.raises(ValueError, match="too small"):
        R.create_from_point_cloud(pts, 1.0, origin=(1.0, 0.0, 0.0))              # a point below the origin: index -1
    inc = R.included(idx, origin, 1.0, np.array([[0.49, 0.0, 0.0], [0.5, 0.0, 0.0], [1.5, 0.0, 0.0], [np.nan, 0, 0], [-0.6, 0, 0], [3e6, 0, 0]]))
    assert list(inc) == [True, True, False, False, False, False]
    lo, hi = R.bounds(idx, origin, 1.0)
    assert np.array_equal(lo, [-0.5, -0.5, -0.5]) and np.array_equal(hi, [2.5, 1.5, 0.5])
    assert [R.round_half_away(q) for q in (0.5, 1.5, 2.5, 0.49999999999999994, -0.5, 2.4)] == [1, 2, 3, 0, -1, 2]


# ---- host surface ----------------------------------------------------------------------------------------------------------------------
def shell(origin=(0.0, 0.0, 0.0), voxel_size=1.0):
    from kinectpy_amd import o3d
    g = o3d.geometry.VoxelGrid()
    g.origin, g.voxel_size = np.asarray(origin, np.float64), float(voxel_size)
    return g


def test_index_arithmetic_by_hand():
    from kinectpy_amd import o3d
    g = o3d.geometry.VoxelGrid()
    assert repr(g) == "VoxelGrid with 0 voxels." and g.is_empty() and not g.has_voxels() and g.has_colors() and g.get_voxels() == []
    assert g.voxel_size == 0.0 and np.array_equal(g.origin, np.zeros(3))
    g = shell((1.0, -2.0, 0.5), 0.25)
    v = g.get_voxel((1.3, -2.0, 0.49))
    assert v.dtype == np.int32 and list(v) == [1, 0, -1]
    assert np.array_equal(g.get_voxel_center_coordinate((1, 0, -1)), [1.375, -1.875, 0.375])
    pts = g.get_voxel_bounding_points((1, 0, -1))
    assert len(pts) == 8 and {tuple(p) for p in pts} == set(itertools.product((1.25, 1.5), (-2.0, -1.75), (0.25, 0.5)))
    assert np.array_equal(pts[0], [1.25, -2.0, 0.25]) and np.array_equal(pts[1], [1.25, -2.0, 0.5]) and np.array_equal(pts[7], [1.5, -1.75, 0.5])
    assert {tuple(p) for p in R.corners([[1, 0, -1]], g.origin, 0.25)[0]} == {tuple(p) for p in pts}
    assert np.array_equal(g.get_min_bound(), g.origin) and np.array_equal(g.get_max_bound(), g.origin) and np.array_equal(g.get_center(), g.origin)
    assert g.clear() is g and g.voxel_size == 0.0
    vx = o3d.geometry.Voxel((1, 2, 3), (0.5, 0.25, 1.0))
    assert vx.grid_index.dtype == np.int32 and list(vx.grid_index) == [1, 2, 3] and list(vx.color) == [0.5, 0.25, 1.0]
    assert list(o3d.geometry.Voxel().grid_index) == [0, 0, 0]


def test_constructor_errors_without_a_device():
    from kinectpy_amd import o3d
    VG = o3d.geometry.VoxelGrid
    for v in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="voxel_size <= 0"):
            VG.create_from_point_cloud(None, v)
        with pytest.raises(RuntimeError, match="voxel_size <= 0"):
            VG.create_from_point_cloud_within_bounds(None, v, (0, 0, 0), (1, 1, 1))
        with pytest.raises(RuntimeError, match="voxel_size <= 0"):
            VG.create_dense((0, 0, 0), (0, 0, 0), v, 1.0, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="voxel_size is too small"):
        VG.create_from_point_cloud_within_bounds(None, 1e-6, (0, 0, 0), (1.0, 1.0, 3000.0))
    with pytest.raises(RuntimeError, match="cells per axis"):
        VG.create_dense((0, 0, 0), (0, 0, 0), 1.0, 2.0 ** 21 + 1, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="cells per axis"):
        VG.create_dense((0, 0, 0), (0, 0, 0), 1.0, 2048.0, 2048.0, 512.0)                # 2^31 voxels
    with pytest.raises(RuntimeError, match="non-negative"):
        VG.create_dense((0, 0, 0), (0, 0, 0), 1.0, -3.0, 1.0, 1.0)
    empty = VG.create_dense((1.0, 2.0, 3.0), (0, 0, 0), 1.0, 0.4, 5.0, 5.0)              # round(0.4) = 0 cells: an empty grid
    assert empty.is_empty() and np.array_equal(empty.origin, [1, 2, 3]) and empty.voxel_size == 1.0


def test_off_path_methods_raise():
    from kinectpy_amd import o3d
    g = shell()
    for call in (lambda: g.add_voxel(o3d.geometry.Voxel()), lambda: g.remove_voxel((0, 0, 0)), lambda: g.to_octree(3), lambda: g.create_from_octree(None),
                 lambda: o3d.geometry.VoxelGrid.create_from_triangle_mesh(None, 1.0),
                 lambda: o3d.geometry.VoxelGrid.create_from_triangle_mesh_within_bounds(None, 1.0, (0, 0, 0), (1, 1, 1))):
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            call()


def test_camera_parameters_and_image_errors_without_a_device():
    from kinectpy_amd import o3d
    p = o3d.camera.PinholeCameraParameters()
    assert np.array_equal(p.extrinsic, np.eye(4)) and isinstance(p.intrinsic, o3d.camera.PinholeCameraIntrinsic)
    p.intrinsic = o3d.camera.PinholeCameraIntrinsic(5, 6, 4.0, 4.0, 2.5, 3.0)
    p.extrinsic = np.arange(16).reshape(4, 4)
    assert p.extrinsic.dtype == np.float64 and p.extrinsic[1, 2] == 6.0
    with pytest.raises(RuntimeError, match="4x4"):
        p.extrinsic = np.eye(3)
    p.extrinsic = np.eye(4)
    g = shell()
    for method in (g.carve_depth_map, g.carve_silhouette):
        with pytest.raises(RuntimeError, match="not compatible with the provided camera_parameters"):
            method(o3d.geometry.Image(np.zeros((5, 6), np.float32)), p)
        with pytest.raises(RuntimeError, match="Unsupported image format"):
            method(o3d.geometry.Image(np.zeros((6, 5), np.uint16)), p)
        with pytest.raises(RuntimeError, match="Unsupported image format"):
            method(o3d.geometry.Image(np.zeros((6, 5, 3), np.uint8)), p)
        assert method(o3d.geometry.Image(np.zeros((6, 5), np.float32)), p) is g              # an empty grid: nothing to carve
    skew = o3d.camera.PinholeCameraParameters(o3d.camera.PinholeCameraIntrinsic(5, 6, np.array([[4.0, 0.1, 2.5], [0, 4.0, 3.0], [0, 0, 1.0]])))
    with pytest.raises(RuntimeError, match="no skew"):
        g.carve_depth_map(o3d.geometry.Image(np.zeros((6, 5), np.float32)), skew)
    scaled = o3d.camera.PinholeCameraIntrinsic(5, 6, np.array([[4.0, 0.0, 2.5], [0, 4.0, 3.0], [0, 0, 2.0]]))
    with pytest.raises(RuntimeError, match="no skew"):
        g.carve_depth_maps(np.zeros((1, 30), np.uint16), scaled, np.eye(4)[None])
    k = p.intrinsic
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        g.carve_depth_maps(np.zeros((1, 30), np.float32), k, np.eye(4)[None])
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        g.carve_depth_maps(np.zeros((2, 30), np.uint16), k, np.eye(4)[None])
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        g.carve_silhouettes(np.zeros((1, 30), np.uint16), k, np.eye(4)[None])
    assert g.carve_silhouettes(np.zeros((1, 6, 5), bool), k, np.eye(4)[None]) is g
    assert g.carve_depth_maps(np.zeros((1, 30), np.uint16), k, np.eye(4)[None]) is g


def test_symbols_are_exported():
    from kinectpy_amd import geometry, o3d, ops
    from kinectpy_amd.preprocessing import fusion
    assert o3d.geometry.VoxelGrid is geometry.VoxelGrid and o3d.geometry.Voxel is geometry.Voxel
    assert o3d.camera.PinholeCameraParameters is o3d.PinholeCameraParameters
    for name in ("voxelgrid_from_cloud", "voxelgrid_dense", "voxelgrid_carve", "voxelgrid_included"):
        assert callable(getattr(ops, name))
    for name in ("create_from_point_cloud", "create_from_point_cloud_within_bounds", "create_dense", "get_voxels", "has_voxels", "has_colors", "is_empty",
                 "clear", "get_voxel", "get_voxel_center_coordinate", "get_voxel_bounding_points", "check_if_included", "carve_depth_map",
                 "carve_silhouette", "carve_depth_maps", "carve_silhouettes", "included_mask", "get_min_bound", "get_max_bound", "get_center"):
        assert callable(getattr(geometry.VoxelGrid, name)), name
    assert isinstance(geometry.VoxelGrid.voxel_indices, property) and isinstance(geometry.VoxelGrid.voxel_colors, property)
    assert callable(fusion.remove_free_space_points)


def test_abi_symbols_workspace_and_argument_checks():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kinectpx.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in _lib.SIGNATURES and hasattr(lib, s), s
    sizes = [1, 2, 63, 64, 65, 257, 2048, 2049, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31 - 1]
    for query in (lib.kpx_voxelgrid_from_cloud_workspace_bytes, lib.kpx_voxelgrid_carve_workspace_bytes):
        b = [query(n) for n in sizes]
        assert all(y >= x > 0 for x, y in zip(b, b[1:])) and b[-1] > b[0], b
        assert query(0) > 0 and query(-1) == 0 and query(2 ** 31) == 0
    assert lib.kpx_voxelgrid_carve_workspace_bytes(10 ** 6) >= 10 ** 6              # one flag byte per voxel
    # argument checks come before the device is touched
    z = np.zeros(16)
    zp, P, Q = z.ctypes.data_as(C.c_void_p), C.c_void_p(4096), C.c_void_p(8192)
    carve = lambda m=10, v=1.0, mode=0, fmt=0, w=8, h=8, scale=1.0, ok=Q, ws=1 << 20: lib.kpx_voxelgrid_carve(
        P, P, m, zp, v, mode, 0, None, fmt, scale, 1.0, w, h, zp, None, 0, 0, ok, Q, P, P, ws, None)
    for call, word in ((lambda: carve(v=0.0), b"voxel_size <= 0"), (lambda: carve(mode=2), b"mode"), (lambda: carve(fmt=3), b"pixel format"),
                       (lambda: carve(w=1), b"width, height >= 2"), (lambda: carve(fmt=1, scale=0.0), b"depth_scale"), (lambda: carve(m=-1), b"bad size"),
                       (lambda: carve(ok=P), b"aliases")):
        assert call() == -1 and word in lib.kpx_last_error(), word
    assert carve(ws=16) == -2 and b"workspace" in lib.kpx_last_error()
    from_cloud = lambda n=10, v=1.0, org=None, ws=1 << 30: lib.kpx_voxelgrid_from_cloud(P, None, n, v, org, P, P, P, P, P, ws, None)
    assert from_cloud(v=-1.0) == -1 and b"voxel_size <= 0" in lib.kpx_last_error()
    assert from_cloud(n=2 ** 31) == -1 and b"bad size" in lib.kpx_last_error()
    z[0] = np.inf
    assert from_cloud(org=zp) == -1 and b"finite" in lib.kpx_last_error()
    assert lib.kpx_voxelgrid_included(P, 0, 5, P, 5, zp, 1.0, P, None) == -1 and b"finite" in lib.kpx_last_error()
    z[0] = 0.0
    assert from_cloud(ws=16) == -2 and b"workspace" in lib.kpx_last_error()
    dense = lambda a, b, c: lib.kpx_voxelgrid_dense(a, b, c, zp, P, P, None)
    assert dense(2 ** 21 + 1, 1, 1) == -1 and b"dimension" in lib.kpx_last_error()
    assert dense(2048, 2048, 512) == -1 and b"2^31 - 1" in lib.kpx_last_error()
    assert dense(3, 0, 5) == 0
    assert lib.kpx_voxelgrid_included(P, 0, 5, P, 5, zp, 0.0, P, None) == -1 and b"voxel_size <= 0" in lib.kpx_last_error()
    assert lib.kpx_voxelgrid_included(P, 0, -1, P, 5, zp, 1.0, P, None) == -1 and b"bad size" in lib.kpx_last_error()
    assert lib.kpx_voxelgrid_included(None, 0, 0, None, 0, zp, 1.0, None, None) == 0

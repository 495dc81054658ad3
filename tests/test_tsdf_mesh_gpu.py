"""GPU suite of the mesh extraction (kpx_tsdf_mesh_*, kpx_mesh_normals, kpx_mesh_surface_area; AC12): every vertex, colour,
triangle, normal and the area bit for bit against the serial restatement tests/tsdf_mesh_ref.py -- on the synthetic ring's fused
volumes and on uploaded random volumes whose sizes sit on the kernels' chunk and group boundaries."""
import copy
import functools

import numpy as np
import pytest

import tsdf_mesh_ref as M

pytestmark = pytest.mark.gpu

W, H, K4 = 80, 72, (63.0, 63.0, 40.0, 36.0)
LENGTH, ORIGIN = 2000.0, (-1000.0, -1100.0, -1000.0)           # the person stands at the world's origin
SCALE, TRUNC = 1.0, 6000.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(None)
def ring():
    """depth u16 (2, 4, n_px), rgb u8 (2, 4, n_px, 3), world -> camera extrinsics of the four ring cameras"""
    from kinectpy_amd.utils import synth
    _, depth, rgb, _, _ = synth.sensor_ring(4, 2, synth.small_xy(8))
    extr = np.stack([np.linalg.inv(synth.camera_pose(g, 4)) for g in range(4)])
    return depth, rgb, extr


def intrinsic():
    from kinectpy_amd import o3d
    return o3d.camera.PinholeCameraIntrinsic(W, H, *K4)


def gpu_volume(res, color=True, origin=ORIGIN, length=LENGTH):
    from kinectpy_amd import o3d
    ns = o3d.pipelines.integration
    return ns.UniformTSDFVolume(length, res, 4.0 * length / res, ns.TSDFVolumeColorType.RGB8 if color else ns.TSDFVolumeColorType.NoColor, origin)


def upload(vol, tsdf, weight, col):
    import torch
    vol._vol.copy_(torch.from_numpy(np.stack([tsdf, weight], 1)))
    if col is not None:
        vol._col.copy_(torch.from_numpy(col))


def download(vol):
    v = vol._vol.cpu().numpy()
    return np.ascontiguousarray(v[:, 0]), np.ascontiguousarray(v[:, 1]), None if vol._col is None else vol._col.cpu().numpy()


def reference(vol):
    """the restatement's mesh of what the device volume holds (the integration itself is tests/test_tsdf_gpu.py's subject)"""
    f, w, c = download(vol)
    return M.extract_triangle_mesh(f, w, c, vol.resolution, vol.voxel_length, vol.origin)


@functools.lru_cache(None)
def ring_case(res, color):
    depth, rgb, extr = ring()
    vol = gpu_volume(res, color)
    vol.integrate_frames(depth[0], rgb[0] if color else None, intrinsic(), extr, SCALE, TRUNC)
    return vol, reference(vol)


@functools.lru_cache(None)
def random_case(res, all_weights=False):
    """tsdf uniform in [-1, 1) with a sprinkling of exact 0, -0 and +-1; one voxel in ten of weight 0 unless all_weights; random
    colours; an origin and a voxel length that are no round numbers"""
    rng = np.random.default_rng(1000 + res + (500 if all_weights else 0))
    n = res ** 3
    f = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    where = rng.random(n) < 0.08
    f[where] = special[rng.integers(0, 4, int(where.sum()))]
    w = np.ones(n, dtype=np.float32) if all_weights else np.where(rng.random(n) < 0.1, 0.0, rng.integers(1, 9, n)).astype(np.float32)
    c = rng.uniform(0.0, 255.0, (n, 3)).astype(np.float32)
    vol = gpu_volume(res, True, origin=(-0.37, 1.91, 12.3), length=res * 0.013)
    upload(vol, f, w, c)
    return vol, M.extract_triangle_mesh(f, w, c, res, vol.voxel_length, vol.origin)


def arrays(mesh):
    g = lambda t: None if t is None else t.cpu().numpy()
    return g(mesh._vert), g(mesh._vcol), g(mesh._tri)


def assert_mesh(vol, ref):
    """extraction, then normals (both forms) and area, against the restatement"""
    rv, rc, rt, _ = ref
    mesh = vol.extract_triangle_mesh()
    v, c, t = arrays(mesh)
    assert v.shape == rv.shape and t.shape == rt.shape, (v.shape, rv.shape, t.shape, rt.shape)
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert same(v, rv), f"vertices differ at {np.flatnonzero((bits(v) != bits(rv)).any(1))[:5]}"
    assert np.array_equal(t, rt), f"triangles differ at {np.flatnonzero((t != rt).any(1))[:5]}"
    if rc is not None:
        assert same(c, rc)
    else:
        assert c is None and not mesh.has_vertex_colors()
    assert not mesh.has_vertex_normals() and not mesh.has_triangle_normals()
    for normalized in (True, False):
        assert mesh.compute_triangle_normals(normalized) is mesh
        assert same(mesh._tnrm.cpu().numpy(), M.triangle_normals(rv, rt, normalized))
        mesh._tnrm = None
        assert mesh.compute_vertex_normals(normalized) is mesh
        assert same(mesh._tnrm.cpu().numpy(), M.triangle_normals(rv, rt, normalized))
        assert same(mesh._vnrm.cpu().numpy(), M.vertex_normals(rv, rt, normalized))
    area = mesh.get_surface_area()
    assert isinstance(area, float) and np.float64(area).view(np.uint64) == np.float64(M.surface_area(rv, rt)).view(np.uint64)
    return mesh


@pytest.mark.parametrize("res", [16, 40])
@pytest.mark.parametrize("color", [True, False])
def test_ring_volume(res, color):
    vol, ref = ring_case(res, color)
    assert len(ref[0]) > 20 and len(ref[2]) > 20
    mesh = assert_mesh(vol, ref)
    assert repr(mesh) == f"TriangleMesh with {len(ref[0])} points and {len(ref[2])} triangles."
    lo, hi = ref[0].astype(np.float64).min(0), ref[0].astype(np.float64).max(0)
    assert np.array_equal(mesh.get_min_bound(), lo) and np.array_equal(mesh.get_max_bound(), hi)


@pytest.mark.parametrize("res", [2, 3, 8, 9, 16, 33])
def test_random_volume_with_holes(res):
    """one voxel in ten has weight 0: about 0.9^8 = 43 % of the cubes stay active, and edges whose four cubes are partly inactive
    occur.  8^3 is exactly one 512-voxel chunk, 9^3 leaves a ragged second one, 33 is odd: rows straddle the 64-voxel groups."""
    vol, ref = random_case(res)
    if res >= 8:
        assert len(ref[2]) > 0
    assert_mesh(vol, ref)


@pytest.mark.parametrize("res", [2, 3, 8, 9, 16, 33])
def test_random_volume_all_active(res):
    """every weight 1: cubes on the volume's border faces are active, and from 16^3 on every one of the 256 codes occurs"""
    vol, ref = random_case(res, True)
    if res >= 16:
        f, w, _ = download(vol)
        hist = np.bincount(M.cube_codes(f, w, res).reshape(-1), minlength=256)
        assert np.all(hist > 0), np.flatnonzero(hist == 0)
    assert_mesh(vol, ref)


@pytest.mark.parametrize("case", ["res1", "zeros", "weightless"])
def test_empty_meshes(case):
    res = 1 if case == "res1" else 9
    vol = gpu_volume(res, True)
    n = res ** 3
    if case == "res1":
        upload(vol, np.full(n, -0.5, np.float32), np.ones(n, np.float32), np.zeros((n, 3), np.float32))
    elif case == "weightless":
        rng = np.random.default_rng(3)
        upload(vol, rng.uniform(-1, 1, n).astype(np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32))
    mesh = vol.extract_triangle_mesh()
    v, c, t = arrays(mesh)
    assert v.shape == (0, 3) and v.dtype == np.float32 and c.shape == (0, 3) and t.shape == (0, 3) and t.dtype == np.int32
    assert mesh.is_empty() and not mesh.has_vertices() and not mesh.has_triangles() and not mesh.has_vertex_colors()
    mesh.compute_vertex_normals()
    assert mesh._vnrm.shape == (0, 3) and mesh._tnrm.shape == (0, 3) and not mesh.has_vertex_normals()
    assert mesh.get_surface_area() == 0.0
    assert np.array_equal(mesh.get_min_bound(), np.zeros(3)) and np.array_equal(mesh.get_max_bound(), np.zeros(3))


def fan():
    """70 triangles round vertex 0 (more than a wave's lanes in one segment of the vertex sums), one degenerate triangle, and an
    unused last vertex"""
    rng = np.random.default_rng(11)
    ang = np.linspace(0.0, 2.0 * np.pi, 71)
    rim = np.stack([np.cos(ang) * (1.0 + 0.3 * rng.random(71)), np.sin(ang) * (1.0 + 0.3 * rng.random(71)), 0.2 * rng.standard_normal(71)], 1)
    v = np.concatenate([[[0.013, -0.02, 0.5]], rim, [[9.0, 9.0, 9.0]]]).astype(np.float32)
    t = [[0, 1 + i, 2 + i] for i in range(70)] + [[5, 5, 9]]
    return v, np.array(t, dtype=np.int32)


def test_vertex_normals_of_a_hand_made_fan():
    from kinectpy_amd import o3d
    v, t = fan()
    mesh = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(v), o3d.utility.Vector3iVector(t))
    assert mesh.has_triangles() and np.array_equal(np.asarray(mesh.triangles), t) and np.asarray(mesh.vertices).dtype == np.float64
    for normalized in (True, False):
        mesh.compute_vertex_normals(normalized)
        assert same(mesh._vnrm.cpu().numpy(), M.vertex_normals(v, t, normalized))
        assert same(mesh._tnrm.cpu().numpy(), M.triangle_normals(v, t, normalized))
    mesh.compute_vertex_normals()
    assert np.array_equal(np.asarray(mesh.vertex_normals)[-1], [0.0, 0.0, 1.0])             # the unused vertex
    assert np.array_equal(np.asarray(mesh.triangle_normals)[-1], [0.0, 0.0, 1.0])           # the degenerate triangle
    assert mesh.get_surface_area() == M.surface_area(v, t)
    # a mesh without triangles: every vertex normal is the zero vector's (0, 0, 1)
    bare = o3d.geometry.TriangleMesh(v)
    bare.compute_vertex_normals()
    assert np.array_equal(np.asarray(bare.vertex_normals), np.tile([0.0, 0.0, 1.0], (len(v), 1))) and not bare.has_triangle_normals()


def test_transform_deepcopy_and_setters():
    from kinectpy_amd import o3d, ops
    v, t = fan()
    mesh = o3d.geometry.TriangleMesh(v, t).compute_vertex_normals()
    mesh.vertex_colors = o3d.utility.Vector3dVector(np.full((len(v), 3), 0.25))
    twin = copy.deepcopy(mesh)
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (1.0, 2.0, 3.0)
    assert mesh.transform(T) is mesh
    assert same(mesh._vert.cpu().numpy(), ops.transform(twin._vert, T).cpu().numpy())
    assert same(mesh._vnrm.cpu().numpy(), ops.rotate(twin._vnrm, T).cpu().numpy())
    assert same(mesh._tnrm.cpu().numpy(), ops.rotate(twin._tnrm, T).cpu().numpy())
    assert same(twin._vert.cpu().numpy(), v) and twin.has_vertex_colors() and twin.has_vertex_normals() and twin.has_triangle_normals()
    assert np.array_equal(mesh.get_max_bound(), mesh._vert.cpu().numpy().astype(np.float64).max(0))
    twin.vertex_normals = o3d.utility.Vector3dVector()
    assert not twin.has_vertex_normals()


@pytest.mark.parametrize("bad", [-1, 73])
def test_triangle_index_out_of_range_raises_before_any_launch(bad):
    from kinectpy_amd import o3d
    v, t = fan()
    assert len(v) == 73
    t = t.copy()
    t[40, 1] = bad
    mesh = o3d.geometry.TriangleMesh(v, t)
    for call in (mesh.compute_vertex_normals, mesh.compute_triangle_normals, mesh.get_surface_area):
        with pytest.raises(RuntimeError, match="out of range"):
            call()
    assert mesh._vnrm is None and mesh._tnrm is None


def test_fuse_depth_tsdf_mesh_and_default():
    from kinectpy_amd.preprocessing.fusion import fuse_depth_tsdf
    from kinectpy_amd.utils import synth
    _, depth, rgb, _, truth = synth.sensor_ring(4, xy=synth.small_xy(8))
    origin = (-1000.0, -1100.0, 1500.0)                 # the master's frame: the person stands 2500 in front of it
    extr = np.stack([np.eye(4)] + [np.linalg.inv(T) for T in truth])
    vol = gpu_volume(32, True, origin)
    vol.integrate_frames(depth[0], rgb[0], intrinsic(), extr, 1.0, 6000.0)
    manual = vol.extract_triangle_mesh().compute_vertex_normals()
    mesh = fuse_depth_tsdf(depth[0], rgb[0], intrinsic(), truth, LENGTH, 32, origin, mesh=True)
    assert len(mesh._vert) > 100 and mesh.has_vertex_normals() and mesh.has_triangle_normals() and mesh.has_vertex_colors()
    for a, b in zip(arrays(mesh) + (mesh._vnrm.cpu().numpy(), mesh._tnrm.cpu().numpy()),
                    arrays(manual) + (manual._vnrm.cpu().numpy(), manual._tnrm.cpu().numpy())):
        assert same(a, b)
    assert same(mesh._vert.cpu().numpy(), reference(vol)[0])
    nocol = fuse_depth_tsdf(depth[0], None, intrinsic(), truth, LENGTH, 32, origin, mesh=True)
    assert same(nocol._vert.cpu().numpy(), mesh._vert.cpu().numpy()) and nocol._vcol is None
    # the default is the point cloud, as before
    pc, want = fuse_depth_tsdf(depth[0], rgb[0], intrinsic(), truth, LENGTH, 32, origin), vol.extract_point_cloud()
    assert len(pc._pts) == 687
    assert same(pc._pts.cpu().numpy(), want._pts.cpu().numpy()) and same(pc._nrm.cpu().numpy(), want._nrm.cpu().numpy())
    assert same(pc._col.cpu().numpy(), want._col.cpu().numpy())


def test_extraction_is_repeatable():
    vol, _ = random_case(33)
    a, b = vol.extract_triangle_mesh(), vol.extract_triangle_mesh()
    for x, y in zip(arrays(a), arrays(b)):
        assert same(x, y)
    for m in (a, b):
        m.compute_vertex_normals()
    assert same(a._vnrm.cpu().numpy(), b._vnrm.cpu().numpy()) and a.get_surface_area() == b.get_surface_area()


def test_ply_file_round_trip_of_an_extracted_mesh(tmp_path):
    from kinectpy_amd import o3d
    vol, ref = ring_case(16, True)
    mesh = vol.extract_triangle_mesh().compute_vertex_normals()
    for ascii_ in (False, True):
        path = str(tmp_path / f"mesh{int(ascii_)}.ply")
        assert o3d.io.write_triangle_mesh(path, mesh, write_ascii=ascii_)
        back = o3d.io.read_triangle_mesh(path)
        assert same(back._vert.cpu().numpy(), mesh._vert.cpu().numpy()) and np.array_equal(back._tri.cpu().numpy(), mesh._tri.cpu().numpy())
        assert same(back._vnrm.cpu().numpy(), mesh._vnrm.cpu().numpy())
        want = np.clip(np.round(mesh._vcol.cpu().numpy().astype(np.float64) * 255.0), 0, 255) / 255.0
        assert np.array_equal(np.asarray(back.vertex_colors), want.astype(np.float32).astype(np.float64))

"""GPU suite of the objects' contracts: value semantics between geometry objects, snapshot at hand-over, cache
coherence.  Every test builds its objects from host arrays, obtains one object from another by a public operation, changes one of
the two in place and holds the other -- and every cached answer of both -- to bit equality.  Sources, mutators and fixtures come from
tests/object_state.py; the kernels underneath are pinned by their own suites, so an error here is an object handing the right kernel
the wrong tensor."""
import copy
import functools

import numpy as np
import pytest

import object_state as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def cloud_h():
    return S.cloud_arrays()


@functools.lru_cache(None)
def mesh_h():
    """the closed mesh with four triangles flipped: orient_triangles has work to do on it, and on whatever holds its triangles"""
    return S.mesh_arrays(flipped=S.FLIPPED)


def assert_equal_objects(got, want, who):
    assert sorted(got) == sorted(want)
    for k in got:
        assert (got[k] is None) == (want[k] is None), f"{who}: {k} is {'absent' if got[k] is None else 'present'}"
        if got[k] is not None:
            assert S.same(got[k], want[k]), f"{who}: {k} differs from the same operation on an object built from host arrays"


def run_cell(source, mutator, arrays, make, host, prepare=lambda o: o):
    """The values are held before the storage: where a mutator does reach the other object, the failure names the array that changed;
    sharing that this mutator does not exploit is caught by disjoint() after it."""
    # ---- B from A, B changed: A stays as it was, and B equals what an object of its own arrays becomes
    a = prepare(make(arrays))
    snap = S.snapshot(a)
    b = source.make(a)
    if source.same_object:
        assert b is a
    else:
        assert b is not a
        S.unchanged(a, snap)
    S.coherent(a), S.coherent(b)
    before = host(b)
    for k in source.equal:
        assert S.same(before[k], arrays[k]), f"{source.name}: {k} is not a's"
    prepare(b)
    mutator.apply(b)
    if not source.same_object:
        S.unchanged(a, snap)
        S.disjoint(a, b)
    S.coherent(a), S.coherent(b)
    fresh = prepare(make(before))
    mutator.apply(fresh)
    S.coherent(fresh)
    assert_equal_objects(host(b), host(fresh), f"{source.name} -> {mutator.name}")
    if isinstance(b, S.G.TriangleMesh):
        assert b.has_adjacency_list() == fresh.has_adjacency_list() and b.adjacency_list == fresh.adjacency_list
    if source.same_object:
        return
    # ---- the other way round: B from A, A changed
    a = prepare(make(arrays))
    b = prepare(source.make(a))
    snap = S.snapshot(b)
    mutator.apply(a)
    S.unchanged(b, snap)
    S.coherent(a), S.coherent(b)
    fresh = prepare(make(arrays))
    mutator.apply(fresh)
    assert_equal_objects(host(a), host(fresh), f"{mutator.name} on the source of {source.name}")
    S.disjoint(a, b)


CLOUD_CELLS = S.pairs(S.CLOUD_SOURCES, S.CLOUD_MUTATORS)
MESH_CELLS = S.pairs(S.MESH_SOURCES, S.MESH_MUTATORS)


@pytest.mark.parametrize("cell", sorted(CLOUD_CELLS))
def test_cloud_source_then_mutator(cell):
    run_cell(*CLOUD_CELLS[cell], cloud_h(), S.make_cloud, S.cloud_host)


@pytest.mark.parametrize("cell", sorted(MESH_CELLS))
def test_mesh_source_then_mutator(cell):
    """both meshes carry an adjacency list when the mutator arrives: whatever changes the triangles has to drop it"""
    run_cell(*MESH_CELLS[cell], mesh_h(), S.make_mesh, S.mesh_host, prepare=lambda m: m.compute_adjacency_list())


def test_flipped_mesh_gives_orient_triangles_work_to_do():
    """the matrix's mesh: orient_triangles turns its four flipped triangles, and their normals, back (triangle 0 keeps its winding)"""
    good, bad = S.mesh_arrays(), mesh_h()
    assert not S.same(good["triangles"], bad["triangles"])
    m = S.make_mesh(bad)
    assert m.orient_triangles() is True
    got = S.mesh_host(m)
    assert S.same(got["triangles"], good["triangles"]) and S.same(got["triangle_normals"], good["triangle_normals"])
    assert S.same(got["vertex_normals"], bad["vertex_normals"])


def test_sampled_cloud_shares_nothing_with_the_mesh():
    m = S.make_mesh(mesh_h())
    snap = S.snapshot(m)
    clouds = [m.sample_points_uniformly(300, seed=3), m.sample_points_uniformly(300, seed=3), m.sample_points_uniformly(77, use_triangle_normal=True)]
    for pc in clouds:
        S.disjoint(m, pc)
        S.coherent(pc)
    S.disjoint(clouds[0], clouds[1])
    S.unchanged(m, snap)
    keep = S.snapshot(clouds[1])
    clouds[0].transform(S.rigid()).normalize_normals()
    S.unchanged(m, snap), S.unchanged(clouds[1], keep)
    m.transform(S.rigid())
    m.orient_triangles()
    S.unchanged(clouds[1], keep)
    S.coherent(m), S.coherent(clouds[0])
    # a mesh without triangle normals gets them from use_triangle_normal=True, in the mesh: the one way this method changes its object
    bare = S.G.TriangleMesh(mesh_h()["vertices"], mesh_h()["triangles"])
    pc = bare.sample_points_uniformly(50, use_triangle_normal=True)
    assert bare.has_triangle_normals() and pc.has_normals()
    S.disjoint(bare, pc)


# ---- bare tensors are adopted ------------------------------------------------------------------------------------------------------------
def test_a_bare_tensor_is_adopted_and_written_in_place():
    import torch
    from kinectpy_amd import _lib as L
    h = cloud_h()
    want = S.cloud_host(S.make_cloud({"points": h["points"], "normals": h["normals"]}).transform(S.rigid()))
    for how in ("constructor", "setter"):
        t = torch.from_numpy(h["points"].copy()).to(L.device())
        n = torch.from_numpy(h["normals"].copy()).to(L.device())
        pc = S.G.PointCloud(t) if how == "constructor" else S.G.PointCloud()
        if how == "setter":
            pc.points = t
        pc.normals = n
        assert pc._pts.data_ptr() == t.data_ptr() and pc._nrm.data_ptr() == n.data_ptr(), how
        assert S.storage_of(pc) == {(x.untyped_storage().data_ptr(), x.untyped_storage().nbytes()) for x in (t, n)}
        pc.transform(S.rigid())
        assert S.same(t.cpu().numpy(), want["points"]) and S.same(n.cpu().numpy(), want["normals"]), f"{how}: transform writes the tensor it adopted"
        S.coherent(pc)
    tri = torch.from_numpy(mesh_h()["triangles"].copy()).to(L.device())
    vert = torch.from_numpy(mesh_h()["vertices"].copy()).to(L.device())
    m = S.G.TriangleMesh(vert, tri)
    assert m._vert.data_ptr() == vert.data_ptr() and m._tri.data_ptr() == tri.data_ptr()


def test_a_tensor_that_needs_converting_is_not_shared():
    import torch
    from kinectpy_amd import _lib as L
    h = cloud_h()
    f64 = torch.from_numpy(h["points"].astype(np.float64)).to(L.device())
    wide = torch.from_numpy(np.concatenate([h["points"], h["points"]], 1)).to(L.device())[:, :3]          # rows 24 bytes apart
    assert not wide.is_contiguous()
    host = torch.from_numpy(h["points"].copy())                                                             # right dtype, wrong device
    for t in (f64, wide, host):
        keep = t.cpu().numpy().copy()
        for pc in (S.G.PointCloud(t), S.G.PointCloud()):
            pc.points = t
            assert S.same(pc._pts.cpu().numpy(), h["points"])
            holder = type("Holder", (), {})()
            holder.t = t
            if t.is_cuda:
                S.disjoint(pc, holder)
            pc.transform(S.rigid())
            assert S.same(t.cpu().numpy(), keep)
            S.coherent(pc)
    tri64 = torch.from_numpy(mesh_h()["triangles"].astype(np.int64)).to(L.device())
    m = S.G.TriangleMesh(mesh_h()["vertices"], tri64)
    assert m._tri.dtype == torch.int32 and m._tri.data_ptr() != tri64.data_ptr()


def test_wrappers_are_copied_where_bare_tensors_are_adopted():
    """the two halves of the rule on one tensor: Vector3dVector(t) is copied on assignment, t itself adopted"""
    import torch
    from kinectpy_amd import _lib as L
    t = torch.from_numpy(cloud_h()["points"].copy()).to(L.device())
    adopted, copied = S.G.PointCloud(t), S.G.PointCloud(S.G.Vector3dVector(t))
    assert adopted._pts.data_ptr() == t.data_ptr()
    S.disjoint(adopted, copied)
    copied.transform(S.rigid())
    assert S.same(t.cpu().numpy(), cloud_h()["points"])
    img = S.G.Image(np.arange(12, dtype=np.float32).reshape(3, 4))
    again = S.G.Image(img)
    again.data[0, 0] = 99.0
    assert img.data[0, 0] == 0.0 and not np.shares_memory(img.data, again.data)


# ---- scenes answer for what they were given ---------------------------------------------------------------------------------------------
def second_mesh():
    h = S.mesh_arrays(levels=1, seed=9)
    h["vertices"] = h["vertices"] * np.float32(0.5) + np.float32([150.0, -40.0, 10.0])
    return h


@pytest.mark.parametrize("how", ["mesh", "mesh, rebuild for a second geometry", "device tensors", "device tensors, rebuild for a second geometry",
                                 "float64 host arrays"])
def test_scene_snapshot(how):
    import torch
    from kinectpy_amd import _lib as L
    h = mesh_h()
    scene = S.G.RaycastingScene()
    built = lambda: "rebuild" in how and S.coherent(scene)     # a first query: the later add_triangles finds a built scene to drop
    if how.startswith("mesh"):
        mesh = S.make_mesh(h)
        assert S.hand_over(scene, mesh) == 0
        kept = mesh
        built()
        mesh.transform(S.rigid())
        mesh.remove_triangles_by_index(list(range(64)))
    elif how.startswith("device"):
        v, t = torch.from_numpy(h["vertices"].copy()).to(L.device()), torch.from_numpy(h["triangles"].copy()).to(L.device())
        S.hand_over(scene, v, t)
        kept = type("Holder", (), {})()
        kept.v, kept.t = v, t
        built()
        v.mul_(3.0), t.copy_(t[:, [0, 2, 1]])
    else:
        v, t = h["vertices"].astype(np.float64), h["triangles"].astype(np.int64)
        S.hand_over(scene, v, t)
        kept = None
        v *= 3.0
        t[:] = 0
    if "rebuild" in how:
        assert scene._scene is not None
        other = S.make_mesh(second_mesh())
        assert S.hand_over(scene, other) == 1 and scene._scene is None                  # the rebuild takes the first geometry from what the scene kept
        other.transform(S.rigid())
    S.coherent(scene)
    fresh = S.fresh_scene(scene)
    rays = S.ray_fan(scene)
    q = rays[..., :3] + 0.25 * rays[..., 3:]
    for got, want in ((scene.compute_closest_points(q), fresh.compute_closest_points(q)),
                      ({"n": scene.count_intersections(rays)}, {"n": fresh.count_intersections(rays)}),
                      ({"d": scene.compute_signed_distance(q)}, {"d": fresh.compute_signed_distance(q)})):
        for k in want:
            assert S.same(got[k], want[k]), k
    n = fresh.count_intersections(rays)
    assert int(n.max()) >= 2                                   # a closed surface, entered and left: the fan does go through it
    if kept is not None:
        S.disjoint(scene, kept)
    if "rebuild" in how:
        assert set(np.unique(fresh.cast_rays(np.concatenate([rays.reshape(-1, 6), far_rays()]))["geometry_ids"])) >= {0, 1}


def far_rays():
    """rays from above onto the second mesh, so that both geometry ids are seen"""
    c = np.float64([10.0, 20.0, 30.0]) * 0.5 + np.float64([150.0, -40.0, 10.0])
    r = np.zeros((4, 6), dtype=np.float32)
    r[:, :3] = c + np.float64([0.0, 0.0, 500.0]) + np.float64([[1, 2, 0], [-3, 1, 0], [2, -2, 0], [0, 0, 0]])
    r[:, 5] = -1.0
    return r


def test_kdtree_answers_for_the_points_it_was_given():
    h = cloud_h()
    pc = S.make_cloud(h)
    tree = S.G.KDTreeFlann(pc)
    S.disjoint(tree, pc)
    snap = S.snapshot(tree)
    q = h["points"][:40] + np.float32(3.0)
    want = [x.cpu().numpy() for x in S.G.KDTreeFlann(h["points"].copy()).search_knn(q, 5)]
    pc.transform(S.rigid()).normalize_normals()
    pc += pc
    got = [x.cpu().numpy() for x in tree.search_knn(q, 5)]
    for g, w in zip(got, want):
        assert S.same(g, w)
    assert np.array_equal(got[0][:, 0], np.arange(40))
    S.unchanged(tree, snap)


# ---- volumes and grids ----------------------------------------------------------------------------------------------------------------------
W, H, K4 = 80, 72, (63.0, 63.0, 40.0, 36.0)


@functools.lru_cache(None)
def frame():
    """one frame of the synthetic ring of tests/tsdf_ref.py's suites: depth u16 (4, n_px), rgb u8 (4, n_px, 3), world -> camera"""
    from kinectpy_amd.utils import synth
    _, depth, rgb, _, _ = synth.sensor_ring(4, 1, synth.small_xy(8))
    return depth[0], rgb[0], np.stack([np.linalg.inv(synth.camera_pose(g, 4)) for g in range(4)])


def volume(kind):
    from kinectpy_amd import o3d
    ns = o3d.pipelines.integration
    if kind == "uniform":
        vol = ns.UniformTSDFVolume(2000.0, 32, 4.0 * 2000.0 / 32, ns.TSDFVolumeColorType.RGB8, (-1000.0, -1100.0, -1000.0))
    else:
        vol = ns.ScalableTSDFVolume(2000.0 / 32, 4.0 * 2000.0 / 32, ns.TSDFVolumeColorType.RGB8, 8, 3)
    depth, rgb, extr = frame()
    vol.integrate_frames(depth, rgb, o3d.camera.PinholeCameraIntrinsic(W, H, *K4), extr, 1.0, 6000.0)
    return vol


@pytest.mark.parametrize("kind", ["uniform", "scalable"])
@pytest.mark.parametrize("what", ["extract_point_cloud", "extract_voxel_point_cloud", "extract_triangle_mesh"])
def test_extractions_are_objects_of_their_own(kind, what):
    vol = volume(kind)
    snap = S.snapshot(vol)
    first, second = getattr(vol, what)(), getattr(vol, what)()
    host = S.mesh_host if what == "extract_triangle_mesh" else S.cloud_host
    rows = len(first.vertices if what == "extract_triangle_mesh" else first.points)
    assert rows > 100, rows
    S.disjoint(first, second), S.disjoint(first, vol), S.disjoint(second, vol)
    assert_equal_objects(host(first), host(second), what)
    keep = S.snapshot(second)
    first.transform(S.rigid())
    if what == "extract_triangle_mesh":
        first.compute_vertex_normals().remove_triangles_by_index([0, 1])
    elif first.has_normals():
        first.orient_normals_to_align_with_direction((0.0, 0.0, 1.0))
    S.unchanged(second, keep), S.unchanged(vol, snap)
    third = getattr(vol, what)()
    S.disjoint(third, [first, second, vol])
    assert_equal_objects(host(third), host(second), what)
    S.coherent(first), S.coherent(second), S.coherent(third)


def grid_and_camera():
    from kinectpy_amd import o3d
    h = cloud_h()
    grid = S.G.VoxelGrid.create_from_point_cloud(S.make_cloud(h), 40.0)
    cam = o3d.camera.PinholeCameraParameters(o3d.camera.PinholeCameraIntrinsic(64, 48, 60.0, 60.0, 32.0, 24.0))
    E = np.eye(4)
    E[2, 3] = 1500.0                                          # the camera 1.5 m in front of the cloud, looking along +z
    cam.extrinsic = E
    depth = np.zeros((48, 64), dtype=np.float32)
    depth[:, :32] = 1400.0                                    # a wall in front of the left half: those voxels go, the rest is unmeasured
    return grid, cam, depth


@pytest.mark.parametrize("how", ["VoxelGrid(other)", "copy.copy", "copy.deepcopy"])
def test_voxel_grid_copies_share_nothing(how):
    grid, cam, depth = grid_and_camera()
    snap = S.snapshot(grid)
    keys, col = grid._keys.cpu().numpy().copy(), grid._col.cpu().numpy().copy()
    dup = {"VoxelGrid(other)": S.G.VoxelGrid, "copy.copy": copy.copy, "copy.deepcopy": copy.deepcopy}[how](grid)
    S.disjoint(grid, dup)
    assert S.same(dup._keys.cpu().numpy(), keys) and S.same(dup._col.cpu().numpy(), col) and dup.origin is not grid.origin
    before = len(keys)
    assert dup.carve_depth_map(depth, cam, keep_voxels_outside_image=True, keep_unmeasured=True) is dup
    assert 0 < dup._count() < before, (dup._count(), before)
    S.unchanged(grid, snap)
    assert S.same(grid._keys.cpu().numpy(), keys) and S.same(grid._col.cpu().numpy(), col)
    dup.origin += 1.0
    assert S.same(grid.get_min_bound(), snap[0]["get_min_bound"])
    keep = S.snapshot(dup)
    grid.carve_depth_map(depth, cam, keep_voxels_outside_image=True, keep_unmeasured=True)          # and the other way round
    grid.clear()
    S.unchanged(dup, keep)


def test_voxel_grid_from_a_cloud_shares_nothing_with_it():
    h = cloud_h()
    pc = S.make_cloud(h)
    lo, hi = h["points"].min(0).astype(np.float64), h["points"].max(0).astype(np.float64)
    grids = [S.G.VoxelGrid.create_from_point_cloud(pc, 40.0), S.G.VoxelGrid.create_from_point_cloud_within_bounds(pc, 40.0, lo, hi),
             S.G.VoxelGrid.create_from_point_cloud(pc, 1.0)]          # one voxel per point: the colours are the cloud's, as copies
    assert grids[2]._count() == 257
    for g in grids:
        S.disjoint(g, pc)
    keep = [S.snapshot(g) for g in grids]
    pc.transform(S.rigid())
    pc.colors = h["colors"][::-1].copy()
    for g, k in zip(grids, keep):
        S.unchanged(g, k)
    snap = S.snapshot(pc)
    grids[0].clear()
    grids[1].origin += 5.0
    S.unchanged(pc, snap)


# ---- empty objects ------------------------------------------------------------------------------------------------------------------------
EMPTY_CLOUD_CALLS = {
    "PointCloud()": lambda e: S.G.PointCloud(),
    "PointCloud(e.points)": lambda e: S.G.PointCloud(e.points),
    "copy.copy": copy.copy, "copy.deepcopy": copy.deepcopy, "clone": lambda e: e.clone(),
    "e + e": lambda e: e + S.G.PointCloud(),
    "e += e": lambda e: e.__iadd__(S.G.PointCloud()),
    "select_by_index": lambda e: e.select_by_index([]),
    "remove_statistical_outlier": lambda e: e.remove_statistical_outlier(8, 2.0)[0],
    "remove_radius_outlier": lambda e: e.remove_radius_outlier(2, 10.0)[0],
    "farthest_point_down_sample": lambda e: e.farthest_point_down_sample(0),
    "voxel_down_sample": lambda e: e.voxel_down_sample(10.0),
    "transform": lambda e: e.transform(S.rigid()),
    "estimate_normals": lambda e: e.estimate_normals(),
    "estimate_covariances": lambda e: e.estimate_covariances(),
    "normalize_normals": lambda e: e.normalize_normals(),
    "orient_normals_to_align_with_direction": lambda e: e.orient_normals_to_align_with_direction(),
    "orient_normals_towards_camera_location": lambda e: e.orient_normals_towards_camera_location(),
    "orient_normals_consistent_tangent_plane": lambda e: e.orient_normals_consistent_tangent_plane(4),
    "points = []": lambda e: (setattr(e, "points", np.zeros((0, 3))), e)[1],
    "colors = []": lambda e: (setattr(e, "colors", np.zeros((0, 3))), e)[1],
    "normals = []": lambda e: (setattr(e, "normals", np.zeros((0, 3))), e)[1],
    "covariances = []": lambda e: (setattr(e, "covariances", np.zeros((0, 3, 3))), e)[1],
}


def test_the_empty_cloud_calls_are_the_classified_ones():
    names = {n for n, k in S.CLASSIFIED["PointCloud"].items() if k in ("returns_new", "mutates_self")}
    spelled = {"PointCloud()": "__init__", "PointCloud(e.points)": "__init__", "copy.copy": "__copy__", "copy.deepcopy": "__deepcopy__",
               "e + e": "__add__", "e += e": "__iadd__"}
    called = {spelled.get(n, n.split(" ")[0]) for n in EMPTY_CLOUD_CALLS}
    assert called <= names, called - names
    assert names == called


@pytest.mark.parametrize("call", sorted(EMPTY_CLOUD_CALLS))
def test_empty_cloud(call):
    h = cloud_h()
    e, witness = S.G.PointCloud(), S.G.PointCloud()
    other = S.make_cloud(h)
    snap = S.snapshot(other)
    r = EMPTY_CLOUD_CALLS[call](e)
    assert isinstance(r, S.G.PointCloud) and not r.has_points() and len(r.points) == 0
    assert not (r.has_colors() or r.has_normals() or r.has_covariances())
    assert S.same(r.get_min_bound(), np.zeros(3)) and S.same(r.get_max_bound(), np.zeros(3))
    kind = S.CLASSIFIED["PointCloud"].get(call.split(" ")[0])
    if kind == "mutates_self" or call == "e += e":
        assert r is e
    elif call not in ("PointCloud()",):
        assert r is not e
    for name in ("_cov", "_bounds", "_col", "_nrm"):           # nothing of the class itself is reachable from the result
        assert getattr(S.G.PointCloud, name, None) is None
    r += other                                                 # fill it: the result is the other cloud's equal and shares nothing with it
    assert_equal_objects(S.cloud_host(r), h, call)
    r.transform(S.rigid()).normalize_normals()
    S.unchanged(other, snap)
    S.disjoint(r, other), S.disjoint(r, witness)
    S.coherent(r), S.coherent(other)
    assert not witness.has_points() and not S.G.PointCloud().has_points()


def _oriented(e):
    assert e.orient_triangles() is True                       # no triangle contradicts another
    return e


def _no_sample(e):
    with pytest.raises(RuntimeError, match="no triangles"):   # the one call that is not legal without triangles, as in Open3D
        e.sample_points_uniformly(10)
    return e


EMPTY_MESH_RAISES = {"sample_points_uniformly"}
EMPTY_MESH_CALLS = {
    "TriangleMesh()": lambda e: S.G.TriangleMesh(),
    "TriangleMesh(e.vertices, e.triangles)": lambda e: S.G.TriangleMesh(e.vertices, e.triangles),
    "copy.copy": copy.copy, "copy.deepcopy": copy.deepcopy,
    "transform": lambda e: e.transform(S.rigid()),
    "compute_adjacency_list": lambda e: e.compute_adjacency_list(),
    "compute_triangle_normals": lambda e: e.compute_triangle_normals(),
    "compute_vertex_normals": lambda e: e.compute_vertex_normals(),
    "orient_triangles": _oriented,
    "select_by_index": lambda e: e.select_by_index([]),
    "select_by_index (no cleanup)": lambda e: e.select_by_index([], cleanup=False),
    "sample_points_uniformly": _no_sample,
    "remove_triangles_by_index": lambda e: e.remove_triangles_by_index([]),
    "remove_vertices_by_index": lambda e: e.remove_vertices_by_index([]),
    "remove_degenerate_triangles": lambda e: e.remove_degenerate_triangles(),
    "remove_triangles_by_mask": lambda e: e.remove_triangles_by_mask(np.zeros(0, dtype=bool)),
    "remove_vertices_by_mask": lambda e: e.remove_vertices_by_mask(np.zeros(0, dtype=bool)),
    "remove_unreferenced_vertices": lambda e: e.remove_unreferenced_vertices(),
    "filter_smooth_simple": lambda e: e.filter_smooth_simple(1),
    "filter_smooth_laplacian": lambda e: e.filter_smooth_laplacian(1),
    "filter_smooth_taubin": lambda e: e.filter_smooth_taubin(1),
    "vertices = []": lambda e: (setattr(e, "vertices", np.zeros((0, 3))), e)[1],
    "triangles = []": lambda e: (setattr(e, "triangles", np.zeros((0, 3), dtype=np.int32)), e)[1],
    "vertex_colors = []": lambda e: (setattr(e, "vertex_colors", np.zeros((0, 3))), e)[1],
    "vertex_normals = []": lambda e: (setattr(e, "vertex_normals", np.zeros((0, 3))), e)[1],
    "triangle_normals = []": lambda e: (setattr(e, "triangle_normals", np.zeros((0, 3))), e)[1],
}


def test_the_empty_mesh_calls_are_the_classified_ones():
    names = {n for n, k in S.CLASSIFIED["TriangleMesh"].items() if k in ("returns_new", "mutates_self")}
    spelled = {"TriangleMesh()": "__init__", "TriangleMesh(e.vertices,": "__init__", "copy.copy": "__copy__", "copy.deepcopy": "__deepcopy__"}
    called = {spelled.get(n.split(" ")[0], n.split(" ")[0]) for n in EMPTY_MESH_CALLS}
    assert names == called, (names - called, called - names)
    assert EMPTY_MESH_RAISES <= names


@pytest.mark.parametrize("call", sorted(EMPTY_MESH_CALLS))
def test_empty_mesh(call):
    """every call that returns or changes a mesh, on a mesh without vertices: an empty mesh, or self, comes back (or the call raises,
    where it is not legal), and filling the result touches no other object"""
    h = mesh_h()
    e = S.G.TriangleMesh()
    other = S.make_mesh(h)
    snap = S.snapshot(other)
    r = EMPTY_MESH_CALLS[call](e)
    assert isinstance(r, S.G.TriangleMesh) and r.is_empty() and not r.has_triangles() and len(r.vertices) == 0 and len(r.triangles) == 0
    assert not (r.has_vertex_colors() or r.has_vertex_normals() or r.has_triangle_normals() or r.has_adjacency_list()) and r.adjacency_list == []
    assert S.same(r.get_min_bound(), np.zeros(3))
    name = call.split(" ")[0]
    assert (r is e) == (S.CLASSIFIED["TriangleMesh"].get(name) == "mutates_self" or name in EMPTY_MESH_RAISES)
    for k in S.MESH_ATTRS:                                     # fill it from the other mesh's properties: copies, every one
        setattr(r, k, getattr(other, k))
    assert_equal_objects(S.mesh_host(r), h, call)
    r.transform(S.rigid())
    assert r.orient_triangles() is True
    S.unchanged(other, snap)
    S.disjoint(r, other)
    S.coherent(r), S.coherent(other)
    assert S.G.TriangleMesh._bounds is None and S.G.TriangleMesh._adj is None and S.G.TriangleMesh._adj_sets is None

"""Test infrastructure for the contracts of DESIGN.md 5.4a -- value semantics between geometry objects, snapshot at hand-over, cache
coherence.  Nothing here is a rounding question: every comparison is bit for bit.

  tensors_of / storage_of / disjoint   which device memory an object can reach, and that two objects reach none in common
  snapshot / unchanged                 host copies of every tensor plus the public answers, and their comparison
  coherent                             every cached answer against a recomputation from the object's current arrays
  CLASSIFIED                           every public callable of the seven classes: query / returns_new / mutates_self / off_path
  CLOUD_SOURCES, CLOUD_MUTATORS,       every way to obtain a cloud (mesh) B from A, every in-place operation; the GPU suite runs
  MESH_SOURCES, MESH_MUTATORS          their product, tests/test_object_state_cpu.py holds the registry to the classes

The module imports without a device; only calling the sources and mutators needs one."""
import collections
import copy
import weakref

import numpy as np
import torch

from kinectpy_amd import geometry as G
from kinectpy_amd import integration as I
from kinectpy_amd.utils import processing as P
from kinectpy_amd.preprocessing import fusion as F


# ---- reachability ------------------------------------------------------------------------------------------------------------------
def tensors_of(obj):
    """{path: tensor} of every torch.Tensor reachable through vars(obj) (PointCloud._pts_t included), looking into lists, tuples,
    dicts and the library's own plain holders (ops.SearchIndex, ops.RayScene)"""
    out, seen = {}, set()

    def walk(path, v):
        if isinstance(v, torch.Tensor):
            out[path] = v
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{path}[{i}]", x)
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(f"{path}[{k!r}]", x)
        elif hasattr(v, "__dict__") and type(v).__module__.startswith("kinectpy_amd") and id(v) not in seen:
            seen.add(id(v))
            for k, x in vars(v).items():
                walk(f"{path}.{k}" if path else k, x)

    seen.add(id(obj))
    for k, x in vars(obj).items():
        walk(k, x)
    return out


def storage_of(obj):
    """the set of (first byte, byte count) of the storages behind tensors_of(obj); a storage of no bytes is nobody's"""
    out = set()
    for t in tensors_of(obj).values():
        s = t.untyped_storage()
        if s.nbytes():
            out.add((s.data_ptr(), s.nbytes()))
    return out


def disjoint(a, b):
    """asserts that no storage reachable from a overlaps one reachable from b (either may be a list of objects)"""
    ranges = lambda o: set().union(*[storage_of(x) for x in (o if isinstance(o, (list, tuple)) else [o])])
    ra, rb = ranges(a), ranges(b)
    for pa, na in ra:
        for pb, nb in rb:
            assert pa + na <= pb or pb + nb <= pa, f"shared storage: [{pa:#x}, +{na}) and [{pb:#x}, +{nb})"
    return True


# ---- snapshots -----------------------------------------------------------------------------------------------------------------------
def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


ANSWERS = ("get_min_bound", "get_max_bound")


def _answers(obj):
    out = {}
    for name in dir(type(obj)):
        if name.startswith("has_") or name in ANSWERS or name == "is_empty":
            out[name] = getattr(obj, name)()
    for name in ("points", "vertices", "triangles"):
        if isinstance(getattr(type(obj), name, None), property):
            out[f"len({name})"] = len(getattr(obj, name))
    return out


def snapshot(obj):
    """(public answers, host copies of every tensor); the answers come first, so the bounds they cache are part of the copies"""
    answers = _answers(obj)
    return answers, {k: t.detach().cpu().numpy().copy() for k, t in tensors_of(obj).items()}


def unchanged(obj, snap):
    answers, arrays = snapshot(obj)
    assert sorted(answers) == sorted(snap[0]) and sorted(arrays) == sorted(snap[1]), (sorted(arrays), sorted(snap[1]))
    for k, v in answers.items():
        assert same(np.asarray(v), np.asarray(snap[0][k])), f"{type(obj).__name__}.{k}() changed: {snap[0][k]} -> {v}"
    for k, v in arrays.items():
        assert same(v, snap[1][k]), f"{type(obj).__name__}.{k} changed"
    return True


# ---- scenes: what was handed over ----------------------------------------------------------------------------------------------------
_HANDED = weakref.WeakKeyDictionary()


def _host(x):
    return x.detach().cpu().numpy().copy() if isinstance(x, torch.Tensor) else np.array(x)


def hand_over(scene, vertices, triangles=None):
    """scene.add_triangles(...), remembering host copies of the arrays as they are at this moment"""
    pair = (_host(vertices._vert), _host(vertices._tri)) if isinstance(vertices, G.TriangleMesh) else (_host(vertices), _host(triangles))
    _HANDED.setdefault(scene, []).append(pair)
    return scene.add_triangles(vertices, triangles)


def fresh_scene(scene):
    """a new scene of the host arrays remembered for `scene`"""
    s = G.RaycastingScene()
    for v, t in _HANDED.get(scene, []):
        s.add_triangles(v.copy(), t.copy())
    return s


def ray_fan(scene):
    """64 rays, float32 (8, 8, 6): from one point outside the remembered geometries' box towards an 8 x 8 grid across it"""
    pairs = _HANDED.get(scene, [])
    v = np.concatenate([p[0].astype(np.float64) for p in pairs]) if pairs else np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    lo, hi = v.min(0), v.max(0)
    mid, ext = (lo + hi) * 0.5, float((hi - lo).max()) + 1.0
    eye = mid + np.array([0.25, -0.5, 3.0]) * ext
    u, w = np.meshgrid(np.linspace(-0.6, 0.6, 8), np.linspace(-0.6, 0.6, 8))
    target = mid[None, None, :] + np.stack([u * ext, w * ext, np.zeros_like(u)], 2)
    rays = np.empty((8, 8, 6))
    rays[..., :3], rays[..., 3:] = eye, target - eye
    return rays.astype(np.float32)


# ---- coherence -------------------------------------------------------------------------------------------------------------------------
def coherent(obj):
    """every cached answer of obj equals its recomputation from the object's current arrays, exactly"""
    if isinstance(obj, (G.PointCloud, G.TriangleMesh)):
        pts = (obj._pts if isinstance(obj, G.PointCloud) else obj._vert).detach().cpu().numpy().astype(np.float64)
        lo, hi = (pts.min(0), pts.max(0)) if len(pts) else (np.zeros(3), np.zeros(3))
        assert same(obj.get_min_bound(), lo), (obj.get_min_bound(), lo)
        assert same(obj.get_max_bound(), hi), (obj.get_max_bound(), hi)
        if obj._bounds is not None and len(pts):
            assert same(obj._bounds.cpu().numpy(), np.concatenate([lo, hi]))
    if isinstance(obj, G.TriangleMesh):
        if obj.has_adjacency_list():
            want = [set() for _ in range(len(pts))]
            for a, b, c in obj._tri.cpu().numpy().tolist():
                want[a] |= {b, c}
                want[b] |= {a, c}
                want[c] |= {a, b}
            assert obj.adjacency_list == want
    if isinstance(obj, G.RaycastingScene):
        rays = ray_fan(obj)
        got, want = obj.cast_rays(rays), fresh_scene(obj).cast_rays(rays)
        assert sorted(got) == sorted(want)
        for k in got:
            assert same(got[k], want[k]), f"cast_rays[{k!r}] differs from a scene of the arrays as they were handed over"
        if _HANDED.get(obj):
            assert np.isfinite(want["t_hit"]).sum() >= 4, "the fan misses the geometry: the comparison would say nothing"
    return True


# ---- classification ----------------------------------------------------------------------------------------------------------------------
KINDS = ("query", "returns_new", "mutates_self", "off_path")
OPERATORS = ("__init__", "__add__", "__iadd__", "__copy__", "__deepcopy__")          # classified where the class defines them
CLASSES = {"PointCloud": G.PointCloud, "TriangleMesh": G.TriangleMesh, "VoxelGrid": G.VoxelGrid, "RaycastingScene": G.RaycastingScene,
           "KDTreeFlann": G.KDTreeFlann, "UniformTSDFVolume": I.UniformTSDFVolume, "ScalableTSDFVolume": I.ScalableTSDFVolume}


def _kinds(query="", returns_new="", mutates_self="", off_path=""):
    out = {}
    for kind, names in zip(KINDS, (query, returns_new, mutates_self, off_path)):
        for n in names.split():
            assert n not in out, n
            out[n] = kind
    return out


# a property with a setter is classified by its setter
CLASSIFIED = {
    "PointCloud": _kinds(
        query="has_points has_colors has_normals has_covariances get_min_bound get_max_bound cluster_dbscan segment_plane "
              "compute_point_cloud_distance compute_nearest_neighbor_distance get_oriented_bounding_box",
        returns_new="__init__ __add__ __copy__ __deepcopy__ clone select_by_index voxel_down_sample remove_statistical_outlier "
                    "remove_radius_outlier farthest_point_down_sample",
        mutates_self="points colors normals covariances __iadd__ transform estimate_normals estimate_covariances normalize_normals "
                     "orient_normals_to_align_with_direction orient_normals_towards_camera_location orient_normals_consistent_tangent_plane"),
    "TriangleMesh": _kinds(
        query="has_vertices has_triangles has_vertex_colors has_vertex_normals has_triangle_normals is_empty get_surface_area get_min_bound "
              "get_max_bound has_adjacency_list adjacency_list get_non_manifold_edges is_edge_manifold cluster_connected_triangles "
              "get_non_manifold_vertices is_vertex_manifold get_self_intersecting_triangles is_self_intersecting is_intersecting is_orientable "
              "get_volume euler_poincare_characteristic",
        returns_new="__init__ __copy__ __deepcopy__ select_by_index filter_smooth_simple filter_smooth_laplacian filter_smooth_taubin "
                    "sample_points_uniformly",
        mutates_self="vertices triangles vertex_colors vertex_normals triangle_normals transform compute_triangle_normals compute_vertex_normals "
                     "compute_adjacency_list orient_triangles remove_triangles_by_mask remove_triangles_by_index remove_degenerate_triangles "
                     "remove_vertices_by_mask remove_vertices_by_index remove_unreferenced_vertices"),
    "VoxelGrid": _kinds(
        query="has_voxels has_colors is_empty voxel_indices voxel_colors get_voxels get_voxel get_voxel_center_coordinate get_voxel_bounding_points "
              "get_min_bound get_max_bound get_center included_mask check_if_included",
        returns_new="__init__ __copy__ __deepcopy__ create_from_point_cloud create_from_point_cloud_within_bounds create_dense",
        mutates_self="clear carve_depth_map carve_silhouette carve_depth_maps carve_silhouettes",
        off_path="create_from_triangle_mesh create_from_triangle_mesh_within_bounds create_from_octree to_octree add_voxel remove_voxel"),
    "RaycastingScene": _kinds(
        query="cast_rays test_occlusions count_intersections compute_closest_points compute_distance compute_occupancy compute_signed_distance "
              "create_rays_pinhole",
        returns_new="__init__", mutates_self="add_triangles"),
    "KDTreeFlann": _kinds(
        query="search_knn search_radius search_hybrid search_knn_vector_3d search_hybrid_vector_3d search_radius_vector_3d search_vector_3d",
        returns_new="__init__", mutates_self="set_geometry"),
    "UniformTSDFVolume": _kinds(
        returns_new="__init__ extract_point_cloud extract_voxel_point_cloud extract_triangle_mesh", mutates_self="reset integrate integrate_frames"),
    "ScalableTSDFVolume": _kinds(
        query="volume_unit_count volume_unit_indices unit_arrays",
        returns_new="__init__ extract_point_cloud extract_voxel_point_cloud extract_triangle_mesh", mutates_self="reset integrate integrate_frames"),
}
# returns_new / mutates_self callables that the source x mutator matrix does not reach, and the test of the GPU suite that does
ELSEWHERE = {
    "TriangleMesh": {"sample_points_uniformly": "test_sampled_cloud_shares_nothing_with_the_mesh"},
}


def public_names(cls):
    """the public methods and properties of cls, and the operators of OPERATORS it defines itself"""
    out = set()
    for name in dir(cls):
        attr = getattr(cls, name)
        if not name.startswith("_") and (callable(attr) or isinstance(attr, property)):
            out.add(name)
    return out | {n for n in OPERATORS if n in vars(cls)}


# ---- fixtures: host arrays -------------------------------------------------------------------------------------------------------------
def rigid():
    """a rotation by 0.7 rad round (1, 2, 3) with a translation larger than either fixture: it moves every bound"""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(0.7) * K + (1.0 - np.cos(0.7)) * (K @ K)
    T[:3, 3] = (1000.0, -2000.0, 1500.0)
    return T


def cloud_arrays(seed=0, n=257):
    """n points -- 257: one past a 256-thread block -- on distinct integer millimetres of [-400, 400]^3, colours, unit normals (rows
    5, 100 and the last are zero), symmetric positive definite covariances"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(81 ** 3, n, replace=False)
    pts = (np.stack([cells // 6561, (cells // 81) % 81, cells % 81], 1) * 10 - 400).astype(np.float32)
    col = rng.random((n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[[5 % n, 100 % n, n - 1]] = 0.0
    a = rng.normal(size=(n, 3, 3))
    cov = a @ a.transpose(0, 2, 1) + 0.5 * np.eye(3)
    return {"points": pts, "colors": col, "normals": nrm, "covariances": cov}


CLOUD_ATTRS = ("points", "colors", "normals", "covariances")


def make_cloud(arrays):
    """a cloud built from host arrays alone (None: attribute absent)"""
    pc = G.PointCloud(arrays["points"].copy())
    for k in CLOUD_ATTRS[1:]:
        if arrays.get(k) is not None:
            setattr(pc, k, arrays[k].copy())
    return pc


def cloud_host(pc):
    on = {"points": True, "colors": pc.has_colors(), "normals": pc.has_normals(), "covariances": pc.has_covariances()}
    t = {"points": pc._pts, "colors": pc._col, "normals": pc._nrm, "covariances": pc._cov}
    return {k: _host(t[k]) if on[k] else None for k in CLOUD_ATTRS}


def mesh_arrays(levels=2, flipped=(), seed=1):
    """an octahedron subdivided `levels` times on the sphere of radius 100 round (10, 20, 30): 66 vertices and 128 triangles at
    level 2, closed and outward; vertex colours, unit vertex normals, triangle normals; `flipped` triangles have their winding (and
    their normal) reversed"""
    v = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, nt = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = np.asarray(v[a]) + np.asarray(v[b])
                v.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        t = nt
    unit = np.asarray(v, dtype=np.float64)
    vert = (unit * 100.0 + np.array([10.0, 20.0, 30.0])).astype(np.float32)
    tri = np.asarray(t, dtype=np.int32)
    flipped = list(flipped)
    tri[flipped] = tri[flipped][:, [0, 2, 1]]
    p = vert.astype(np.float64)
    tn = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    tn = (tn / np.linalg.norm(tn, axis=1, keepdims=True)).astype(np.float32)
    rng = np.random.default_rng(seed)
    return {"vertices": vert, "triangles": tri, "vertex_colors": rng.random((len(vert), 3)).astype(np.float32),
            "vertex_normals": unit.astype(np.float32), "triangle_normals": tn}


MESH_ATTRS = ("vertices", "triangles", "vertex_colors", "vertex_normals", "triangle_normals")
FLIPPED = (3, 10, 50, 127)


def make_mesh(arrays):
    m = G.TriangleMesh(arrays["vertices"].copy(), arrays["triangles"].copy())
    for k in MESH_ATTRS[2:]:
        if arrays.get(k) is not None:
            setattr(m, k, arrays[k].copy())
    return m


def mesh_host(m):
    on = {"vertices": True, "triangles": True, "vertex_colors": m.has_vertex_colors(), "vertex_normals": m.has_vertex_normals(),
          "triangle_normals": m.has_triangle_normals()}
    t = {"vertices": m._vert, "triangles": m._tri, "vertex_colors": m._vcol, "vertex_normals": m._vnrm, "triangle_normals": m._tnrm}
    return {k: _host(t[k]) if on[k] else None for k in MESH_ATTRS}


# ---- registry: sources and mutators -----------------------------------------------------------------------------------------------------
# Source.make(a) -> b.  uses: the classified callables it goes through; carries: the attributes b is sure to have (a mutator that needs
# another is not paired with it); equal: the attributes of b that must equal a's bit for bit; same_object: b is a (an in-place helper)
Source = collections.namedtuple("Source", "name uses make carries equal same_object", defaults=((), False))
# Mutator.apply(obj): deterministic, legal on any object that has `needs`
Mutator = collections.namedtuple("Mutator", "name uses apply needs", defaults=((),))
ALL4, PCN = CLOUD_ATTRS, CLOUD_ATTRS[:3]


def _assigned(attr, attrs, make, arrays):
    def f(a):
        b = make(arrays())               # an object of its own, of the same size, with every attribute
        setattr(b, attr, getattr(a, attr))
        return b
    return f


def _other_cloud():
    h = cloud_arrays(seed=7)
    return {k: h[k][::-1].copy() for k in h}


def _iadd_into_empty(a):
    e = G.PointCloud()
    e += a
    return e


def _first(x):
    return x[0]


CLOUD_SOURCES = [Source(f"b.{k} = a.{k}", (k,), _assigned(k, CLOUD_ATTRS, make_cloud, _other_cloud), ALL4, (k,)) for k in CLOUD_ATTRS] + [
    Source("PointCloud(a.points)", ("__init__", "points"), lambda a: G.PointCloud(a.points), ("points",), ("points",)),
    Source("copy.copy(a)", ("__copy__",), copy.copy, ALL4, ALL4),
    Source("copy.deepcopy(a)", ("__deepcopy__",), copy.deepcopy, ALL4, ALL4),
    Source("a.clone()", ("clone",), lambda a: a.clone(), ALL4, ALL4),
    Source("a + e", ("__add__",), lambda a: a + G.PointCloud(), ("points",), ("points",)),
    Source("e + a", ("__add__",), lambda a: G.PointCloud() + a, ALL4, ALL4),
    Source("e += a", ("__iadd__",), _iadd_into_empty, ALL4, ALL4),
    Source("a + a", ("__add__",), lambda a: a + a, ALL4),
    Source("select_by_index(all)", ("select_by_index",), lambda a: a.select_by_index(np.arange(len(a.points))), PCN, PCN),
    Source("select_by_index([], invert)", ("select_by_index",), lambda a: a.select_by_index([], invert=True), PCN, PCN),
    Source("_select(all)", ("_select",), lambda a: a._select(torch.arange(len(a.points), dtype=torch.int32, device=a._pts.device)), PCN, PCN),
    Source("voxel_down_sample(1 point per voxel)", ("voxel_down_sample",), lambda a: a.voxel_down_sample(1.0), PCN),
    Source("remove_statistical_outlier(keeps all)", ("remove_statistical_outlier",), lambda a: _first(a.remove_statistical_outlier(8, 1e6)), PCN, PCN),
    Source("remove_radius_outlier(keeps all)", ("remove_radius_outlier",), lambda a: _first(a.remove_radius_outlier(1, 1e4)), PCN, PCN),
    Source("farthest_point_down_sample(100)", ("farthest_point_down_sample",), lambda a: a.farthest_point_down_sample(100), PCN),
    Source("farthest_point_down_sample(all)", ("farthest_point_down_sample",), lambda a: a.farthest_point_down_sample(len(a.points)), ALL4, ALL4),
    Source("scale_point_cloud", ("processing.scale_point_cloud",), lambda a: P.scale_point_cloud(a, 0.5, 2.0, 0.25), ALL4, CLOUD_ATTRS[1:]),
    Source("normalize_pointcloud", ("processing.normalize_pointcloud",), lambda a: P.normalize_pointcloud(a), ALL4, same_object=True),
]


def _iadd_other(b):
    b += make_cloud(cloud_arrays(seed=11, n=33))
    return b


def _set_cloud(attr):
    def f(b):
        n = len(b.points)
        setattr(b, attr, cloud_arrays(seed=13, n=n)[attr])
    return f


CLOUD_MUTATORS = [
    Mutator("transform", ("transform",), lambda b: b.transform(rigid())),
    Mutator("normalize_normals", ("normalize_normals",), lambda b: b.normalize_normals(), ("normals",)),
    Mutator("orient_normals_to_align_with_direction", ("orient_normals_to_align_with_direction",),
            lambda b: b.orient_normals_to_align_with_direction((0.0, 1.0, 0.0)), ("normals",)),
    Mutator("orient_normals_towards_camera_location", ("orient_normals_towards_camera_location",),
            lambda b: b.orient_normals_towards_camera_location((50.0, -30.0, 20.0)), ("normals",)),
    Mutator("orient_normals_consistent_tangent_plane", ("orient_normals_consistent_tangent_plane",),
            lambda b: b.orient_normals_consistent_tangent_plane(6), ("normals",)),
    Mutator("orient_normals_to_sensors", ("fusion.orient_normals_to_sensors",), lambda b: F.orient_normals_to_sensors([b], [rigid()]), ("normals",)),
    Mutator("estimate_normals", ("estimate_normals",), lambda b: b.estimate_normals(G.KDTreeSearchParamKNN(8))),
    Mutator("estimate_covariances", ("estimate_covariances",), lambda b: b.estimate_covariances(G.KDTreeSearchParamKNN(8))),
    Mutator("+=", ("__iadd__",), _iadd_other),
    Mutator("normalize_pointcloud", ("processing.normalize_pointcloud",), lambda b: P.normalize_pointcloud(b)),
] + [Mutator(f"{k} = array", (k,), _set_cloud(k)) for k in CLOUD_ATTRS]

VT = MESH_ATTRS[:2]
ALL5 = MESH_ATTRS
_other_mesh = lambda: mesh_arrays(seed=5)
_all_vertices = lambda a: np.arange(len(a.vertices))

MESH_SOURCES = [Source(f"m2.{k} = m1.{k}", (k,), _assigned(k, MESH_ATTRS, make_mesh, _other_mesh), ALL5, (k,)) for k in MESH_ATTRS] + [
    Source("TriangleMesh(m.vertices, m.triangles)", ("__init__", "vertices", "triangles"), lambda a: G.TriangleMesh(a.vertices, a.triangles), VT, VT),
    Source("copy.copy(m)", ("__copy__",), copy.copy, ALL5, ALL5),
    Source("copy.deepcopy(m)", ("__deepcopy__",), copy.deepcopy, ALL5, ALL5),
    Source("select_by_index(all, cleanup)", ("select_by_index",), lambda a: a.select_by_index(_all_vertices(a), True), ALL5, ALL5),
    Source("select_by_index(all, no cleanup)", ("select_by_index",), lambda a: a.select_by_index(_all_vertices(a), False), ALL5, ALL5),
    Source("filter_smooth_simple", ("filter_smooth_simple",), lambda a: a.filter_smooth_simple(1), MESH_ATTRS[:4], ("triangles",)),
    Source("filter_smooth_laplacian(Color)", ("filter_smooth_laplacian",), lambda a: a.filter_smooth_laplacian(2, 0.5, G.FilterScope.Color),
           MESH_ATTRS[:4], ("vertices", "triangles", "vertex_normals")),
    Source("filter_smooth_taubin(Vertex)", ("filter_smooth_taubin",), lambda a: a.filter_smooth_taubin(1, 0.5, -0.53, G.FilterScope.Vertex),
           MESH_ATTRS[:4], ("triangles", "vertex_colors", "vertex_normals")),
]


def _mask(n, every):
    m = np.zeros(n, dtype=bool)
    m[::every] = True
    return m


def _set_mesh(attr):
    def f(b):
        h = mesh_arrays(flipped=(1, 2), seed=17)
        if attr in ("vertices", "triangles"):
            assert len(b.vertices) == len(h["vertices"])           # the setters are tried on meshes that kept every vertex
        rows = len(b.triangles) if attr == "triangle_normals" else len(b.vertices)
        setattr(b, attr, h[attr] if attr == "triangles" else h[attr][:rows] * np.float32(0.5))
    return f


MESH_MUTATORS = [
    Mutator("transform", ("transform",), lambda b: b.transform(rigid())),
    Mutator("orient_triangles", ("orient_triangles",), lambda b: b.orient_triangles()),
    Mutator("compute_triangle_normals", ("compute_triangle_normals",), lambda b: b.compute_triangle_normals()),
    Mutator("compute_vertex_normals", ("compute_vertex_normals",), lambda b: b.compute_vertex_normals()),
    Mutator("compute_adjacency_list", ("compute_adjacency_list",), lambda b: b.compute_adjacency_list()),
    Mutator("remove_triangles_by_mask", ("remove_triangles_by_mask",), lambda b: b.remove_triangles_by_mask(_mask(len(b.triangles), 3))),
    Mutator("remove_triangles_by_index", ("remove_triangles_by_index",), lambda b: b.remove_triangles_by_index([0, 7, 7, len(b.triangles) - 1])),
    Mutator("remove_degenerate_triangles", ("remove_degenerate_triangles", "triangles"),
            lambda b: (setattr(b, "triangles", np.concatenate([[[0, 0, 1]], np.asarray(b.triangles)[1:]])), b.remove_degenerate_triangles())),
    Mutator("remove_vertices_by_mask", ("remove_vertices_by_mask",), lambda b: b.remove_vertices_by_mask(_mask(len(b.vertices), 5))),
    Mutator("remove_vertices_by_index", ("remove_vertices_by_index",), lambda b: b.remove_vertices_by_index([2, 3, len(b.vertices) - 1])),
    Mutator("remove_unreferenced_vertices", ("remove_unreferenced_vertices", "remove_triangles_by_index"),
            lambda b: b.remove_triangles_by_index(list(range(0, 40))).remove_unreferenced_vertices()),
] + [Mutator(f"{k} = array", (k,), _set_mesh(k)) for k in MESH_ATTRS]

# names in `uses` that are no method of the class: the helpers of DESIGN.md 5.4a's list
HELPERS = {"_select": G.PointCloud._select, "processing.scale_point_cloud": P.scale_point_cloud,
           "processing.normalize_pointcloud": P.normalize_pointcloud, "fusion.orient_normals_to_sensors": F.orient_normals_to_sensors}


def pairs(sources, mutators):
    """the legal cells of the matrix as pytest ids -> (source, mutator): the mutator's needs are among what the source carries"""
    return {f"{s.name} -> {m.name}": (s, m) for s in sources for m in mutators if set(m.needs) <= set(s.carries)}

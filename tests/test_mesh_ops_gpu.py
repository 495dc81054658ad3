"""GPU suite of the mesh clean-up (kpx_mesh.hip; AC13): every device result -- adjacency, non-manifold edges, clusters with their
counts and areas, ordered removal, smoothing, uniform samples -- bit for bit against the serial restatement tests/mesh_ops_ref.py.
The meshes are built on the host by tests/tsdf_mesh_ref.py from the random volumes of test_tsdf_mesh_gpu.random_case (restated
here), plus a closed sphere, truncated triangle lists and hand-built cases that sit on the kernels' edges."""
import functools

import numpy as np
import pytest

import mesh_ops_ref as R
import tsdf_mesh_ref as M

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(None)
def random_mesh(res):
    """test_tsdf_mesh_gpu.random_case's volume, meshed on the host -> vertices, colours in [0, 1], triangles.
    res 8: 429 vertices, 458 triangles, 26 clusters; 13: 2083, 2408, 89; 24: 13918, 16548, 576 (several 2048-item compaction tiles)"""
    rng = np.random.default_rng(1000 + res)
    n = res ** 3
    f = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    where = rng.random(n) < 0.08
    f[where] = special[rng.integers(0, 4, int(where.sum()))]
    w = np.where(rng.random(n) < 0.1, 0.0, rng.integers(1, 9, n)).astype(np.float32)
    c = rng.uniform(0.0, 255.0, (n, 3)).astype(np.float32)
    return M.extract_triangle_mesh(f, w, c, res, (res * 0.013) / res, np.array((-0.37, 1.91, 12.3)))[:3]


@functools.lru_cache(None)
def sphere():
    f, w = M.sphere_volume()
    v, _, t, _ = M.extract_triangle_mesh(f, w, None, 16, 1.0, (0.0, 0.0, 0.0))
    return v, np.random.default_rng(9).random(v.shape).astype(np.float32), t


@functools.lru_cache(None)
def case(name):
    """-> vertices float32 (V, 3), colours float32 (V, 3), triangles int32 (T, 3); treat as read-only"""
    if name == "sphere":
        return sphere()
    kind, _, arg = name.partition("-")
    if kind == "res":
        return random_mesh(int(arg))
    if kind == "cut":                                        # the first n triangles: unreferenced and isolated vertices remain
        res, n = arg.split("-")
        v, c, t = random_mesh(int(res))
        return v, c, np.ascontiguousarray(t[:int(n)])
    rng = np.random.default_rng(77)
    if name == "book":                                       # five triangles on one edge: a run of five equal keys
        v, t = rng.random((7, 3)), [[0, 1, 2 + k] for k in range(5)]
    elif name == "bowtie":                                   # two triangles that share one vertex and no edge
        v, t = rng.random((5, 3)), [[0, 1, 2], [2, 3, 4]]
    elif name == "strip":                                    # 5000 triangles in a row, their indices shuffled: deep union-find paths
        x = np.arange(5002)
        v = np.stack([x * 0.5, (x % 2) + 0.1 * rng.random(5002), 0.05 * rng.random(5002)], 1)
        t = np.stack([x[:-2], x[1:-1], x[2:]], 1)[rng.permutation(5000)]
    elif name == "degenerate":                               # repeated indices, collinear corners, a repeated triangle, an unused vertex
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [1, 1, 0.5], [3, 3, 3], [0.5, 0.5, 2]])
        t = [[0, 1, 3], [0, 1, 2], [1, 1, 4], [1, 4, 2], [4, 4, 4], [0, 1, 2], [2, 6, 2], [1, 2, 4]]
    elif name == "disjoint":                                 # 70 000 triangles that share nothing: 70 000 roots, 35 compaction tiles
        v = rng.random((210000, 3)) * 4.0
        t = np.arange(210000).reshape(-1, 3)
    elif name == "one":
        v, t = rng.random((3, 3)), [[0, 1, 2]]
    elif name == "point":                                    # one vertex, one triangle that names it three times
        v, t = rng.random((1, 3)), [[0, 0, 0]]
    elif name == "bare":                                     # one vertex, no triangle
        v, t = rng.random((1, 3)), np.zeros((0, 3))
    elif name == "empty":
        v, t = np.zeros((0, 3)), np.zeros((0, 3))
    else:
        raise KeyError(name)
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    return v, np.random.default_rng(len(v)).random(v.shape).astype(np.float32), np.asarray(t, dtype=np.int32).reshape(-1, 3)


def build(v, t, c=None, vn=None, tn=None):
    from kinectpy_amd import o3d
    mesh = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(v), o3d.utility.Vector3iVector(t))
    for name, a in (("vertex_colors", c), ("vertex_normals", vn), ("triangle_normals", tn)):
        if a is not None:
            setattr(mesh, name, o3d.utility.Vector3dVector(a))
    return mesh


def attributes(mesh):
    return tuple(host(a) for a in (mesh._vert, mesh._vcol, mesh._vnrm, mesh._tri, mesh._tnrm))


def assert_rows(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is None or (g is None and len(w) == 0):         # an attribute without rows reads as absent
            assert g is None or len(g) == 0
        else:
            assert same(g, np.ascontiguousarray(w)), (g.shape, w.shape)


def normals_of(v, t):
    """float32 per-vertex and per-triangle rows to carry along (any values do)"""
    return M.vertex_normals(v, t), M.triangle_normals(v, t)


def check_topology(v, t):
    mesh = build(v, t)
    assert not mesh.has_adjacency_list() and mesh.adjacency_list == []
    assert mesh.compute_adjacency_list() is mesh and mesh.has_adjacency_list() == (len(v) > 0)          # Open3D: none without vertices
    off, nb = (host(a) for a in mesh._adj)
    roff, rnb = R.adjacency(t, len(v))
    assert same(off, roff) and same(nb, rnb)
    sets = mesh.adjacency_list
    assert len(sets) == len(v) and all(isinstance(s, set) for s in sets)
    for i in (0, len(v) // 2, len(v) - 1) if len(v) else ():
        assert sets[i] == set(rnb[roff[i]:roff[i + 1]].tolist())
    for allow in (True, False):
        e = np.asarray(mesh.get_non_manifold_edges(allow))
        want = R.non_manifold_edges(t, allow)
        assert e.dtype == np.int32 and np.array_equal(e.reshape(-1, 2), want)
        assert mesh.is_edge_manifold(allow) == (len(want) == 0)
    lab, num, area = (host(a) for a in mesh.cluster_connected_triangles())
    rlab, rnum, rarea = R.cluster_connected_triangles(v, t)
    assert same(lab, rlab) and same(num, rnum) and same(area, rarea), (len(num), len(rnum))
    return rlab, rnum


def check_removal(v, c, t, seed=0):
    vn, tn = normals_of(v, t)
    rng = np.random.default_rng(seed)
    tmask, vmask = rng.random(len(t)) < 0.4, rng.random(len(v)) < 0.2
    mesh = build(v, t, c, vn, tn)
    assert mesh.remove_triangles_by_mask(tmask) is mesh
    t2, tn2 = R.remove_triangles(t, tmask, tn)
    assert_rows(attributes(mesh), (v, c, vn, t2, tn2))
    assert mesh.remove_vertices_by_mask(vmask) is mesh
    want = R.remove_vertices(v, t2, vmask, c, vn, tn2)
    assert_rows(attributes(mesh), (want[0], want[1], want[2], want[3], want[4]))
    assert mesh.remove_unreferenced_vertices() is mesh
    v3, c3, n3, t3, tn3 = want
    final = R.remove_vertices(v3, t3, ~R.referenced(t3, len(v3)), c3, n3, tn3)
    assert_rows(attributes(mesh), final)
    if len(final[3]):
        assert R.referenced(final[3], len(final[0])).all()


def check_smoothing(v, c, t):
    vn, _ = normals_of(v, t)
    for method, call in (("simple", lambda m: m.filter_smooth_simple(1)), ("laplacian", lambda m: m.filter_smooth_laplacian(1)),
                         ("taubin", lambda m: m.filter_smooth_taubin(1))):
        src = build(v, t, c, vn)
        out = call(src)
        rv, rn, rc = R.smooth(v, t, method, 1, normals=vn, colors=c)
        assert out is not src and not out.has_triangle_normals() and np.array_equal(host(out._tri), t)
        assert_rows((host(out._vert), host(out._vnrm), host(out._vcol)), (rv, rn, rc))
        assert same(host(src._vert), v)                      # the source is left alone


def check_sampling(v, c, t, n=65):
    if len(t) == 0 or not R.triangle_areas(v, t).sum() > 0.0:
        mesh = build(v, t, c)
        with pytest.raises(RuntimeError, match="no triangles" if len(t) == 0 else "no surface area"):
            mesh.sample_points_uniformly(n)
        return
    vn, _ = normals_of(v, t)
    pc = build(v, t, c, vn).sample_points_uniformly(n, seed=5)
    rp, rc, rn, _ = R.sample_points_uniformly(v, t, n, 5, colors=c, vertex_normals=vn)
    assert_rows((host(pc._pts), host(pc._col), host(pc._nrm)), (rp, rc, rn))


ALL = ["res-8", "res-13", "res-24", "sphere", "cut-13-2047", "cut-13-2048", "cut-13-2049", "cut-24-2047", "cut-24-2048", "cut-24-2049", "book",
       "bowtie", "strip", "degenerate", "disjoint", "one", "point", "bare", "empty"]


@pytest.mark.parametrize("name", ALL)
def test_topology(name):
    v, _, t = case(name)
    lab, num = check_topology(v, t)
    if name == "book":
        assert num.tolist() == [5] and R.non_manifold_edges(t, True).tolist() == [[0, 1]]
    if name == "bowtie":
        assert lab.tolist() == [0, 1]
    if name == "strip":
        assert num.tolist() == [5000]
    if name == "disjoint":
        assert len(num) == 70000 and np.array_equal(lab, np.arange(70000))
    if name == "res-24":
        assert (len(v), len(t), len(num), int((num == 1).sum()), int(num.max())) == (13918, 16548, 576, 135, 12025)
    if name == "sphere":
        assert num.tolist() == [1056] and len(R.non_manifold_edges(t, False)) == 0


@pytest.mark.parametrize("name", ALL)
def test_removal(name):
    check_removal(*case(name))


@pytest.mark.parametrize("name", [n for n in ALL if n != "disjoint"])
def test_smoothing_one_iteration(name):
    check_smoothing(*case(name))


@pytest.mark.parametrize("name", ALL)
def test_sampling(name):
    check_sampling(*case(name))


def test_removal_masks_indices_and_errors():
    v, c, t = case("res-13")
    vn, tn = normals_of(v, t)
    full = (v, c, vn, t, tn)
    for mask, want_t in ((np.zeros(len(t), bool), len(t)), (np.ones(len(t), bool), 0)):
        mesh = build(v, t, c, vn, tn)
        mesh.remove_triangles_by_mask(mask)
        assert len(mesh._tri) == want_t and same(host(mesh._vert), v)
        assert_rows(attributes(mesh), (v, c, vn) + R.remove_triangles(t, mask, tn))
    for mask, want_v in ((np.zeros(len(v), bool), len(v)), (np.ones(len(v), bool), 0)):
        mesh = build(v, t, c, vn, tn).compute_adjacency_list()
        mesh.get_min_bound()
        mesh.remove_vertices_by_mask(mask)
        assert len(mesh._vert) == want_v and not mesh.has_adjacency_list() and mesh._bounds is None
        assert_rows(attributes(mesh), R.remove_vertices(v, t, mask, c, vn, tn))
    mesh = build(v, t, c, vn, tn)
    for call, n in ((mesh.remove_triangles_by_mask, len(t)), (mesh.remove_vertices_by_mask, len(v))):
        for wrong in (n - 1, n + 1, 0):
            with pytest.raises(RuntimeError):
                call(np.zeros(wrong, bool))
    assert_rows(attributes(mesh), full)                      # a refused call changes nothing
    idx = [5, 5, -3, len(t), 17, len(t) - 1, 10 ** 12]
    mesh.remove_triangles_by_index(idx)
    assert_rows(attributes(mesh), (v, c, vn) + R.remove_triangles(t, R.index_mask(idx, len(t)), tn))
    idx = [0, 3, 3, len(v) - 1, len(v), -1]
    mesh = build(v, t, c, vn, tn).remove_vertices_by_index(idx)
    assert_rows(attributes(mesh), R.remove_vertices(v, t, R.index_mask(idx, len(v)), c, vn, tn))
    # a mesh without optional attributes, and one with colours only
    for cols in (None, c):
        mesh = build(v, t, cols).remove_vertices_by_mask(np.arange(len(v)) % 3 == 0)
        assert_rows(attributes(mesh), R.remove_vertices(v, t, np.arange(len(v)) % 3 == 0, cols))


def test_remove_degenerate_triangles_and_select_by_index():
    v, c, t = case("degenerate")
    _, tn = normals_of(v, t)
    mesh = build(v, t, c, None, tn)
    assert mesh.remove_degenerate_triangles() is mesh
    assert_rows(attributes(mesh), (v, c, None) + R.remove_triangles(t, R.degenerate(t), tn))
    assert len(mesh._tri) == 5
    v, c, t = case("res-8")
    idx = np.random.default_rng(3).permutation(len(v))[:300]
    keep = R.index_mask(idx, len(v))
    raw = build(v, t, c).select_by_index(idx, cleanup=False)
    want = R.remove_vertices(v, t, ~keep, c)
    assert_rows(attributes(raw), want)
    clean = build(v, t, c).select_by_index(idx)
    assert_rows(attributes(clean), R.remove_vertices(want[0], want[3], ~R.referenced(want[3], len(want[0])), want[1]))


@pytest.mark.parametrize("method", ["simple", "laplacian", "taubin"])
@pytest.mark.parametrize("iterations", [0, 5])
def test_smoothing_iterations(method, iterations):
    v, c, t = case("res-13")
    vn, _ = normals_of(v, t)
    mesh = build(v, t, c, vn)
    out = {"simple": lambda: mesh.filter_smooth_simple(iterations), "laplacian": lambda: mesh.filter_smooth_laplacian(iterations, 0.37),
           "taubin": lambda: mesh.filter_smooth_taubin(iterations, 0.6, -0.61)}[method]()
    lam, mu = {"simple": (0.5, -0.53), "laplacian": (0.37, -0.53), "taubin": (0.6, -0.61)}[method]
    rv, rn, rc = R.smooth(v, t, method, iterations, lam, mu, normals=vn, colors=c)
    assert_rows((host(out._vert), host(out._vnrm), host(out._vcol)), (rv, rn, rc))
    if iterations == 0:
        assert same(rv, v) and same(rn, vn) and same(rc, c)
    with pytest.raises(RuntimeError):
        mesh.filter_smooth_taubin(-1)


@pytest.mark.parametrize("scope", ["All", "Vertex", "Normal", "Color"])
@pytest.mark.parametrize("has", ["both", "colors", "normals", "neither"])
def test_smoothing_scopes(scope, has):
    from kinectpy_amd import o3d
    v, c, t = case("cut-13-2048")                            # isolated vertices: empty rows
    vn, _ = normals_of(v, t)
    c = c if has in ("both", "colors") else None
    vn = vn if has in ("both", "normals") else None
    on = (scope in ("All", "Vertex"), scope in ("All", "Normal"), scope in ("All", "Color"))
    out = build(v, t, c, vn).filter_smooth_laplacian(2, 0.5, o3d.geometry.FilterScope[scope])
    assert_rows((host(out._vert), host(out._vnrm), host(out._vcol)), R.smooth(v, t, "laplacian", 2, normals=vn, colors=c, scope=on))
    out = build(v, t, c, vn).filter_smooth_taubin(2, filter_scope=o3d.geometry.FilterScope[scope])
    assert_rows((host(out._vert), host(out._vnrm), host(out._vcol)), R.smooth(v, t, "taubin", 2, normals=vn, colors=c, scope=on))


@pytest.mark.parametrize("scope", ["All", "Vertex", "Normal", "Color"])
@pytest.mark.parametrize("iterations", [0, 1])
def test_smoothing_returns_an_independent_mesh(scope, iterations):
    """a filter's result shares no storage with its source, whichever arrays the scope leaves unfiltered: transform works in place on
    the vertices and the vertex normals, and moving the result must leave every array of the source bit for bit as it was"""
    from kinectpy_amd import o3d
    v, c, t = case("res-8")
    vn, _ = normals_of(v, t)
    T = np.array([[0.0, -1.0, 0.0, 5.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.25], [0.0, 0.0, 0.0, 1.0]])
    src = build(v, t, c, vn)
    out = src.filter_smooth_laplacian(iterations, 0.5, o3d.geometry.FilterScope[scope])
    before = attributes(out)
    mine = {a.data_ptr() for a in (src._vert, src._vcol, src._vnrm, src._tri)}
    assert not mine & {a.data_ptr() for a in (out._vert, out._vcol, out._vnrm, out._tri)}
    assert out.transform(T) is out
    assert not same(host(out._vert), before[0]) and not same(host(out._vnrm), before[2])
    assert_rows(attributes(src), (v, c, vn, t, None))
    src.transform(T)                                         # and the other way round
    assert same(host(out._vcol), before[1]) and not same(host(src._vert), v)
    again = attributes(out)
    src.transform(T)
    assert_rows(attributes(out), again)


def test_taubin_with_mu_zero_is_the_laplacian_plus_an_identity_step():
    v, c, t = case("res-8")
    mesh = build(v, t, c)
    tau, lap = mesh.filter_smooth_taubin(3, 0.5, 0.0), mesh.filter_smooth_laplacian(3, 0.5)
    rv, _, rc = R.smooth(v, t, "taubin", 3, 0.5, 0.0, colors=c)
    assert same(host(tau._vert), rv) and same(host(tau._vcol), rc)
    assert same(host(tau._vert), host(lap._vert)) and same(host(tau._vcol), host(lap._vcol))


@pytest.mark.parametrize("n", [1, 64, 65, 100000])
def test_sampling_sizes(n):
    v, c, t = case("res-13")
    vn, tn = normals_of(v, t)
    pc = build(v, t, c, vn).sample_points_uniformly(n)
    rp, rc, rn, tri_of = R.sample_points_uniformly(v, t, n, 0, colors=c, vertex_normals=vn)
    assert_rows((host(pc._pts), host(pc._col), host(pc._nrm)), (rp, rc, rn))
    upto, _ = R.sample_counts(v, t, n)
    assert np.array_equal(np.bincount(tri_of, minlength=len(t)), np.diff(np.concatenate([[0], upto])))
    bare = build(v, t).sample_points_uniformly(n, seed=2 ** 40 + 7)
    rp2 = R.sample_points_uniformly(v, t, n, 2 ** 40 + 7)[0]
    assert same(host(bare._pts), rp2) and bare._col is None and bare._nrm is None and (n == 1 or not same(rp2, rp))


def test_sampling_normals_and_errors():
    v, c, t = case("res-8")
    vn, tn = normals_of(v, t)
    mesh = build(v, t, c, vn)
    pc = mesh.sample_points_uniformly(500, use_triangle_normal=True, seed=3)
    assert mesh.has_triangle_normals() and same(host(mesh._tnrm), tn)          # computed on the way, as Open3D does
    rp, rc, rn, _ = R.sample_points_uniformly(v, t, 500, 3, colors=c, triangle_normals=tn)
    assert_rows((host(pc._pts), host(pc._col), host(pc._nrm)), (rp, rc, rn))
    own = np.random.default_rng(8).random(tn.shape).astype(np.float32)          # the mesh's own triangle normals are used as they are
    pc = build(v, t, None, None, own).sample_points_uniformly(500, use_triangle_normal=True)
    assert same(host(pc._nrm), R.sample_points_uniformly(v, t, 500, 0, triangle_normals=own)[2]) and pc._col is None
    assert build(v, t, None, None, own).sample_points_uniformly(500)._nrm is None
    for bad in (lambda: mesh.sample_points_uniformly(0), lambda: mesh.sample_points_uniformly(-4), lambda: build(v, np.zeros((0, 3), np.int32)).sample_points_uniformly(5),
                lambda: build(np.zeros((3, 3), np.float32), [[0, 1, 2]]).sample_points_uniformly(5)):
        with pytest.raises(RuntimeError):
            bad()


def test_out_of_range_triangle_raises_before_any_launch():
    v, c, t = case("res-8")
    t = t.copy()
    t[40, 1] = len(v)
    mesh = build(v, t, c)
    for call in (mesh.compute_adjacency_list, mesh.get_non_manifold_edges, mesh.cluster_connected_triangles, mesh.filter_smooth_taubin,
                 mesh.sample_points_uniformly, mesh.remove_unreferenced_vertices):
        with pytest.raises(RuntimeError, match="out of range"):
            call()


def test_clusters_and_samples_repeat_run_to_run():
    v, c, t = case("res-24")
    mesh = build(v, t, c)
    a, b = mesh.cluster_connected_triangles(), mesh.cluster_connected_triangles()
    for x, y in zip(a, b):
        assert same(host(x), host(y))
    p, q = mesh.sample_points_uniformly(20000, seed=1), mesh.sample_points_uniformly(20000, seed=1)
    assert same(host(p._pts), host(q._pts)) and same(host(p._col), host(q._col))


def test_fuse_depth_tsdf_cleans_the_mesh():
    """the ring of test_tsdf_mesh_gpu.py at resolution 32: components below k triangles go, with their vertices, then two Taubin
    iterations, then the normals -- the same as the steps by hand, and as the restatement's steps on the extracted mesh"""
    from kinectpy_amd.preprocessing.fusion import fuse_depth_tsdf
    from kinectpy_amd import o3d
    from kinectpy_amd.utils import synth
    _, depth, rgb, _, truth = synth.sensor_ring(4, xy=synth.small_xy(8))
    origin, length = (-1000.0, -1100.0, 1500.0), 2000.0
    intrinsic = o3d.camera.PinholeCameraIntrinsic(80, 72, 63.0, 63.0, 40.0, 36.0)
    plain = fuse_depth_tsdf(depth[0], rgb[0], intrinsic, truth, length, 32, origin, mesh=True)
    v, c, _, t, _ = attributes(plain)
    lab, num, _ = R.cluster_connected_triangles(v, t)
    sizes = sorted(num.tolist())                             # measured: 4, 8, 8, 12 and 1451 triangles
    k = sizes[-2] + 1                                        # every speck goes, the body stays
    assert sizes[0] < k < sizes[-1]
    mesh = fuse_depth_tsdf(depth[0], rgb[0], intrinsic, truth, length, 32, origin, mesh=True, min_cluster_triangles=k, taubin_iterations=2)
    # by hand, on the device
    hand = fuse_depth_tsdf(depth[0], rgb[0], intrinsic, truth, length, 32, origin, mesh=True)
    hand._vnrm = hand._tnrm = None
    hl, hn, _ = hand.cluster_connected_triangles()
    hand.remove_triangles_by_mask(host(hn)[host(hl)] < k).remove_unreferenced_vertices()
    hand = hand.filter_smooth_taubin(2).compute_vertex_normals()
    assert_rows(attributes(mesh), attributes(hand))
    # by the restatement
    t2, _ = R.remove_triangles(t, num[lab] < k)
    v3, c3, _, t3, _ = R.remove_vertices(v, t2, ~R.referenced(t2, len(v)), c)
    sv, _, sc = R.smooth(v3, t3, "taubin", 2, colors=c3)
    assert_rows(attributes(mesh), (sv, sc, M.vertex_normals(sv, t3), t3, M.triangle_normals(sv, t3)))
    left = R.cluster_connected_triangles(sv, t3)[1]
    assert len(left) < len(num) and left.min() >= k
    # both switches off: what the function returned before
    for a, b in zip(attributes(fuse_depth_tsdf(depth[0], rgb[0], intrinsic, truth, length, 32, origin, mesh=True, min_cluster_triangles=0, taubin_iterations=0)),
                    attributes(plain)):
        assert same(a, b)

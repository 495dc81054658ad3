"""CPU suite of the mesh clean-up (AC13): tests/mesh_ops_ref.py, the pinned restatement the device is held to bit for bit, judged
against independent means -- SciPy's connected components, Python sets, the geometry of a sphere -- and the parts of the feature that
need no GPU: the workspace queries, the namespace, the pipeline hook's defaults."""
import functools
import inspect

import numpy as np
import pytest

import mesh_ops_ref as R
import tsdf_mesh_ref as M

CENTRE, RADIUS = np.array([7.3, 8.1, 6.6]), 5.3


@functools.lru_cache(None)
def sphere():
    """the marching-cubes mesh of tsdf_mesh_ref.sphere_volume() in voxel units: 530 vertices, 1056 triangles, closed"""
    f, w = M.sphere_volume()
    v, _, t, _ = M.extract_triangle_mesh(f, w, None, 16, 1.0, (0.0, 0.0, 0.0))
    return v, t


def random_mesh(res):
    """the generator of test_tsdf_mesh_gpu.random_case, on the host"""
    rng = np.random.default_rng(1000 + res)
    n = res ** 3
    f = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    where = rng.random(n) < 0.08
    f[where] = special[rng.integers(0, 4, int(where.sum()))]
    w = np.where(rng.random(n) < 0.1, 0.0, rng.integers(1, 9, n)).astype(np.float32)
    c = rng.uniform(0.0, 255.0, (n, 3)).astype(np.float32)
    return M.extract_triangle_mesh(f, w, c, res, (res * 0.013) / res, np.array((-0.37, 1.91, 12.3)))[:3]


def scipy_components(triangles):
    """labels of the connected components of the shared-edge graph, renumbered by smallest triangle index"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    T = len(triangles)
    by_edge = {}
    for t, (a, b, c) in enumerate(np.asarray(triangles).tolist()):
        for e in ((a, b), (b, c), (c, a)):
            by_edge.setdefault((min(e), max(e)), []).append(t)
    rows, cols = [], []
    for members in by_edge.values():
        for m in members[1:]:
            rows.append(members[0])
            cols.append(m)
    _, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(T, T)), directed=False)
    first = {}
    for t, c in enumerate(lab.tolist()):
        first.setdefault(c, len(first))            # the order in which ascending triangles meet the components
    return np.array([first[c] for c in lab.tolist()], dtype=np.int32)


@pytest.mark.parametrize("res", [8, 13])
def test_clusters_against_scipy(res):
    v, _, t = random_mesh(res)
    lab, count, area = R.cluster_connected_triangles(v, t)
    assert (len(v), len(t), len(count), int((count == 1).sum())) == {8: (429, 458, 26, 8), 13: (2083, 2408, 89, 28)}[res]
    assert np.array_equal(lab, scipy_components(t))
    assert np.array_equal(count, np.bincount(lab))
    assert area.shape == count.shape and np.isclose(area.sum(), M.surface_area(v, t), rtol=1e-12)
    if res == 13:
        off, _ = R.adjacency(t, len(v))
        assert count.max() == 1919 and np.diff(off).max() == 15
        assert len(R.non_manifold_edges(t, False)) - len(R.non_manifold_edges(t, True)) == 1776          # boundary edges


def test_hand_built_clusters_and_edges():
    book = np.array([[0, 1, 2 + k] for k in range(5)])                      # five pages on the spine {0, 1}
    lab, count, _ = R.cluster_connected_triangles(np.zeros((7, 3), np.float32), book)
    assert lab.tolist() == [0] * 5 and count.tolist() == [5]
    assert R.non_manifold_edges(book, True).tolist() == [[0, 1]]
    assert len(R.non_manifold_edges(book, False)) == 11                     # the spine and ten boundary edges
    bowtie = np.array([[0, 1, 2], [2, 3, 4]])                               # two triangles that share a vertex only
    assert R.cluster_connected_triangles(np.zeros((5, 3), np.float32), bowtie)[0].tolist() == [0, 1]


@pytest.mark.parametrize("res", [8, 13])
def test_adjacency_against_python_sets(res):
    v, _, t = random_mesh(res)
    t = np.concatenate([t, [[5, 5, 9]]])                                    # a degenerate triangle: 5 is its own neighbour
    want = [set() for _ in range(len(v))]
    for a, b, c in t.tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            want[x].add(y)
            want[y].add(x)
    off, nb = R.adjacency(t, len(v))
    assert off.dtype == np.int32 and nb.dtype == np.int32 and off[0] == 0 and off[-1] == len(nb)
    for i in range(len(v)):
        row = nb[off[i]:off[i + 1]].tolist()
        assert row == sorted(want[i])
    assert 5 in nb[off[5]:off[6]]


def test_sphere_is_one_closed_cluster():
    v, t = sphere()
    assert v.shape == (530, 3) and t.shape == (1056, 3)
    lab, count, area = R.cluster_connected_triangles(v, t)
    assert count.tolist() == [1056] and not lab.any()
    assert area[0] == M.surface_area(v, t)                                  # one cluster: the same chain
    assert len(R.non_manifold_edges(t, False)) == 0 and len(R.non_manifold_edges(t, True)) == 0


def test_removal_keeps_order_and_attributes():
    v, c, t = random_mesh(8)
    rng = np.random.default_rng(2)
    gone = rng.random(len(v)) < 0.3
    v2, c2, _, t2, _ = R.remove_vertices(v, t, gone, c)
    assert len(v2) == int((~gone).sum()) and np.array_equal(v2, v[~gone]) and np.array_equal(c2, c[~gone])
    survivors = [row for row in t.tolist() if not gone[row].any()]
    assert np.array_equal(v2[t2], v[np.array(survivors)])                   # the same corners, renumbered
    ref = R.referenced(t2, len(v2))
    v3, _, _, t3, _ = R.remove_vertices(v2, t2, ~ref)
    assert R.referenced(t3, len(v3)).all() and np.array_equal(v3[t3], v2[t2])
    assert R.degenerate(np.array([[0, 1, 2], [3, 3, 4], [5, 6, 5], [7, 8, 8]])).tolist() == [False, True, True, True]
    assert R.index_mask([3, -1, 99, 3, 0], 5).tolist() == [True, False, False, True, False]


def noisy_sphere():
    v, t = sphere()
    rng = np.random.default_rng(5)
    d = v.astype(np.float64) - CENTRE
    return (CENTRE + d * (1.0 + 0.03 * rng.standard_normal(len(v)))[:, None]).astype(np.float32), t


def radii(v):
    return np.linalg.norm(v.astype(np.float64) - CENTRE, axis=1)


def test_smoothing_on_a_noisy_sphere():
    """Radial noise of 3 % on the sphere mesh, ten iterations of each filter.  Measured (mean radius, variance of the radii):
        noiseless mesh  5.29185  3.9e-05        noisy      5.28812  0.02369
        simple          4.66020  0.00432        laplacian  4.97239  0.00577        taubin  5.30493  0.00724
    Every filter lowers the variance; the Laplacian shrinks the sphere by 0.32, Taubin's second step holds it within 0.013."""
    noisy, t = noisy_sphere()
    clean = radii(sphere()[0]).mean()
    out = {m: radii(R.smooth(noisy, t, m, 10)[0]) for m in ("simple", "laplacian", "taubin")}
    for m, r in out.items():
        assert r.var() < radii(noisy).var(), m
    assert abs(out["taubin"].mean() - clean) < abs(out["laplacian"].mean() - clean)
    assert out["laplacian"].mean() < clean                                  # the shrinkage Taubin is there to undo


def test_smoothing_scopes_and_edges():
    noisy, t = noisy_sphere()
    n = M.vertex_normals(noisy, t)
    c = np.random.default_rng(1).random(noisy.shape).astype(np.float32)
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
    v0, n0, c0 = R.smooth(noisy, t, "taubin", 0, normals=n, colors=c)
    assert same(v0, noisy) and same(n0, n) and same(c0, c)                  # no iteration: float32 -> float64 -> float32
    va, na, ca = R.smooth(noisy, t, "laplacian", 2, normals=n, colors=c)
    vn = R.smooth(noisy, t, "laplacian", 2, normals=n, colors=c, scope=(False, True, False))
    assert same(vn[0], noisy) and same(vn[2], c) and not same(vn[1], n)
    assert not same(vn[1], na)                                              # the weights follow the moving vertices under All
    vv = R.smooth(noisy, t, "laplacian", 2, normals=n, colors=c, scope=(True, False, False))
    assert same(vv[0], va) and same(vv[1], n)
    # mu = 0: the second step is y + 0 * (s / W - y) = y, so Taubin(lambda, 0) is the Laplacian
    assert same(R.smooth(noisy, t, "taubin", 3, 0.5, 0.0)[0], R.smooth(noisy, t, "laplacian", 3, 0.5)[0])
    # an isolated vertex keeps its value under the Laplacian and under the simple filter (the mean of itself)
    lone = np.concatenate([noisy, [[1.0, 2.0, 3.0]]]).astype(np.float32)
    for m in ("simple", "laplacian", "taubin"):
        assert R.smooth(lone, t, m, 2)[0][-1].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        R.smooth(noisy, t, "simple", -1)


def test_llround():
    assert [R.llround(x) for x in (0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 2.4999999999999996, 7.0)] == [0, 0, 1, 2, 3, 2, 7]


@pytest.mark.parametrize("n", [1, 64, 65, 5000])
def test_sampling_counts_follow_the_llround_rule(n):
    v, t = sphere()
    upto, total = R.sample_counts(v, t, n)
    assert total == M.surface_area(v, t) and upto[-1] == n and np.all(np.diff(upto) >= 0)
    area = R.triangle_areas(v, t)
    want = [R.llround(float(np.float64(s) / np.float64(total)) * n) for s in np.cumsum(area)]       # cumsum is the same serial chain
    want[-1] = n
    assert upto.tolist() == want
    _, _, _, tri_of = R.sample_points_uniformly(v, t, n, seed=3)
    counts = np.bincount(tri_of, minlength=len(t))
    assert counts.sum() == n and np.array_equal(counts, np.diff(np.concatenate([[0], upto])))
    assert np.all(np.diff(tri_of) >= 0)                                     # ordered by triangle


def test_sampled_points_lie_in_their_triangles():
    """Tolerance.  A sample is (a v0 + b v1) + c v2 with a + b + c = 1 up to 2^-52, evaluated in float64 (error below 1e-15 of the
    coordinates) and rounded once to float32: each coordinate moves by at most half an ulp, 2^-24 |coordinate| <= 2^-24 C with C the
    largest |coordinate| of the mesh, so the point moves by at most sqrt(3) 2^-24 C < tol = 2 * 2^-24 C.  Hence its distance to the
    triangle's plane is at most tol, and a barycentric coordinate -- signed distance to the opposite edge's line over the altitude
    h_i = 2 A / |edge_i| -- is at least -tol / h_i."""
    v, t = sphere()
    c = np.random.default_rng(4).random(v.shape).astype(np.float32)
    pts, col, nrm, tri_of = R.sample_points_uniformly(v, t, 5000, seed=1, colors=c, vertex_normals=M.vertex_normals(v, t))
    assert pts.dtype == np.float32 and pts.shape == (5000, 3) and col.shape == (5000, 3) and nrm.shape == (5000, 3)
    tol = 2.0 * 2.0 ** -24 * float(np.abs(v).max())
    V = v.astype(np.float64)[t[tri_of]]
    e1, e2, d = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0], pts.astype(np.float64) - V[:, 0]
    nvec = np.cross(e1, e2)
    twice_area = np.linalg.norm(nvec, axis=1)
    assert np.all(np.abs((d * nvec).sum(1)) / twice_area <= tol)
    bary = np.stack([np.zeros(len(d)), (np.cross(d, e2) * nvec).sum(1) / twice_area ** 2, (np.cross(e1, d) * nvec).sum(1) / twice_area ** 2], 1)
    bary[:, 0] = 1.0 - bary[:, 1] - bary[:, 2]
    edge = np.stack([np.linalg.norm(V[:, 2] - V[:, 1], axis=1), np.linalg.norm(e2, axis=1), np.linalg.norm(e1, axis=1)], 1)
    assert np.all(bary >= -tol / (twice_area[:, None] / edge))
    assert np.all(col >= 0.0) and np.all(col <= 1.0)
    again = R.sample_points_uniformly(v, t, 5000, seed=1, colors=c)
    other = R.sample_points_uniformly(v, t, 5000, seed=2, colors=c)
    assert np.array_equal(again[0], pts) and np.array_equal(again[1], col)
    assert np.array_equal(other[3], tri_of) and not np.array_equal(other[0], pts)          # the seed moves the points, not the counts
    tn = M.triangle_normals(v, t)
    assert np.array_equal(R.sample_points_uniformly(v, t, 64, triangle_normals=tn)[2], tn[R.sample_points_uniformly(v, t, 64)[3]])
    flat = np.zeros((3, 3), np.float32)
    for bad in (lambda: R.sample_points_uniformly(v, t, 0), lambda: R.sample_points_uniformly(flat, [[0, 1, 2]], 5),
                lambda: R.sample_points_uniformly(v, np.zeros((0, 3), np.int32), 5)):
        with pytest.raises(ValueError):
            bad()


def test_zero_area_triangles_get_no_samples():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [1, 1, 0]], np.float32)
    t = np.array([[0, 1, 3], [0, 1, 2], [1, 1, 4], [1, 4, 2]])             # collinear, real, degenerate, real
    tri_of = R.sample_points_uniformly(v, t, 101)[3]
    assert set(tri_of.tolist()) == {1, 3} and np.bincount(tri_of).tolist() == [0, 51, 0, 50]


# ---- the product's side, as far as it goes without a GPU ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.load()


def test_workspace_queries_answer_without_a_gpu(lib):
    V, T = 200000, 330000
    adj, edges, clusters = (f(V, T) for f in (lib.kpx_mesh_adjacency_workspace_bytes, lib.kpx_mesh_edges_workspace_bytes, lib.kpx_mesh_cluster_workspace_bytes))
    assert adj >= 6 * T * (8 + 8 + 4) and edges >= 3 * T * 16                 # two key arrays (the sort carries no values), the owners
    assert clusters >= 3 * T * 24 + 23 * T                                    # keys and their numbers; parent, rank, four sort arrays
    assert lib.kpx_mesh_adjacency_workspace_bytes(10, 20) < adj
    assert lib.kpx_mesh_select_workspace_bytes(V, T) >= 4 * V
    assert lib.kpx_mesh_smooth_workspace_bytes(V) >= 7 * 24 * V
    assert lib.kpx_mesh_sample_workspace_bytes(T) >= 16 * T
    for f in (lib.kpx_mesh_adjacency_workspace_bytes, lib.kpx_mesh_edges_workspace_bytes, lib.kpx_mesh_cluster_workspace_bytes,
              lib.kpx_mesh_select_workspace_bytes):
        assert f(0, 0) > 0 and f(-1, 5) == 0 and f(5, 2 ** 31) == 0          # 6 T must fit an int32
    assert lib.kpx_mesh_smooth_workspace_bytes(-1) == 0 and lib.kpx_mesh_sample_workspace_bytes(-1) == 0


def test_arguments_are_checked_before_the_device(lib):
    import ctypes as C
    rc = lib.kpx_mesh_smooth(None, None, None, 10, None, None, 0, 7, 1, C.c_double(0.5), C.c_double(-0.53), None, None, None, None, 0, None)
    assert rc == -1 and b"unknown method" in lib.kpx_last_error()
    rc = lib.kpx_mesh_smooth(None, None, None, 10, None, None, 0, 2, -1, C.c_double(0.5), C.c_double(-0.53), None, None, None, None, 0, None)
    assert rc == -1 and b"number_of_iterations" in lib.kpx_last_error()
    rc = lib.kpx_mesh_sample_points(None, None, None, None, 10, None, 10, 0, 0, None, None, None, None, None, 0, None)
    assert rc == -1 and b"number_of_points" in lib.kpx_last_error()
    rc = lib.kpx_mesh_sample_points(None, None, None, None, 10, None, 0, 5, 0, None, None, None, None, None, 0, None)
    assert rc == -1 and b"no triangles" in lib.kpx_last_error()
    rc = lib.kpx_mesh_flags(9, None, 1, 1, None, 0, None, 1, None)
    assert rc == -1 and b"unknown kind" in lib.kpx_last_error()
    rc = lib.kpx_mesh_adjacency(None, 5, 2 ** 31, None, None, None, None, 0, None)
    assert rc != 0 and b"at most" in lib.kpx_last_error()


def test_namespace_exports():
    from kinectpy_amd import o3d, ops
    fs = o3d.geometry.FilterScope
    assert {m.name for m in fs} == {"All", "Color", "Normal", "Vertex"}
    mesh = o3d.geometry.TriangleMesh
    for name in ("compute_adjacency_list", "adjacency_list", "get_non_manifold_edges", "is_edge_manifold", "cluster_connected_triangles",
                 "remove_triangles_by_mask", "remove_triangles_by_index", "remove_vertices_by_mask", "remove_vertices_by_index",
                 "remove_unreferenced_vertices", "remove_degenerate_triangles", "select_by_index", "filter_smooth_simple",
                 "filter_smooth_laplacian", "filter_smooth_taubin", "sample_points_uniformly"):
        assert hasattr(mesh, name), name
    for name in ("mesh_adjacency", "mesh_non_manifold_edges", "mesh_cluster_triangles", "mesh_flags", "mesh_select_triangles", "mesh_select_vertices",
                 "mesh_smooth", "mesh_sample_points"):
        assert callable(getattr(ops, name)), name
    sig = inspect.signature(mesh.filter_smooth_taubin).parameters
    assert (sig["number_of_iterations"].default, sig["lambda_filter"].default, sig["mu"].default, sig["filter_scope"].default) == (1, 0.5, -0.53, fs.All)
    sig = inspect.signature(mesh.sample_points_uniformly).parameters
    assert (sig["number_of_points"].default, sig["use_triangle_normal"].default, sig["seed"].default) == (100, False, 0)
    for name in ("remove_duplicated_vertices", "simplify_quadric_decimation", "is_watertight", "sample_points_poisson_disk", "crop"):
        assert not hasattr(mesh, name), name                                # stated as not built


def test_fuse_depth_tsdf_clean_up_is_off_by_default():
    from kinectpy_amd.preprocessing.fusion import fuse_depth_tsdf
    sig = inspect.signature(fuse_depth_tsdf).parameters
    assert sig["mesh"].default is False and sig["min_cluster_triangles"].default == 0 and sig["taubin_iterations"].default == 0

"""GPU suite of the neighbour search: ops.search_* and o3d.geometry.KDTreeFlann against the float64 brute force of
tests/search_ref.py -- indices, squared distances and counts compared for EXACT equality on quantised coordinates (where the
reference's plain sum and the library's fma chain are both exact) -- and against the C oracle's hybrid search on a general float
cloud (self-query)."""
import numpy as np
import pytest
import torch

from tests import search_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as O
    return O


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def _same_knn(got, want, what=""):
    for g, w, name in zip(got, want, ("idx", "d2", "count")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _same_csr(got, want, what=""):
    for g, w, name in zip(got, want, ("offsets", "idx", "d2")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


# ---- 1. foreign queries ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def foreign():
    rng = np.random.default_rng(11)
    pts = R.quantised(rng, 3000, [-40, -25, -10], [40, 25, 10])
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    qs = R.quantised(rng, 500, c - 1.25 * e, c + 1.25 * e)
    far = np.array([c + [100 * 2 * e[0], 0, 0], c - 100 * 2 * e], dtype=np.float32)        # 100 box lengths away (exact: |x| <= 4096 + ...)
    qs = np.concatenate([qs, far])
    outside = np.any((qs < lo) | (qs > hi), axis=1)
    assert 50 < outside.sum() < 450
    return pts, qs, R.d2_matrix(pts, qs)


@pytest.mark.parametrize("k", [1, 2, 8, 33, 200, 3000, 3500])
def test_foreign_queries(ops, foreign, k):
    pts, qs, _ = foreign
    want = R.knn(pts, qs, k)
    assert np.all(want[2] == min(k, 3000))
    got = _np(*ops.search_knn(ops.search_index(pts), qs, k))
    _same_knn(got, want, k)
    if k == 3500:
        assert np.all(got[0][:, 3000:] == -1) and np.all(np.isinf(got[1][:, 3000:]))


# ---- 2. ties / 3. strictness ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice():
    g = np.arange(12, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return pts[np.random.default_rng(2).permutation(len(pts))]


def test_ties_take_the_lowest_index(ops, lattice):
    """k = 20 at a cell centre: 8 corners at d2 = 0.75, then the 24 points at d2 = 2.75 -- of which the lowest indices stay.  Every
    cell centre is a query; the k-th and (k+1)-th distances are equal wherever the second shell is complete (the 9^3 cells that
    do not touch the lattice's boundary -- a corner cell has only 12 + 8 = 20 points in the two shells), checked here."""
    c = np.arange(11, dtype=np.float32) + 0.5
    centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    qs = np.concatenate([centres, lattice[::3]])
    k = 20
    want = R.knn(lattice, qs, k)
    ref21 = R.knn(lattice, qs, k + 1)[1]
    inner = np.all((centres >= 1.5) & (centres <= 9.5), axis=1)
    assert inner.sum() == 729 and np.all(ref21[:len(centres)][inner][:, k - 1] == ref21[:len(centres)][inner][:, k])
    got = _np(*ops.search_knn(ops.search_index(lattice), qs, k))
    _same_knn(got, want)


def test_radius_is_strict(ops, lattice):
    index = ops.search_index(lattice)
    qs = lattice[::5]
    interior = np.all((qs >= 1) & (qs <= 10), axis=1)
    for r, n_in in ((1.0, 1), (float(np.nextafter(1.0, 2.0)), 7)):
        want_h = R.knn(lattice, qs, 10, r)
        assert np.all(want_h[2][interior] == n_in)
        _same_knn(_np(*ops.search_hybrid(index, qs, r, 10)), want_h, r)
        want_r = R.radius(lattice, qs, r)
        assert np.all(np.diff(want_r[0])[interior] == n_in)
        _same_csr(_np(*ops.search_radius(index, qs, r)), want_r, r)


# ---- 4. radius CSR / 5. hybrid = radius cut -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clustered():
    rng = np.random.default_rng(4)
    pts = np.concatenate([R.quantised(rng, 4000, -2, 2), R.quantised(rng, 1000, -500, 500)])
    pts = pts[rng.permutation(len(pts))]
    qs = np.concatenate([R.quantised(rng, 100, -2, 2), R.quantised(rng, 150, -500, 500), R.quantised(rng, 50, 1500, 1600)])
    return pts, qs[rng.permutation(len(qs))]


@pytest.mark.parametrize("m", [1, 300])
def test_radius_csr(ops, clustered, m):
    """empty segments (the queries near 1500 at small radii), short ones, segments beyond the LDS sort length (the ~4000 points
    of the cluster at r = 8) and, at r = 4000, every segment holding all 5000 points"""
    pts, qs = clustered
    qs = qs[:m] if m > 1 else R.quantised(np.random.default_rng(1), 1, -1, 1)
    index = ops.search_index(pts)
    for r in (0.5, 8.0, 4000.0):
        want = R.radius(pts, qs, r)
        lens = np.diff(want[0])
        if r == 4000.0:
            assert np.all(lens == 5000)
        elif m > 1 and r == 8.0:
            assert lens.min() == 0 and lens.max() > 1024
        elif m > 1:
            assert lens.min() == 0 and np.any((lens > 0) & (lens <= 1024))
        _same_csr(_np(*ops.search_radius(index, qs, r)), want, (m, r))


@pytest.mark.parametrize("max_nn", [1, 30, 4096])
def test_hybrid_is_the_radius_cut(ops, clustered, max_nn):
    pts, qs = clustered
    index = ops.search_index(pts)
    r = 8.0
    off, ridx, rd2 = _np(*ops.search_radius(index, qs, r))
    hidx, hd2, hcnt = _np(*ops.search_hybrid(index, qs, r, max_nn))
    lens = np.diff(off)
    assert np.array_equal(hcnt, np.minimum(lens, max_nn).astype(np.int32)) and lens.max() > 1024
    for i in range(len(qs)):
        c = hcnt[i]
        assert np.array_equal(hidx[i, :c], ridx[off[i]:off[i] + c]) and np.array_equal(hd2[i, :c], rd2[off[i]:off[i] + c])
        assert np.all(hidx[i, c:] == -1) and np.all(np.isinf(hd2[i, c:]))


# ---- 6. general floats, self-query, against the C oracle ------------------------------------------------------------------
@pytest.mark.parametrize("radius,max_nn", [(100.0, 30), (300.0, 150)])
def test_general_floats_self_query(ops, oracle, radius, max_nn):
    from kinectpy_amd.utils import synth
    pts = synth.filter_cloud(20_000)
    nbr, cnt, d2 = oracle.hybrid_knn_d2(pts, radius, max_nn)
    gi, gd, gc = _np(*ops.search_hybrid(ops.search_index(pts), pts, radius, max_nn))
    assert np.array_equal(gc, cnt) and cnt.max() == max_nn and cnt.min() < max_nn
    mask = np.arange(max_nn)[None, :] < cnt[:, None]
    assert np.array_equal(gi[mask], nbr[mask])
    assert np.array_equal(gd[mask].view(np.uint64), d2[mask].view(np.uint64))
    assert np.all(gi[~mask] == -1) and np.all(np.isinf(gd[~mask]))


# ---- 7. degenerate clouds and queries ------------------------------------------------------------------------------------
def test_degenerate_clouds(ops):
    rng = np.random.default_rng(8)
    qs = np.concatenate([R.quantised(rng, 40, -20, 20), np.array([[3, 3, 3], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)])
    clouds = {
        "empty": np.zeros((0, 3), np.float32),
        "one": np.array([[3, 3, 3]], np.float32),
        "coincident": np.tile(np.array([[1.5, -2.25, 7]], np.float32), (500, 1)),
        "coplanar": np.concatenate([R.quantised(rng, 2000, -16, 16)[:, :2], np.full((2000, 1), 2.5, np.float32)], 1),
    }
    for name, pts in clouds.items():
        index = ops.search_index(pts)
        assert len(index) == len(pts)
        for k in (1, 7, 600):
            got = _np(*ops.search_knn(index, qs, k))
            _same_knn(got, R.knn(pts, qs, k), (name, k))
            assert np.all(got[2][-3:] == 0) and np.all(got[0][-3:] == -1)          # non-finite queries find nothing
        for r in (0.25, 6.0, 100.0):
            _same_knn(_np(*ops.search_hybrid(index, qs, r, 9)), R.knn(pts, qs, 9, r), (name, r))
            _same_csr(_np(*ops.search_radius(index, qs, r)), R.radius(pts, qs, r), (name, r))
        # no queries at all
        i0, d0, c0 = ops.search_knn(index, np.zeros((0, 3), np.float32), 4)
        assert tuple(i0.shape) == (0, 4) and tuple(d0.shape) == (0, 4) and tuple(c0.shape) == (0,)
        o0, ri0, rd0 = _np(*ops.search_radius(index, np.zeros((0, 3), np.float32), 1.0))
        assert o0.tolist() == [0] and len(ri0) == 0 and len(rd0) == 0


# ---- 8. the index outlives its cloud ---------------------------------------------------------------------------------------
def test_index_lifetime_and_repeatability(ops, foreign):
    pts, qs, _ = foreign
    src = torch.as_tensor(pts).cuda()
    index = ops.search_index(src)
    src.zero_()
    torch.cuda.synchronize()
    fresh = ops.search_index(pts)
    first = None
    for _ in range(2):
        res = (_np(*ops.search_knn(index, qs, 8)) + _np(*ops.search_radius(index, qs, 6.0)) + _np(*ops.search_hybrid(index, qs, 6.0, 5))
               + _np(*ops.search_knn(index, qs, 700)))
        if first is None:
            first = res
            ref = (_np(*ops.search_knn(fresh, qs, 8)) + _np(*ops.search_radius(fresh, qs, 6.0)) + _np(*ops.search_hybrid(fresh, qs, 6.0, 5))
                   + _np(*ops.search_knn(fresh, qs, 700)))
            assert all(np.array_equal(a, b) for a, b in zip(res, ref))
        assert all(np.array_equal(a, b) for a, b in zip(res, first))
    _same_knn(first[:3], R.knn(pts, qs, 8))


# ---- 9. the Open3D-shaped surface -----------------------------------------------------------------------------------------
def test_kdtreeflann_api(foreign):
    from kinectpy_amd import o3d
    pts, qs, D = foreign
    cloud = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(pts))
    tree = o3d.geometry.KDTreeFlann(cloud)
    tree2 = o3d.geometry.KDTreeFlann()
    assert tree2.set_geometry(pts.astype(np.float64))
    bi, bd, bc = _np(*tree.search_knn(qs, 6))
    hi_, hd, hc = _np(*tree.search_hybrid(qs, 5.0, 4))
    off, ri, rd = _np(*tree.search_radius(qs, 5.0))
    _same_knn((bi, bd, bc), R.knn(pts, qs, 6))
    for j in (0, 17, 501):
        for t in (tree, tree2):
            c, i, d = t.search_knn_vector_3d(qs[j].astype(np.float64), 6)
            assert c == bc[j] and np.array_equal(i, bi[j, :c]) and np.array_equal(d, bd[j, :c])
        c, i, d = tree.search_hybrid_vector_3d(qs[j], 5.0, 4)
        assert c == hc[j] and np.array_equal(i, hi_[j, :c]) and np.array_equal(d, hd[j, :c])
        c, i, d = tree.search_radius_vector_3d(qs[j], 5.0)
        assert c == off[j + 1] - off[j] and np.array_equal(i, ri[off[j]:off[j + 1]]) and np.array_equal(d, rd[off[j]:off[j + 1]])
        for param, want in ((o3d.geometry.KDTreeSearchParamKNN(6), (bc[j], bi[j, :bc[j]])), (o3d.geometry.KDTreeSearchParamHybrid(5.0, 4), (hc[j], hi_[j, :hc[j]])),
                            (o3d.geometry.KDTreeSearchParamRadius(5.0), (off[j + 1] - off[j], ri[off[j]:off[j + 1]]))):
            c, i, _ = tree.search_vector_3d(qs[j], param)
            assert c == want[0] and np.array_equal(i, want[1])
    # distances between clouds
    other = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(qs))
    dist = other.compute_point_cloud_distance(cloud)
    assert dist.dtype == np.float64 and np.array_equal(dist, np.sqrt(D.min(axis=1)))


def test_nearest_neighbor_distance(lattice):
    from kinectpy_amd import o3d
    P = lambda a: o3d.geometry.PointCloud(o3d.utility.Vector3dVector(np.asarray(a, np.float32)))
    d = P(lattice).compute_nearest_neighbor_distance()
    assert d.dtype == np.float64 and d.shape == (len(lattice),) and np.all(d == 1.0)
    assert P([[1, 2, 3]]).compute_nearest_neighbor_distance().tolist() == [0.0]
    dup = np.array([[0, 0, 0], [5, 0, 0], [0, 0, 0], [9, 0, 0]], np.float32)
    assert P(dup).compute_nearest_neighbor_distance().tolist() == [0.0, 4.0, 0.0, 4.0]
    assert len(P(np.zeros((0, 3))).compute_nearest_neighbor_distance()) == 0

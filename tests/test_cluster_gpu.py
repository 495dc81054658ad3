"""cluster_dbscan / remove_radius_outlier on the MI355X against the literal Open3D loop (tests/dbscan_ref.py) and analytic labels."""
import numpy as np
import pytest
import torch

from kinectpy_amd import ops
from kinectpy_amd.geometry import PointCloud
from kinectpy_amd.utils import synth
from tests import dbscan_ref as R

pytestmark = pytest.mark.gpu

NEXT1 = float(np.nextafter(1.0, 2.0))


def _dbscan(pts, eps, min_points):
    labels, cnt = ops.cluster_dbscan(np.ascontiguousarray(pts, dtype=np.float32), eps, min_points)
    return labels.cpu().numpy(), int(cnt.cpu()[0])


def _check(pts, eps, min_points, nbrs):
    lab, nc = _dbscan(pts, eps, min_points)
    ref = R.dbscan_loop(*nbrs, min_points)
    assert np.array_equal(lab, ref), (eps, min_points, int((lab != ref).sum()))
    assert nc == ref.max(initial=-1) + 1
    return lab


def _spacing(pts):
    from scipy.spatial import cKDTree
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=2)
    return float(np.median(d[:, 1]))


def _oracle_nbrs(O, pts, eps):
    max_nn = 256
    while True:
        nbr, cnt = O.hybrid_knn(pts, eps, max_nn)
        if cnt.max(initial=0) < max_nn:
            return R.oracle_neighbours(O, pts, eps, max_nn)
        max_nn *= 2


def test_frame_cloud_subsets_match_loop(base_cloud):
    rng = np.random.default_rng(5)
    for size in (4000, 30000):
        pts = base_cloud[np.sort(rng.choice(len(base_cloud), size, replace=False))]
        pts = pts[rng.permutation(size)]
        h = _spacing(pts)
        for f in (0.5, 1.5, 4.0):
            eps = float(np.round(f * h, 1)) or 0.5
            nbrs = R.integer_neighbours(pts, eps)
            for mp in (0, 1, 5, 10, 50):
                _check(pts, eps, mp, nbrs)


def test_filter_cloud_subsets_match_loop(oracle):
    pts = synth.filter_cloud(50_000, seed=9)
    h = _spacing(pts)
    for f in (0.5, 1.5, 4.0):
        eps = f * h
        nbrs = _oracle_nbrs(oracle, pts, eps)
        for mp in (0, 1, 5, 10, 50):
            _check(pts, eps, mp, nbrs)


def _lattice(nx, ny, nz, off=(0, 0, 0)):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g + np.asarray(off)).astype(np.float32)


def test_strict_radius_on_lattice():
    pts = _lattice(12, 10, 8)
    pts = pts[np.random.default_rng(1).permutation(len(pts))]
    lab, nc = _dbscan(pts, 1.0, 2)                    # d2 = 1 is not < 1: every point is alone
    assert nc == 0 and np.all(lab == -1)
    lab, nc = _dbscan(pts, 1.0, 1)                    # every point core and alone: cluster = index
    assert nc == len(pts) and np.array_equal(lab, np.arange(len(pts)))
    for mp in (2, 5, 7, 8):                           # face neighbours now count (interior: 7 with itself)
        _check(pts, NEXT1, mp, R.integer_neighbours(pts, NEXT1))
    lab, nc = _dbscan(pts, NEXT1, 2)
    assert nc == 1 and np.all(lab == 0)


def test_border_takes_smallest_cluster_and_bridge_joins_nothing():
    pts, bridge, A, B = R.two_blobs_and_bridge()
    rng = np.random.default_rng(3)
    for _ in range(60):
        perm = rng.permutation(len(pts))
        inv = np.argsort(perm)
        p = pts[perm]
        lab = _check(p, NEXT1, 4, R.integer_neighbours(p, NEXT1))
        la, lb = lab[inv[A]], lab[inv[B]]
        assert len(set(la.tolist())) == 1 and len(set(lb.tolist())) == 1 and la[0] != lb[0]
        assert lab[inv[bridge]] == min(la[0], lb[0])


def test_deep_tree_line():
    n = 1_000_000
    rng = np.random.default_rng(11)
    pts = np.zeros((n, 3), dtype=np.float32)
    pts[:, 0] = rng.permutation(n).astype(np.float32)        # index order unrelated to position
    lab, nc = _dbscan(pts, 1.5, 3)
    assert nc == 1 and np.all(lab == 0)                       # the end points (two neighbours) are border points of cluster 0
    lab, nc = _dbscan(pts, 1.5, 4)
    assert nc == 0 and np.all(lab == -1)


def test_duplicates():
    rng = np.random.default_rng(2)
    pts = np.concatenate([np.zeros((5000, 3), np.float32), _lattice(5, 5, 5, (50, 0, 0)), np.array([[30, 30, 30]], np.float32)])
    perm = rng.permutation(len(pts))
    p = pts[perm]
    lab, nc = _dbscan(p, 1.5, 5)
    is_dup, is_lat = perm < 5000, (perm >= 5000) & (perm < 5125)
    first = sorted([np.flatnonzero(is_dup)[0], np.flatnonzero(is_lat)[0]])
    want = np.full(len(p), -1)
    want[is_dup] = first.index(np.flatnonzero(is_dup)[0])
    want[is_lat] = first.index(np.flatnonzero(is_lat)[0])
    assert nc == 2 and np.array_equal(lab, want)


def test_all_noise_and_tiny():
    pts = np.random.default_rng(4).integers(0, 20, size=(1000, 3)).astype(np.float32)
    lab, nc = _dbscan(pts, 3.0, 1001)
    assert nc == 0 and np.all(lab == -1)
    assert PointCloud().cluster_dbscan(1.0, 5).shape == (0,)
    lab, nc = _dbscan(np.zeros((0, 3), np.float32), 1.0, 5)
    assert nc == 0 and lab.shape == (0,)
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    for mp, want, wnc in ((0, 0, 1), (1, 0, 1), (2, -1, 0)):
        lab, nc = _dbscan(one, 1.0, mp)
        assert nc == wnc and np.array_equal(lab, [want])


def test_beyond_4m_points():
    blocks = [_lattice(100, 100, 100, (102 * b, 0, 0)) for b in range(5)]
    k = np.arange(1000)
    single = np.stack([2 * (k % 255), np.full(1000, -3), 2 * (k // 255)], -1).astype(np.float32)
    pts = np.concatenate(blocks + [single])
    n = len(pts)
    assert n > (1 << 22)
    perm = np.random.default_rng(8).permutation(n)
    p = pts[perm]
    lab, nc = _dbscan(p, 1.5, 3)
    group = np.minimum(perm // 1_000_000, 5)                   # 0..4 lattices, 5 singletons
    firsts = [int(np.flatnonzero(group == b)[0]) for b in range(5)]
    rank = {b: sorted(firsts).index(firsts[b]) for b in range(5)}
    want = np.array([rank[b] for b in range(5)] + [-1])[group]
    assert nc == 5 and np.array_equal(lab, want)


def test_use_case_person_and_wall():
    pts = synth.filter_cloud(200_000)
    pts = pts[pts[:, 1] < synth.FLOOR_Y - 20]                  # floor removed
    pc = PointCloud(pts)
    lab = pc.cluster_dbscan(50.0, 10)
    person = (np.abs(pts[:, 2] - 2000) < 300) & (np.abs(pts[:, 0]) < 450)
    wall = np.abs(pts[:, 2] - 3500) < 15
    rest = ~person & ~wall
    lp = np.bincount(lab[person][lab[person] >= 0]).argmax()
    lw = np.bincount(lab[wall][lab[wall] >= 0]).argmax()
    assert lp != lw
    assert (lab[person] == lp).mean() > 0.9 and (lab[wall] == lw).mean() > 0.9
    assert (lab[rest] == -1).mean() > 0.8


def test_run_to_run_identical(base_cloud):
    a = ops.cluster_dbscan(base_cloud, 20.0, 10)
    b = ops.cluster_dbscan(base_cloud, 20.0, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_radius_outlier_matches_counts(base_cloud, oracle):
    rng = np.random.default_rng(6)
    pts = base_cloud[np.sort(rng.choice(len(base_cloud), 40_000, replace=False))]
    col = rng.random((len(pts), 3)).astype(np.float32)
    nrm = rng.standard_normal((len(pts), 3)).astype(np.float32)
    for radius, nb in ((10.0, 1), (20.0, 5), (35.5, 16)):
        cnt = R.counts(R.integer_neighbours(pts, radius)[0])
        want = np.flatnonzero(cnt > nb)
        keep = ops.remove_radius_outlier(pts, nb, radius).cpu().numpy()
        assert np.array_equal(keep, want)
        pc = PointCloud(pts)
        pc.colors = col
        pc.normals = nrm
        out, ind = pc.remove_radius_outlier(nb, radius)
        assert np.array_equal(ind, want)
        assert np.array_equal(np.asarray(out.points), pts[want]) and np.array_equal(np.asarray(out.colors), col[want])
        assert np.array_equal(np.asarray(out.normals), nrm[want])
    fc = synth.filter_cloud(30_000, seed=4)
    for radius, nb in ((15.0, 2), (40.0, 10)):
        cnt = R.counts(_oracle_nbrs(oracle, fc, radius)[0])
        assert np.array_equal(ops.remove_radius_outlier(fc, nb, radius).cpu().numpy(), np.flatnonzero(cnt > nb))
    with pytest.raises(RuntimeError, match="number of points and radius must be positive"):
        PointCloud(pts).remove_radius_outlier(0, 1.0)
    with pytest.raises(RuntimeError):
        PointCloud(pts).cluster_dbscan(0.0, 5)


def test_reachable_through_o3d_shim():
    from kinectpy_amd import o3d
    pc = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(_lattice(4, 4, 4)))
    assert np.all(pc.cluster_dbscan(NEXT1, 2) == 0)
    out, ind = pc.remove_radius_outlier(4, NEXT1)         # corners have 4 neighbours with themselves: dropped
    g = _lattice(4, 4, 4)
    corner = np.all((g == 0) | (g == 3), axis=1)
    assert np.array_equal(ind, np.flatnonzero(~corner)) and len(out.points) == 56

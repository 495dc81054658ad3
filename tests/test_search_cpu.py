"""CPU suite of the neighbour search: the brute-force reference agrees with SciPy's k-d tree on quantised
coordinates, the six C-ABI entries exist and are bound, every documented argument rejection happens before the device is touched,
KDTreeFlann refuses what is not a cloud."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import search_ref as R

NAMES = ("kpx_search_index_bytes", "kpx_search_index_build", "kpx_search_workspace_bytes", "kpx_search_knn", "kpx_search_radius_count",
         "kpx_search_radius_fill")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.load()


def test_reference_agrees_with_ckdtree():
    """index SETS per distance level (SciPy's order among equal distances is its own)"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(5)
    pts = R.quantised(rng, 700, -8, 8)
    qs = np.concatenate([R.quantised(rng, 60, -10, 10), pts[:10]])
    tree = cKDTree(pts.astype(np.float64))
    k = 12
    idx, d2, cnt = R.knn(pts, qs, k)
    dd, _ = tree.query(qs.astype(np.float64), k=k)
    assert np.all(cnt == k)
    assert np.array_equal(d2, dd * dd) or np.allclose(d2, dd * dd, rtol=1e-14, atol=0)
    D = R.d2_matrix(pts, qs)
    for i in range(len(qs)):
        assert np.array_equal(D[i, idx[i]], d2[i]) and np.all(np.diff(d2[i]) >= 0)
        for level in np.unique(d2[i]):
            mine = idx[i][d2[i] == level]
            assert np.all(np.diff(mine) > 0)                                    # the tie rule: ascending index
            every = np.flatnonzero(D[i] == level)
            if level < d2[i, -1]:
                assert np.array_equal(mine, every)                              # a level below the last is complete
            else:
                assert np.array_equal(mine, every[:len(mine)])                  # the last level: its lowest indices
    r = 2.5
    off, ridx, rd2 = R.radius(pts, qs, r)
    balls = tree.query_ball_point(qs.astype(np.float64), r)
    for i in range(len(qs)):
        seg = ridx[off[i]:off[i + 1]]
        inside = np.array(sorted(j for j in balls[i] if D[i, j] < r * r), dtype=np.int64)      # SciPy's ball is closed, ours strict
        assert np.array_equal(np.sort(seg), inside)
        assert np.all(np.diff(rd2[off[i]:off[i + 1]]) >= 0)


def test_symbols_exported_and_bound(lib):
    from kinectpy_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES


def test_sizes_are_host_arithmetic(lib):
    sizes = [lib.kpx_search_index_bytes(n) for n in (0, 1, 1000, 65536, 300_000, 5_000_000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert lib.kpx_search_index_bytes(5_000_000) > 5_000_000 * 16
    assert lib.kpx_search_workspace_bytes(1000, 8) >= 1000 * 4
    assert lib.kpx_search_workspace_bytes(100_000, 0) > lib.kpx_search_workspace_bytes(1000, 8)


_FAKE = C.c_void_p(4096)          # never dereferenced: the arguments are rejected first
_BIG = 1 << 30


@pytest.mark.parametrize("k,msg", [(0, b"at least 1"), (-3, b"at least 1"), (4097, b"4096")])
def test_knn_rejects_k(lib, k, msg):
    rc = lib.kpx_search_knn(_FAKE, _BIG, _FAKE, 10, k, 0.0, _FAKE, _FAKE, _FAKE, _FAKE, 1 << 20, None)
    assert rc == -1 and msg in lib.kpx_last_error()


@pytest.mark.parametrize("radius", [0.0, -1.0, math.nan])
def test_radius_calls_reject_radius(lib, radius):
    rc = lib.kpx_search_radius_count(_FAKE, _BIG, _FAKE, 10, radius, _FAKE, _FAKE, 1 << 20, None)
    assert rc == -1 and b"radius must be positive" in lib.kpx_last_error()
    rc = lib.kpx_search_radius_fill(_FAKE, _BIG, _FAKE, 10, radius, _FAKE, 5, _FAKE, _FAKE, _FAKE, 1 << 20, None)
    assert rc == -1 and b"radius must be positive" in lib.kpx_last_error()


def test_null_index_and_short_index(lib):
    calls = {
        "knn": lambda ix, nb: lib.kpx_search_knn(ix, nb, _FAKE, 10, 5, 0.0, _FAKE, _FAKE, _FAKE, _FAKE, 1 << 20, None),
        "count": lambda ix, nb: lib.kpx_search_radius_count(ix, nb, _FAKE, 10, 1.0, _FAKE, _FAKE, 1 << 20, None),
        "fill": lambda ix, nb: lib.kpx_search_radius_fill(ix, nb, _FAKE, 10, 1.0, _FAKE, 5, _FAKE, _FAKE, _FAKE, 1 << 20, None),
    }
    for name, call in calls.items():
        assert call(None, _BIG) == -1 and b"null index" in lib.kpx_last_error(), name
        assert call(_FAKE, lib.kpx_search_index_bytes(0) - 1) == -1 and b"index_bytes" in lib.kpx_last_error(), name
    rc = lib.kpx_search_index_build(_FAKE, 10, None, _BIG, _FAKE, 1 << 20, None)
    assert rc == -1 and b"null index" in lib.kpx_last_error()
    rc = lib.kpx_search_index_build(_FAKE, 1000, _FAKE, lib.kpx_search_index_bytes(1000) - 1, _FAKE, 1 << 20, None)
    assert rc == -1 and b"index_bytes" in lib.kpx_last_error()


def test_radius_fill_range(lib):
    rc = lib.kpx_search_radius_fill(_FAKE, _BIG, _FAKE, 10, 1.0, _FAKE, 1 << 31, _FAKE, _FAKE, _FAKE, 1 << 20, None)
    assert rc == -3 and b"2^31" in lib.kpx_last_error()


def test_kdtreeflann_refuses_non_clouds():
    from kinectpy_amd import o3d
    for bad in ("cloud", 5, 2.5, {"points": 1}, np.zeros((4, 2)), np.zeros(7), [[1.0, 2.0]], object()):
        with pytest.raises(TypeError):
            o3d.geometry.KDTreeFlann(bad)
    t = o3d.geometry.KDTreeFlann()
    with pytest.raises(TypeError):
        t.search_vector_3d([0, 0, 0], "knn")
    assert o3d.geometry.KDTreeSearchParamRadius(2).radius == 2.0
    assert hasattr(o3d.geometry.PointCloud, "compute_point_cloud_distance") and hasattr(o3d.geometry.PointCloud, "compute_nearest_neighbor_distance")

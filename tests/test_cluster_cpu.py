"""CPU suite for cluster_dbscan / remove_radius_outlier: the C-ABI entries exist, are bound, reject bad arguments before touching
the device, size their workspace on the host; the literal Open3D loop of the reference helper equals the closed form the kernels
compute ("Clustering")."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import dbscan_ref as R

NAMES = ("kpx_dbscan_workspace_bytes", "kpx_cluster_dbscan", "kpx_radius_outlier_workspace_bytes", "kpx_remove_radius_outlier")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from kinectpy_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES


_FAKE = C.c_void_p(4096)          # never dereferenced: the arguments are rejected first


@pytest.mark.parametrize("eps,min_points,msg", [(0.0, 5, b"eps"), (-1.0, 5, b"eps"), (math.nan, 5, b"eps"), (1.0, -1, b"min_points")])
def test_dbscan_rejects(lib, eps, min_points, msg):
    rc = lib.kpx_cluster_dbscan(_FAKE, 10, eps, min_points, _FAKE, _FAKE, _FAKE, 1 << 20, None)
    assert rc == -1 and msg in lib.kpx_last_error()


@pytest.mark.parametrize("nb_points,radius", [(0, 1.0), (-3, 1.0), (5, 0.0), (5, -2.0), (5, math.nan)])
def test_radius_outlier_rejects(lib, nb_points, radius):
    rc = lib.kpx_remove_radius_outlier(_FAKE, 10, nb_points, radius, _FAKE, _FAKE, _FAKE, 1 << 20, None)
    assert rc == -1
    assert lib.kpx_last_error() == b"Illegal input parameters, number of points and radius must be positive"


def test_workspace_monotone(lib):
    for f in (lib.kpx_dbscan_workspace_bytes, lib.kpx_radius_outlier_workspace_bytes):
        sizes = [f(n) for n in (0, 1, 1000, 65536, 65537, 300_000, 5_000_000)]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes)
        assert f(5_000_000) > 5_000_000 * 4


def _random_cloud(rng):
    n = int(rng.integers(1, 120))
    side = int(rng.integers(2, 12))
    return rng.integers(0, side, size=(n, 3)).astype(np.float64)


def test_loop_equals_closed_form():
    rng = np.random.default_rng(42)
    for case in range(300):
        pts = _random_cloud(rng)
        eps = float(rng.choice([1.0, np.nextafter(1.0, 2.0), 1.5, 2.0, 2.5, 3.2]))
        min_points = int(rng.choice([0, 1, 2, 3, 5, 8]))
        for _ in range(3):
            perm = rng.permutation(len(pts))
            p = pts[perm]
            ip, ix = R.integer_neighbours(p, eps)
            a = R.dbscan_loop(ip, ix, min_points)
            b = R.dbscan_closed_form(ip, ix, min_points)
            assert np.array_equal(a, b), (case, eps, min_points)


def test_loop_border_takes_smallest_cluster():
    pts, bridge, A, B = R.two_blobs_and_bridge()
    eps = float(np.nextafter(1.0, 2.0))
    rng = np.random.default_rng(0)
    for _ in range(100):
        perm = rng.permutation(len(pts))
        inv = np.argsort(perm)
        ip, ix = R.integer_neighbours(pts[perm], eps)
        lab = R.dbscan_loop(ip, ix, 4)
        assert np.array_equal(lab, R.dbscan_closed_form(ip, ix, 4))
        la, lb, lp = lab[inv[A]], lab[inv[B]], lab[inv[bridge]]
        assert len(set(la.tolist())) == 1 and len(set(lb.tolist())) == 1 and la[0] != lb[0]       # the bridge joins nothing
        assert lp == min(la[0], lb[0])
        assert sorted(set(lab.tolist())) == [-1, 0, 1]

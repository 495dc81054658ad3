"""The float64 sampled-row references of oracle/lineage2.py (sor_avg_at, hybrid_cov_at, normals_at) and the checks built on them
(check_sor_f64, check_normals_f64), on CPU: they agree with the C oracle, and each check rejects a result that is wrong by one index,
one neighbour, 1e-9 of the threshold or 1e-3 rad of a normal.  The GPU suite relies on these checks where the full oracle is too slow."""
import numpy as np
import pytest

from kinectpy_amd.utils import synth
from oracle import lineage2 as L2


@pytest.fixture(scope="module")
def cloud():
    """a frame-density sample, a sparse halo around it and a block of lattice points (ties at the k-th distance)"""
    rng = np.random.default_rng(11)
    base = synth.frame_cloud()
    p = base[rng.choice(len(base), 6000, replace=False)]
    lo, hi = p.min(0), p.max(0)
    halo = rng.uniform(lo - 300, hi + 300, size=(150, 3))
    g = np.arange(6, dtype=np.float64) * 4.0
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + lo
    q = np.concatenate([p, halo, lat]).astype(np.float32)
    return np.ascontiguousarray(q[rng.permutation(len(q))])


@pytest.mark.parametrize("k", [1, 20, 129])
def test_sor_avg_at_equals_the_oracle(oracle, cloud, k):
    rows = np.arange(0, len(cloud), 7)
    _, _, ra = oracle.sor(cloud, k, 2.0)
    avg, dk, dk1 = L2.sor_avg_at(cloud, k, rows, workers=4)
    assert np.allclose(avg, ra[rows], rtol=L2.TOL_AVG, atol=0)
    assert np.all(dk1 >= dk)


def test_hybrid_cov_and_normals_at_equal_the_oracle(oracle, cloud):
    rows = np.arange(0, len(cloud), 5)
    rn, cov, cnt = oracle.estimate_normals(cloud, 120.0, 60)
    c, C = L2.hybrid_cov_at(cloud, 120.0, 60, rows, workers=4)
    assert np.array_equal(c, cnt[rows])
    six = np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1)
    scale = np.abs(six).max(1, keepdims=True) + 1e-30
    ok = c >= 3                                                        # (the oracle leaves the covariance of smaller neighbourhoods at 0)
    assert ok.mean() > 0.9 and np.all(np.abs(six - cov[rows])[ok] <= 1e-9 * scale[ok])
    frac = L2.check_normals_f64(cloud, 120.0, 60, rn.astype(np.float32), rows, workers=4)
    assert frac > 0.8


@pytest.fixture(scope="module")
def sor_case(oracle, cloud):
    k, ratio = 20, 1.0
    keep, stats, avg = oracle.sor(cloud, k, ratio)
    rows = np.arange(0, len(cloud), 3)
    return k, ratio, keep, np.array(stats), avg, rows


def test_check_sor_accepts_the_oracle(cloud, sor_case):
    k, ratio, keep, stats, avg, rows = sor_case
    assert L2.check_sor_f64(cloud, k, ratio, keep, stats, avg, rows, workers=4) > len(rows) // 2


def test_check_sor_rejects_one_flipped_keep_index(cloud, sor_case):
    k, ratio, keep, stats, avg, rows = sor_case
    far = np.abs(avg - stats[2]) > 1e-3 * stats[2]
    dropped = np.flatnonzero(far & ~np.isin(np.arange(len(avg)), keep))[0]
    with pytest.raises(AssertionError, match="keep list"):
        L2.check_sor_f64(cloud, k, ratio, np.sort(np.append(keep, dropped)), stats, avg, rows, workers=4)
    sel = keep[far[keep]]
    kept = sel[len(sel) // 2]
    with pytest.raises(AssertionError, match="keep list"):
        L2.check_sor_f64(cloud, k, ratio, keep[keep != kept], stats, avg, rows, workers=4)


def test_check_sor_rejects_the_k_plus_first_neighbour(cloud, sor_case):
    """one sampled row's mean taken over neighbours 1 .. k-1 and k+1 instead of 1 .. k"""
    k, ratio, keep, stats, avg, rows = sor_case
    _, dk, dk1 = L2.sor_avg_at(cloud, k, rows, workers=4)
    r = int(np.flatnonzero(dk1 > dk)[0])
    bad = avg.copy()
    bad[rows[r]] += (dk1[r] - dk[r]) / k
    with pytest.raises(AssertionError, match="avg off"):
        L2.check_sor_f64(cloud, k, ratio, keep, stats, bad, rows, workers=4)


def test_check_sor_rejects_a_threshold_off_by_1e9(cloud, sor_case):
    k, ratio, keep, stats, avg, rows = sor_case
    bad = stats.copy()
    bad[2] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="statistics"):
        L2.check_sor_f64(cloud, k, ratio, keep, bad, avg, rows, workers=4)


def test_check_normals_rejects_a_tilt_of_1e3_rad(oracle, cloud):
    rows = np.arange(0, len(cloud), 5)
    rn, _, _ = oracle.estimate_normals(cloud, 120.0, 60)
    _, well, _ = L2.normals_at(cloud, 120.0, 60, rows, workers=4)
    i = rows[np.flatnonzero(well)[0]]
    n = rn[i]
    axis = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    axis /= np.linalg.norm(axis)
    bad = rn.copy()
    bad[i] = np.cos(1e-3) * n + np.sin(1e-3) * axis                    # rotated by 1e-3 rad about an axis orthogonal to n
    L2.check_normals_f64(cloud, 120.0, 60, rn, rows, workers=4)
    with pytest.raises(AssertionError, match="normal off"):
        L2.check_normals_f64(cloud, 120.0, 60, bad, rows, workers=4)


def test_sampled_rows_resolve_ties_past_the_query_window():
    """an integer lattice where k = 40 cuts through the shell of 24 points at d^2 = 5 (33 points are closer), past the k + 17 rows the tree
    is asked for: the rule (d^2, index) holds, not the tree's order"""
    g = np.arange(9, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rows = np.array([4 * 81 + 4 * 9 + 4])                              # the centre
    avg, dk, dk1 = L2.sor_avg_at(p, 40, rows, workers=1)
    want = (6 * 1.0 + 12 * np.sqrt(2.0) + 8 * np.sqrt(3.0) + 6 * 2.0 + 7 * np.sqrt(5.0)) / 40
    assert np.isclose(avg[0], want, rtol=1e-15) and dk[0] == dk1[0] == np.sqrt(5.0)
    cnt, _ = L2.hybrid_cov_at(p, 2.5, 40, rows, workers=1)
    assert cnt[0] == 40
    q = p.astype(np.float64)
    brute = np.lexsort((np.arange(len(p)), ((q - q[rows[0]]) ** 2).sum(1)))[:40]
    tree_idx, _, _ = L2._kth_cut(L2.cKDTree(q), q, q[rows], 40, 1)
    assert np.array_equal(tree_idx[0], brute)

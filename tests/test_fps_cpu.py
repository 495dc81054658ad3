"""The vectorised farthest-point reference (tests/fps_ref.py) against the literal loop, and its exactness check -- no GPU."""
import numpy as np
import pytest

from tests import fps_ref as R


def _clouds():
    rng = np.random.default_rng(5)
    yield "random", rng.integers(-500, 500, size=(150, 3)).astype(np.float32)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 10.0
    yield "lattice", g.astype(np.float32)
    yield "lattice_permuted", g[rng.permutation(len(g))].astype(np.float32)
    yield "duplicates", np.tile(np.float32([[3, -7, 1200]]), (40, 1))
    dup = np.tile(np.float32([[0, 0, 1000]]), (30, 1))
    dup[17] = (100, 0, 1000)
    yield "duplicates_and_one_outlier", dup
    yield "float_random", rng.normal(scale=300.0, size=(120, 3)).astype(np.float32)


@pytest.mark.parametrize("name,pts", list(_clouds()), ids=[c[0] for c in _clouds()])
def test_vectorised_reference_equals_the_loop(name, pts):
    n = len(pts)
    for start in (0, n // 2, n - 1):
        for k in (1, 2, n // 3, n - 1, n):
            s1, c1 = R.fps_loop(pts, k, start)
            s2, c2 = R.fps(pts, k, start)
            assert np.array_equal(s1, s2), (name, start, k)
            assert np.array_equal(c1.view(np.int64), c2.view(np.int64)), (name, start, k)
            assert np.all(np.diff(c2) <= 0)


def test_all_zero_rule_repeats_the_previous_index():
    pts = np.tile(np.float32([[0, 0, 1000]]), (10, 1))
    pts[4] = (50, 0, 1000)
    sel, cover = R.fps(pts, 5, 7)
    # 7 -> the outlier 4 -> every distance is 0 from then on: 4 repeats (np.argmax alone would pick 0)
    assert sel.tolist() == [7, 4, 4, 4, 4]
    assert cover.tolist() == [2500.0, 0.0, 0.0, 0.0, 0.0]
    s1, c1 = R.fps_loop(pts, 5, 7)
    assert np.array_equal(sel, s1) and np.array_equal(cover, c1)


def test_ties_take_the_smallest_index():
    pts = np.float32([[0, 0, 0], [10, 0, 0], [-10, 0, 0], [0, 10, 0], [0, -10, 0]])
    sel, cover = R.fps(pts, 3, 0)
    assert sel.tolist() == [0, 1, 2] and cover.tolist() == [100.0, 100.0, 100.0]


def test_squares_exact_accepts_integer_mm_and_rejects_an_inexact_cloud():
    rng = np.random.default_rng(1)
    mm = rng.integers(-4000, 4000, size=(1000, 3)).astype(np.float32)
    assert R.squares_exact(mm)
    R.assert_squares_exact(mm)
    half = np.float32([[0.5, 0.25, 1000.0], [1.0, 0.75, 1200.5]])          # few-bit fractions: exact by the pairwise check
    assert R.squares_exact(half)
    bad = np.float32([[1048576.0, 0, 0], [0.0009765625, 0, 0]])            # dx = 2^20 - 2^-10: 31 significant bits
    assert R.two_product_err(bad[0, 0] - np.float64(bad[1, 0]), bad[0, 0] - np.float64(bad[1, 0])) != 0.0
    assert not R.squares_exact(bad)
    with pytest.raises(AssertionError):
        R.assert_squares_exact(bad)

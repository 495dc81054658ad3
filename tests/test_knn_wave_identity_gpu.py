"""The wave-per-query neighbour kernels (knn_wave_kernel: remove_statistical_outlier, estimate_normals, estimate_covariances) reduce,
scan and broadcast on the vector ALU (csrc/kpx_wave.h) instead of through ds_bpermute, SOR takes its square roots once per selected
candidate, and the frame's voxel keys are formed in 32-bit words.  None of that may move a bit: integer sums, minima and maxima are
exact in any order and the floating-point sums keep their tree.

Expected values: tests/golden/knn_wave_parent_*.npz, recorded by tests/golden/make_knn_wave_golden.py with the build of commit
97ba49b (the commit before the change; the full id is in every file).  Clouds and calls: tests/knn_wave_cases.py -- a noisy patch, fewer
points than k, a lattice whose k-th shell is cut by the index rule, 30 % exact duplicates, a clump beyond the first pass's buffer, a
radius that leaves queries with fewer than three neighbours; and one four-sensor frame through the native frame loop, which covers
the 32-bit key path and the order it gives the fused cloud."""
import os

import numpy as np
import pytest

import knn_wave_cases as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARENT = "97ba49b"


def golden(name):
    g = dict(np.load(os.path.join(GOLDEN, "knn_wave_parent_%s.npz" % name)))
    commit = str(g.pop("parent_commit"))
    assert len(commit) == 40 and commit.startswith(PARENT), commit
    return g


def compare(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
        assert np.array_equal(got[key], want[key]) and S.same_bits(got[key], want[key]), \
            (what, key, int((got[key] != want[key]).sum()), got[key].ravel()[:4], want[key].ravel()[:4])


def test_recorded_cases_are_what_they_claim():
    """what the recorded values are worth: sizes, the degenerate results where the cases ask for them"""
    for name in S.CASES:
        g, n = golden(name), len(S.cloud(name))
        assert n <= 5000 and g["sor.avg"].shape == (n,) and g["normals"].shape == (n, 3) and g["cov"].shape == (n, 3, 3), name
        assert np.all(np.diff(g["sor.keep"]) > 0) and 0 < len(g["sor.keep"]) <= n, name
    flat = lambda g: np.all(g["normals"] == np.array([0, 0, 1], np.float32), axis=1) & np.all(g["cov"] == np.eye(3), axis=(1, 2))
    assert 50 <= flat(golden("sparse")).sum() < len(S.cloud("sparse")) // 2            # the isolated points, not the patch
    assert not flat(golden("patch")).any()
    pts = S.cloud("few").astype(np.float64)                                              # m <= k: the mean over all 15 points, itself included
    d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    assert np.allclose(golden("few")["sor.avg"], d.sum(1) / 15.0, rtol=1e-12)
    lat = golden("lattice")["sor.avg"]                                                   # interior: 0, 6 x 10, 12 x 10 sqrt 2, one of the 8 at 10 sqrt 3
    assert np.isclose(lat.min(), (60.0 + 120.0 * np.sqrt(2.0) + 10.0 * np.sqrt(3.0)) / 20.0, rtol=1e-12)
    # the k-th distance is shared and the index rule decides: around an interior lattice point 19 points lie nearer than d^2 = 300 and
    # 27 at or below it (k = 20 cuts the shell of 8), 27 nearer than 400 and 33 at or below it (max_nn = 30 cuts the shell of 6)
    lp = S.cloud("lattice").astype(np.float64)
    inner = lp[np.all((lp >= 30.0) & (lp <= 80.0), axis=1)][0]
    d2 = ((lp - inner) ** 2).sum(1)
    assert ((d2 < 300).sum(), (d2 <= 300).sum(), (d2 < 400).sum(), (d2 <= 400).sum()) == (19, 27, 27, 33)
    assert S.SOR[0] == 20 and S.CASES["lattice"]["max_nn"] == 30 and S.CASES["lattice"]["radius"] ** 2 > 400
    # more candidates at ONE distance than the first pass's buffer holds (512 at k <= 32 / max_nn <= 48): even the ball of the k-th
    # candidate overflows it, so the copies' queries are truncated, gathered again and handed to the next pass
    _, mult = np.unique(S.cloud("clump"), axis=0, return_counts=True)
    assert mult.max() == 600 > 512 and (mult > 1).sum() == 1
    dup = golden("duplicates")["sor.avg"]
    assert (dup > 0).all() and len(np.unique(S.cloud("duplicates"), axis=0)) == 1400
    f = golden("frame")
    assert f["points"].shape == f["colours"].shape and f["points"].shape[0] > 5000 and f["transforms"].shape[-2:] == (4, 4)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_sor_normals_covariances_equal_the_parent(name):
    from kinectpy_amd import ops
    compare(S.run_case(ops, name), golden(name), name)


def test_frame_step_equals_the_parent():
    compare(S.run_frame(), golden("frame"), "frame")

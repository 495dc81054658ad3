"""The group pass of the neighbour search (knn_group_kernel, csrc/kpx_gridknn.h): a query per row of 16 lanes, four queries per wave; it
settles the common path -- the clipped 3 x 3 x 3 block, not truncated, the k-th inside the cover, a high-word pivot with exactly k
candidates at or below it -- and lists every other query for the unchanged wave-per-query passes behind it.  It stands in front of
remove_statistical_outlier / kpx_sor_partial (k <= 32) and estimate_normals / estimate_covariances (max_nn <= 48), and none of their
results may move a bit: the sums keep the association of the wave form, and a listed query gets what it always got.

Expected values: tests/golden/knn_group_parent_*.npz, recorded by tests/golden/make_knn_group_golden.py with the build of commit 36949ed
(the commit before the change; the full id is in every file), and, for the calls of tests/knn_wave_cases.py, the files of
tests/test_knn_wave_identity_gpu.py.  Clouds and calls: tests/knn_group_cases.py.  So that handing on cannot hide a broken settle path,
ops.knn_group_last() -- the queries the last group pass was given and the ones it handed on -- is asserted where a case is built to
settle, to hand on, or to do both."""
import os

import numpy as np
import pytest

import knn_group_cases as S
import knn_wave_cases as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARENT = "36949ed"
_ran = {}


def golden(name, family="knn_group"):
    g = dict(np.load(os.path.join(GOLDEN, "%s_parent_%s.npz" % (family, name))))
    commit = str(g.pop("parent_commit"))
    assert len(commit) == 40 and (family != "knn_group" or commit.startswith(PARENT)), commit
    return g


def ran(name):
    """-> (arrays, group-pass counts by call) of one case, computed once"""
    if name not in _ran:
        from kinectpy_amd import ops
        counts = {}
        _ran[name] = (S.run_case(ops, name, counts), counts)
    return _ran[name]


def compare(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
        assert got[key].tobytes() == want[key].tobytes(), \
            (what, key, int((got[key] != want[key]).sum()), got[key].ravel()[:4], want[key].ravel()[:4])


def test_cases_are_what_they_claim():
    for name in S.CASES:
        assert len(S.cloud(name)) <= 5000, name
    assert [len(S.cloud("tiny_%d" % n)) for n in (1, 2, 3, 5, 41)] == [1, 2, 3, 5, 41] and 41 % 4 == 1
    slab = S.cloud("slab")
    assert np.ptp(slab[:, 2]) <= 1.0 and np.ptp(slab[:, 0]) > 600.0                      # far thinner than any cell of ~8 points
    assert all(G + d in S.STRADDLE for G in S.GROUP_CAP.values() for d in (-1, 0, 1))
    for c in S.STRADDLE:
        p = S.cloud("straddle_%d" % c).astype(np.float64)
        near = np.all(np.abs(p - 1000.0) <= 2.0, axis=1)
        assert near.sum() == c and np.all(np.abs(p[~near] - 1000.0).min(axis=1) >= 800.0), c
    for q0, q1 in S.PARTIAL_RANGES[1:-1]:
        assert q0 % 4 or q1 % 4
    for name in S.CASES:                                                                  # every recorded array is there and is the parent's
        g = golden(name)
        assert g, name


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_equals_the_parent(name):
    compare(ran(name)[0], golden(name), name)


def test_partial_ranges_equal_the_rows_of_the_full_call():
    got = ran("partial")[0]
    (f0, f1), full = S.PARTIAL_RANGES[0], got["partial_%d_%d.avg" % S.PARTIAL_RANGES[0]]
    assert (f0, f1) == (0, len(S.cloud("partial"))) and full.shape == (f1,)
    for q0, q1 in S.PARTIAL_RANGES[1:]:
        part = got["partial_%d_%d.avg" % (q0, q1)]
        assert part.shape == (q1 - q0,) and part.tobytes() == full[q0:q1].tobytes(), (q0, q1)


def _wave_case_counts(name):
    """the calls of tests/knn_wave_cases.py (SOR (20, 2.0), the case's hybrid normals) -> group-pass counts, results checked against that
    test's recorded values"""
    import torch
    from kinectpy_amd import ops
    want = golden(name, "knn_wave")
    pts = torch.as_tensor(W.cloud(name)).cuda()
    _, _, avg = ops.sor(pts, W.SOR[0], W.SOR[1], want_avg=True)
    sor = ops.knn_group_last()
    assert avg.cpu().numpy().tobytes() == want["sor.avg"].tobytes(), name
    nrm = ops.estimate_normals(pts, W.CASES[name]["radius"], W.CASES[name]["max_nn"])
    normals = ops.knn_group_last()
    assert nrm.cpu().numpy().tobytes() == want["normals"].tobytes(), name
    n = len(pts)
    print(name, "sor (given, handed on)", sor, "normals", normals)
    assert sor[0] == n and normals[0] == n and 0 <= sor[1] <= n and 0 <= normals[1] <= n
    return sor, normals


def test_patch_settles_in_the_group_pass():
    """the common path: cells of about 48 mm against a 20th-neighbour distance of about 40 mm -- nearly every interior query is covered"""
    sor, normals = _wave_case_counts("patch")
    assert 2 * sor[1] <= sor[0] and 2 * normals[1] <= normals[0], (sor, normals)


@pytest.mark.parametrize("name", ["lattice", "clump"])
def test_ties_and_overflow_are_handed_on(name):
    """a shell of equal distances at the k-th (lattice), 600 copies of one point (clump): never settled by a high-word pivot"""
    sor, normals = _wave_case_counts(name)
    assert sor[1] >= 1 and normals[1] >= 1, (sor, normals)


def test_dense_and_sparse_rows_side_by_side():
    counts = ran("alternate")[1]
    n = len(S.cloud("alternate"))
    for key in ("sor20", "nrm70_30"):
        given, handed = counts[key]
        print("alternate", key, (given, handed))
        assert given == n and 20 * handed >= n and 20 * (given - handed) >= n, (key, given, handed)


def test_candidate_counts_around_the_group_buffer():
    """c candidates in the block of every clump query: below the buffer they settle (up to the rare shared high word), at and above it
    every one of them is handed on"""
    for key, G in S.GROUP_CAP.items():
        for c in (G - 1, G, G + 1):
            given, handed = ran("straddle_%d" % c)[1][key]
            print("straddle", c, key, (given, handed))
            assert given == c + 40
            if c < G:                                                                     # (the 40 far points may all be handed on)
                assert 10 * (handed - 40) <= c, (c, key, handed)
            else:
                assert handed >= c, (c, key, handed)

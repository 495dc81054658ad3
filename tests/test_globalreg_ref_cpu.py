"""The global-registration references of tests/globalreg_ref.py on CPU: the order-free argmin and the FPFH bin-edge check accept the C
oracle's output and reject planted faults; the RANSAC bookkeeping and the oracle's flat-triple rule and iteration count behave as the
GPU suite (test_global_registration_gpu.py) relies on."""
import numpy as np
import pytest

import globalreg_ref as R
from kinectpy_amd.utils import synth


def test_argmin_ref_equals_the_oracle_and_takes_the_lowest_tie(oracle):
    rng = np.random.default_rng(1)
    for na, nb in ((1, 1), (17, 129), (300, 2049)):
        fa = rng.integers(0, 3, size=(na, 33)).astype(np.float64)
        fb = rng.integers(0, 3, size=(nb, 33)).astype(np.float64)
        h = nb // 2
        fb[h:2 * h] = fb[:h]                                       # every row past h repeats one below h
        fb[2 * h:] = fb[:nb - 2 * h]
        want = R.argmin_ref(fa, fb)
        assert np.array_equal(want, oracle.feature_nn(fa, fb))
        if nb > 1:
            assert np.all(want < h)
            bad = want.copy()
            bad[0] += h                                            # the same distance at a higher index
            assert not np.array_equal(bad, oracle.feature_nn(fa, fb))
    with pytest.raises(AssertionError):
        R.argmin_ref(np.full((1, 33), 0.5), np.zeros((1, 33)))     # not an integer feature: the reference does not apply


def test_fnn_splits_and_ransac_chunks():
    assert R.fnn_splits(1, 40000) == 16 and R.fnn_splits(65536, 129) == 1 and R.fnn_splits(32768, 129) == 2
    assert R.fnn_splits(8192, 2049) == 8 and R.fnn_splits(64, 127) == 1 and R.fnn_splits(65, 2049) == 16
    assert R.fnn_place(16 * 128, 64, 2049)[:2] == (0, 16) and R.fnn_place(5 * 128 + 19, 64, 2049) == (5, 5, 3, 1)
    assert [R.ransac_chunk(k) for k in (0, 63, 64, 575, 576, 1087, 1088)] == [0, 0, 1, 1, 2, 2, 3]


@pytest.fixture(scope="module")
def edge_cloud():
    """a lattice with axis normals, plus a pair whose f2 sits exactly on a bin edge: offset (9, 6, 2) (length 11) against the
    normal (1, 0, 0) gives f2 = 9/11, binned coordinate 11 (9/11 + 1) / 2 = 10"""
    g = np.arange(5, dtype=np.float64) * 3.0
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    nrm = np.tile([0.0, 0.0, 1.0], (len(p), 1))
    q = np.array([[100.0, 100.0, 100.0], [109.0, 106.0, 102.0]])
    qn = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return np.concatenate([p, q]).astype(np.float32), np.concatenate([nrm, qn]).astype(np.float32)


def test_fpfh_edge_flags_find_the_planted_edge_pair(oracle, edge_cloud):
    p, n = edge_cloud
    nbr, cnt, d2 = oracle.hybrid_knn_d2(p, 12.0, 40)
    flags = R.fpfh_edge_flags(p, n, nbr, cnt)
    assert flags[-2:, 2].tolist() == [1, 1] and flags[:-2].sum() == 0
    x = R.pair_bins(p[-2:-1], n[-2:-1], p[-1:], n[-1:])
    assert abs(x[0, 2] - 10.0) < 1e-14


def test_check_fpfh_accepts_the_oracle_and_rejects_planted_faults(oracle, edge_cloud):
    p, n = edge_cloud
    want, _ = oracle.fpfh(p, n, 12.0, 40)
    nbr, cnt, d2 = oracle.hybrid_knn_d2(p, 12.0, 40)
    flags = R.fpfh_edge_flags(p, n, nbr, cnt)
    assert R.check_fpfh(want.copy(), want, flags, nbr, cnt, d2) == 2
    rows_ok = np.nonzero(cnt > 1)[0][:3]
    for i in rows_ok:                                               # an untouched row, off by 1e-6 in one bin
        bad = want.copy()
        bad[i, 22 + np.argmax(want[i, 22:])] += 1e-6
        with pytest.raises(AssertionError):
            R.check_fpfh(bad, want, flags, nbr, cnt, d2)
    t = len(p) - 2                                                 # the touched row: one bin move of its flagged pair is allowed
    inc = 100.0 / (cnt[t] - 1)
    moved = want.copy()
    moved[t, 22 + 9] += inc
    moved[t, 22 + 10] -= inc
    R.check_fpfh(moved, want, flags, nbr, cnt, d2)
    twice = want.copy()                                            # more than its own and its neighbour's flagged pair can move is not
    twice[t, 22 + 8] += 3 * inc
    twice[t, 22 + 10] -= 3 * inc
    with pytest.raises(AssertionError):
        R.check_fpfh(twice, want, flags, nbr, cnt, d2)
    lost = want.copy()                                             # mass lost: the per-feature sum changes
    lost[t, 22 + 10] -= 0.5 * inc
    with pytest.raises(AssertionError):
        R.check_fpfh(lost, want, flags, nbr, cnt, d2)
    moved_f0 = want.copy()                                         # a move in a feature without a flagged pair
    moved_f0[t, 0] += inc
    moved_f0[t, 1] -= inc
    with pytest.raises(AssertionError):
        R.check_fpfh(moved_f0, want, flags, nbr, cnt, d2)


def _draws(oracle, nc, seed, iters):
    """the oracle's (and the kernel's) three picks of iteration itr: Philox(ctr = (0, itr, 1, 0), key = seed), (u nc) >> 32"""
    out = []
    for itr in range(iters):
        u = oracle.philox4x32([0, itr, 1, 0], [seed & 0xFFFFFFFF, seed >> 32])
        out.append([(int(u[q]) * nc) >> 32 for q in range(3)])
    return np.array(out)


def test_oracle_rejects_flat_triples_and_counts_iterations(oracle):
    """three true correspondences: a draw that repeats one is a flat triple (rejected); a draw of all three passes.  With confidence
    0.999 the first validation has inlier ratio 1, est_k drops to 0 and the loop ends at the next iteration."""
    base = synth.frame_cloud()
    src, tgt, _ = R.corres_scene(base, 300, 0.0, 0.0, 10, 2)
    corr = np.array([[0, 0], [50, 50], [120, 120]], dtype=np.int32)
    d = _draws(oracle, 3, 11, 400)
    distinct = np.array([len(set(r)) == 3 for r in d])
    _, st = oracle.ransac_corres(src, tgt, corr, 20.0, 3, 0.95, 400, 1.0, 11)
    assert st["validations"] == distinct.sum() and 0 < st["validations"] < 400
    _, st = oracle.ransac_corres(src, tgt, corr, 20.0, 3, 0.95, 400, 0.999, 11)
    assert st["validations"] == 1 and st["iterations"] == int(np.argmax(distinct)) + 1
    line = np.stack([np.arange(30.0), 2 * np.arange(30.0), np.zeros(30)], 1).astype(np.float32)
    _, st = oracle.ransac_corres(line, line, np.stack([np.arange(30), np.arange(30)], 1).astype(np.int32), 5.0, 3, 0.95, 500, 0.999, 1)
    assert st["validations"] == 0 and st["iterations"] == 500


def test_ransac_path_bookkeeping(oracle):
    base = synth.frame_cloud()
    src, tgt, corr = R.corres_scene(base, 600, 0.15, 0.0, 1000, 3)
    _, st, path = R.ransac_path(oracle, src, tgt, corr, 20.0, 40000, 1.0, 2)
    assert not path["exit"] and len(path["survivors"]) == 2 and sum(path["survivors"]) == st["validations"]
    _, st2, path2 = R.ransac_path(oracle, src, tgt, corr, 20.0, 40000, 0.99, 2)
    assert path2["exit"] and path2["stop_batch"] == 0 and path2["stop_k"] == st2["validations"] < path["survivors"][0]

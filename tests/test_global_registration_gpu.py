"""GPU suite (-m gpu): global registration (rows a11-a13) across its batch, chunk, split and tie paths.

feature_nn is checked bit for bit at the row-block (64 rows), stage (128 columns) and split boundaries, with ties placed across lanes,
stages and splits, against an order-free float64 argmin (integer features: every distance is exact) and the oracle; RANSAC on
synthetic correspondence sets whose path through the batched loop (survivors per batch of 32768, the speculative chunk of 64, the
chunks of 512, the est_k exit) is read from the oracle's own counts; FPFH on edge clouds with the bin-edge check of
tests/globalreg_ref.py; the whole chain at the reference's default voxel.  The library's constants are restated in globalreg_ref.py
and must be moved with kpx_fpfh.hip's."""
import numpy as np
import pytest

import globalreg_ref as R
from kinectpy_amd.utils import synth
from oracle import lineage2 as L2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


def npy(t):
    return t.cpu().numpy()


# ----------------------------------------------------------------- A. feature_nn
FNN_SHAPES = [(1, 40000), (17, 1), (15, 2), (16, 127), (63, 128), (64, 129), (65, 2047), (64, 2049), (65, 40000),
              (8192, 2049), (16000, 2047), (32768, 129), (65536, 129), (65537, 2)]


@pytest.mark.parametrize("na,nb", FNN_SHAPES)
def test_feature_nn_integer_features_exact(ops, oracle, na, nb):
    rng = np.random.default_rng(na * 7 + nb)
    fa = rng.integers(0, 4, size=(na, 33)).astype(np.float64)
    fb = rng.integers(0, 4, size=(nb, 33)).astype(np.float64)
    got = npy(ops.feature_nn(fa, fb))
    want = R.argmin_ref(fa, fb)
    assert np.array_equal(got, want)
    assert np.array_equal(got, oracle.feature_nn(fa, fb))


def test_feature_nn_shapes_cross_every_split_form():
    splits = {R.fnn_splits(na, nb) for na, nb in FNN_SHAPES}
    assert {1, 2, 16} <= splits and any(1 < s < 16 for s in splits - {2})
    assert {na % 64 for na, _ in FNN_SHAPES} >= {0, 1, 15, 16, 17, 63} and {nb % 128 for _, nb in FNN_SHAPES} >= {0, 1, 2, 127}


@pytest.mark.parametrize("na,nb", [(64, 2049), (65, 40000), (8192, 2049), (1, 300)])
def test_feature_nn_ties_across_lanes_stages_and_splits(ops, oracle, na, nb):
    rng = np.random.default_rng(5)
    fa = rng.integers(0, 4, size=(na, 33)).astype(np.float64)
    fb = rng.integers(0, 4, size=(nb, 33)).astype(np.float64)
    S = R.fnn_splits(na, nb)
    v = np.full(33, 7.0)
    cand = [c for c in (5 * 128 + 3, 5 * 128 + 19, 5 * 128 + 4, 16 * 128, 1 * 128 + 127, 2 * 128 + 64, 0 * 128 + 200) if c < nb]
    fb[cand] = v
    zeros = [c for c in (3 * 128 + 9, 12 * 128 + 1, 16 * 128 + 1, 250, 130) if c < nb]
    fb[zeros] = 0.0
    fa[0::3] = v
    fa[1::3] = 0.0
    place = [R.fnn_place(c, na, nb) for c in cand]
    if S > 1 and nb > 16 * 128:      # copies in several splits and stages, in one lane group and in different lanes, the lowest not in split 0
        assert len({p[0] for p in place}) >= 3 and len({p[1] for p in place}) >= 3 and len({p[2] for p in place}) >= 3
        assert R.fnn_place(min(cand), na, nb)[0] != 0
    got = npy(ops.feature_nn(fa, fb))
    assert np.all(got[0::3] == min(cand)) and np.all(got[1::3] == min(zeros))
    assert np.array_equal(got, R.argmin_ref(fa, fb)) and np.array_equal(got, oracle.feature_nn(fa, fb))


@pytest.fixture(scope="module")
def view_clouds(oracle):
    """the two cluttered views of test_parity_gpu's two_views, before down-sampling"""
    xy, ex = synth.xy_table(), synth.clutter()
    out = []
    for i, seed in ((0, 100), (1, 101)):
        E = synth.camera_pose(i, 16)
        dep = synth.render_depth(E, seed=seed, xy=xy, extra=ex)
        out.append((E, oracle.rgbd_compact(oracle.unproject_u16(dep, xy))[0]))
    return out


@pytest.mark.parametrize("voxel", [60.0, 40.0])
def test_feature_nn_real_features(ops, oracle, view_clouds, voxel):
    feats = []
    for _, p in view_clouds:
        d = oracle.voxel_downsample(p, voxel)[0]
        nrm = npy(ops.estimate_normals(d, 2 * voxel, 40))
        feats.append(oracle.fpfh(d, nrm, 5 * voxel, 40)[0])
    got = npy(ops.feature_nn(feats[1], feats[0]))
    assert np.array_equal(got, oracle.feature_nn(feats[1], feats[0]))
    rows = np.arange(0, len(got), 5)
    exc, bound = R.nn_dist_excess(feats[1][rows], feats[0], got[rows])
    assert np.all(exc >= 0) and np.all(exc <= bound)


def test_feature_nn_extreme_features_stay_in_range(ops, oracle):
    """finite features of ~1e150 (every distance beyond |a|^2 + 1e300), NaN and inf rows: every index in [0, nb), equal to the oracle's"""
    rng = np.random.default_rng(3)
    for na, nb in ((50, 100), (70, 129), (3, 1)):
        fa = rng.normal(size=(na, 33)) * 1e150
        fb = rng.normal(size=(nb, 33)) * 1e150
        fa[1, 4] = np.nan
        fa[2, 0] = np.inf
        if na > 5:
            fa[5] = 1e300                     # |a|^2 overflows
        if nb > 3:
            fb[3, 7] = np.nan
            fb[2, 1] = -np.inf
        got = npy(ops.feature_nn(fa, fb))
        assert got.min() >= 0 and got.max() < nb
        assert np.array_equal(got, oracle.feature_nn(fa, fb))
        corr = ops.feature_correspondences(fa, fb, True, 3)
        assert np.array_equal(corr, oracle.feature_correspondences(fa, fb, True, 3))
        assert corr[:, 0].max() < na and corr[:, 1].max() < nb


# ----------------------------------------------------------------- B. RANSAC control flow
CONF_MAX = 1.0 - 2.0 ** -52          # the largest confidence below 1: the longest est_k a ratio allows
# name: (n_src, true fraction, second-motion fraction, n_corres, scene seed, target noise sigma, max_dist, max_iteration, confidence,
#        ransac seed, expected path)
RANSAC_CASES = {
    "le64_survivors": (3000, 0.1, 0.0, 2000, 1, 0.0, 20.0, 32768, 1.0, 7, dict(surv=(1, 64), exit=False)),
    "65_576_survivors": (3000, 0.2, 0.0, 2000, 1, 0.0, 20.0, 32768, 1.0, 7, dict(surv=(65, 576), exit=False)),
    "gt576_survivors": (1000, 0.3, 0.0, 2000, 1, 0.0, 20.0, 32768, 1.0, 7, dict(surv=(577, None), exit=False)),
    "exit_in_spec_chunk": (1000, 0.3, 0.0, 2000, 1, 0.0, 20.0, 250000, 0.99, 7, dict(exit=True, batch=0, chunk=0)),
    "exit_in_later_chunk": (2000, 0.3, 0.3, 2000, 0, 0.0, 20.0, 250000, CONF_MAX, 7, dict(exit=True, batch=0, chunk=1)),
    "exit_at_chunk_start": (2000, 0.3, 0.3, 2000, 0, 0.0, 20.0, 250000, CONF_MAX, 23, dict(exit=True, batch=0, k=64)),
    "exit_in_batch2": (2000, 0.05, 0.0, 2000, 1, 0.0, 20.0, 250000, 0.999, 7, dict(exit=True, batch=1)),
    "three_batches_kept": (2000, 0.1, 0.0, 2000, 0, 2.0, 20.0, 70000, 1.0, 7, dict(exit=False, batches=3, kept=True)),
}
MAX_ITERATIONS = (1, 64, 65, 32767, 32768, 32769)


def _scene(base_cloud, n, f1, f2, nc, sd, sigma):
    src, tgt, corr = R.corres_scene(base_cloud, n, f1, f2, nc, sd)
    if sigma:
        tgt = (tgt + np.random.default_rng(sd).normal(0, sigma, tgt.shape)).astype(np.float32)
    return src, tgt, corr


def _check_against_oracle(ops, oracle, src, tgt, corr, max_dist, max_iter, conf, seed, oT=None, ost=None):
    g = ops.ransac_corres(src, tgt, corr, max_dist, 3, 0.95, max_iter, conf, seed)
    if ost is None:
        oT, ost = oracle.ransac_corres(src, tgt, corr, max_dist, 3, 0.95, max_iter, conf, seed)
    assert (g["iterations"], g["validations"]) == (ost["iterations"], ost["validations"])
    assert g["fitness"] == ost["fitness"]
    # the two Kabsch constructions (eigenvectors of S^T S / Horn's quaternion) agree to ~1e-12 in T; with an exact synthetic motion
    # the rmse is ~1e-4 and that difference is 1e-8 of it: relative 1e-9 above 1, absolute 1e-9 below
    assert abs(g["inlier_rmse"] - ost["rmse"]) <= 1e-9 * max(ost["rmse"], 1.0)
    T = g["transformation"]
    assert np.abs(T - oT).max() < 1e-6
    assert np.array_equal(T[3], [0, 0, 0, 1])
    if g["validations"]:
        Rm = T[:3, :3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12
    else:
        assert np.array_equal(T, np.eye(4)) and g["fitness"] == 0.0 and g["inlier_rmse"] == 0.0
    if max_dist > 0 and len(corr) >= 3:
        fit, rmse, _ = L2.evaluate_registration(src, tgt, max_dist, T)           # float64 re-score with a k-d tree
        assert fit == g["fitness"] and abs(rmse - g["inlier_rmse"]) <= 1e-9 * max(rmse, 1.0)
    return g, ost


@pytest.mark.parametrize("name", list(RANSAC_CASES))
def test_ransac_paths_match_oracle(ops, oracle, base_cloud, name):
    n, f1, f2, nc, sd, sigma, md, mi, conf, seed, want = RANSAC_CASES[name]
    src, tgt, corr = _scene(base_cloud, n, f1, f2, nc, sd, sigma)
    oT, ost, path = R.ransac_path(oracle, src, tgt, corr, md, mi, conf, seed)
    # the path this case exists for, from the oracle's counts
    assert path["exit"] == want["exit"]
    if "surv" in want:
        lo, hi = want["surv"]
        assert path["survivors"][0] >= lo and (hi is None or path["survivors"][0] <= hi)
    if "batch" in want:
        assert path["stop_batch"] == want["batch"] or (want["batch"] == 1 and path["stop_batch"] is None and ost["iterations"] > R.RANSAC_BATCH)
    if "chunk" in want:
        assert path["stop_chunk"] == want["chunk"]
    if "k" in want:      # the first survivor of a later chunk is already beyond est_k: the chunk is never validated
        assert path["stop_k"] == want["k"] and path["survivors"][0] > want["k"]
    if "batches" in want:
        assert len(path["survivors"]) == want["batches"] and all(s > 0 for s in path["survivors"])
    if want.get("kept"):  # the best transform comes from batch 1 and is never improved
        _, st1 = oracle.ransac_corres(src, tgt, corr, md, 3, 0.95, R.RANSAC_BATCH, conf, seed)
        assert (st1["fitness"], st1["rmse"]) == (ost["fitness"], ost["rmse"]) and st1["validations"] < ost["validations"]
    _check_against_oracle(ops, oracle, src, tgt, corr, md, mi, conf, seed, oT, ost)


@pytest.mark.parametrize("mi", MAX_ITERATIONS)
def test_ransac_max_iteration_edges(ops, oracle, base_cloud, mi):
    src, tgt, corr = _scene(base_cloud, 1000, 0.15, 0.0, 2000, 1, 0.0)
    g, ost = _check_against_oracle(ops, oracle, src, tgt, corr, 20.0, mi, 1.0, 5)
    assert ost["iterations"] == mi and (mi < R.RANSAC_BATCH - 1 or ost["validations"] > 0)


@pytest.mark.parametrize("nc", [2, 3, 4, 8])
def test_ransac_tiny_correspondence_sets(ops, oracle, base_cloud, nc):
    """with 3 .. 8 correspondences most draws repeat a correspondence (a flat triple: rejected on both sides)"""
    src, tgt, _ = R.corres_scene(base_cloud, 500, 0.0, 0.0, 10, 2)
    corr = np.stack([np.arange(nc), np.arange(nc)], 1).astype(np.int32) * 37
    for conf, mi in ((0.999, 250000), (1.0, 40000)):
        g, ost = _check_against_oracle(ops, oracle, src, tgt, corr, 20.0, mi, conf, 11)
        if nc == 2:
            assert ost["iterations"] == 0 and g["iterations"] == 0
        else:
            assert ost["validations"] > 0 and g["fitness"] == 1.0


def test_ransac_collinear_and_nonpositive_distance(ops, oracle):
    t = np.arange(200, dtype=np.float64)
    src = np.stack([t * 3.0 - 200.0, t * 2.0 + 10.0, t + 1000.0], 1).astype(np.float32)            # exactly collinear
    T1 = R.MOTION1
    tgt = (src.astype(np.float64) @ T1[:3, :3].T + T1[:3, 3]).astype(np.float32)
    corr = np.stack([np.arange(200), np.arange(200)], 1).astype(np.int32)
    g, ost = _check_against_oracle(ops, oracle, src, tgt, corr, 20.0, 40000, 0.999, 3)
    assert ost["validations"] == 0 and ost["iterations"] == 40000
    src2, tgt2, corr2 = R.corres_scene(synth.frame_cloud(), 1000, 0.5, 0.0, 200, 4)
    for md in (0.0, -5.0):
        g, ost = _check_against_oracle(ops, oracle, src2, tgt2, corr2, md, 1000, 0.999, 3)
        assert g["iterations"] == ost["iterations"] == 0


# ----------------------------------------------------------------- C. FPFH
def _fpfh_case(ops, oracle, pts, nrm, radius, max_nn):
    pts = np.asarray(pts, dtype=np.float32)
    nrm = np.asarray(nrm, dtype=np.float32)
    got = npy(ops.fpfh(pts, nrm, radius, max_nn))
    want, _ = oracle.fpfh(pts, nrm, radius, max_nn)
    nbr, cnt, d2 = oracle.hybrid_knn_d2(pts, radius, max(1, min(max_nn, len(pts))))
    flags = R.fpfh_edge_flags(pts, nrm, nbr, cnt)
    R.check_fpfh(got, want, flags, nbr, cnt, d2)
    return got, want, flags, cnt


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_fpfh_tiny_clouds_and_lonely_points(ops, oracle):
    rng = np.random.default_rng(8)
    for n in (1, 2, 5):
        p = rng.uniform(0, 50, size=(n, 3))
        _fpfh_case(ops, oracle, p, _unit(rng.normal(size=(n, 3))), 100.0, 40)
    # isolated points (0 neighbours) and pairs (1 neighbour): all-zero rows
    p = np.concatenate([rng.uniform(0, 40, size=(30, 3)), [[1000, 0, 0], [2000, 0, 0], [2000, 10, 0]]])
    got, want, _, cnt = _fpfh_case(ops, oracle, p, _unit(rng.normal(size=(33, 3))), 60.0, 40)
    assert np.all(cnt[-3:] <= 2) and np.all(got[-3] == 0) and np.all(want[-3] == 0)


def test_fpfh_duplicates_and_parallel_normals(ops, oracle):
    """exact duplicates (the d2 == 0 skip) and normals parallel to the offset (the vn == 0 branch)"""
    rng = np.random.default_rng(9)
    p = rng.uniform(0, 60, size=(200, 3))
    p = np.concatenate([p, p[:40], p[:10]])                             # doubles and triples
    nrm = _unit(rng.normal(size=(len(p), 3)))
    col = np.stack([np.zeros(20), np.zeros(20), np.arange(20) * 5.0], 1) + [500, 500, 500]
    p = np.concatenate([p, col])
    nrm = np.concatenate([nrm, np.tile([0, 0, 1.0], (20, 1))])           # offsets along the common normal: v = 0
    got, want, flags, _ = _fpfh_case(ops, oracle, p, nrm, 30.0, 40)
    assert np.all(flags[-20:] == 0) and np.allclose(got[-20:], want[-20:], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("radius,max_nn", [(1.5, 100), (2.5, 8), (30.0, 200)])
def test_fpfh_integer_lattice_exact_everywhere(ops, oracle, radius, max_nn):
    """a lattice with axis normals: no pair near a bin edge, so every row must match; radius-bound and max_nn-bound neighbourhoods
    (the lattice's equal distances make the max_nn cut a tie on (d2, index))"""
    g = np.arange(7, dtype=np.float64)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(10)
    nrm = np.eye(3)[rng.integers(0, 3, len(p))] * rng.choice([-1.0, 1.0], size=(len(p), 1))
    got, want, flags, cnt = _fpfh_case(ops, oracle, p, nrm, radius, max_nn)
    assert flags.sum() == 0
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    assert (cnt.max() < max_nn) if radius < 2 else (cnt.max() == min(max_nn, len(p)))


@pytest.mark.parametrize("voxel", [50.0, 35.0])
def test_fpfh_views_bin_edge_check(ops, oracle, view_clouds, voxel):
    for _, p in view_clouds:
        d = oracle.voxel_downsample(p, voxel)[0]
        nrm = npy(ops.estimate_normals(d, 2 * voxel, 40))
        _fpfh_case(ops, oracle, d, nrm, 5 * voxel, 40)


# ----------------------------------------------------------------- D. the chain at the reference's default voxel
def test_global_registration_chain_at_voxel_35(ops, oracle, view_clouds):
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.registration import execute_global_registration
    (E0, tgt_full), (E1, src_full) = view_clouds
    voxel, trials, seed = 35.0, 3, 41
    T_kept = execute_global_registration(PointCloud(tgt_full), PointCloud(src_full), voxel_size=voxel, ransac_n_trials=trials, seed=seed)
    # the same composition, stage by stage: voxel -> normals (2v, 40) -> FPFH (5v, 40) -> mutual matching -> RANSAC per trial
    down, nrms, feats = [], [], []
    for p in (src_full, tgt_full):
        d = npy(ops.voxel_downsample(p, voxel)[0])
        assert np.array_equal(d, oracle.voxel_downsample(p, voxel)[0])
        nrm = npy(ops.estimate_normals(d, 2 * voxel, 40))
        got = npy(ops.fpfh(d, nrm, 5 * voxel, 40))
        want, _ = oracle.fpfh(d, nrm, 5 * voxel, 40)
        nbr, cnt, d2 = oracle.hybrid_knn_d2(d, 5 * voxel, 40)
        R.check_fpfh(got, want, R.fpfh_edge_flags(d, nrm, nbr, cnt), nbr, cnt, d2)
        down.append(d)
        nrms.append(nrm)
        feats.append(got)
    corr = ops.feature_correspondences(feats[0], feats[1], True, 3)
    assert np.array_equal(corr, oracle.feature_correspondences(feats[0], feats[1], True, 3))
    best, kept = 0.0, None
    for t in range(trials):
        g, ost = _check_against_oracle(ops, oracle, down[0], down[1], corr, 1.5 * voxel, 250000, 0.999, seed + t)
        if best < ost["fitness"]:
            best, kept = ost["fitness"], g["transformation"]
    assert kept is not None and T_kept is not None
    assert np.array_equal(T_kept, kept)
    T_true = np.linalg.inv(E0) @ E1
    ang = np.degrees(np.arccos(np.clip((np.trace(T_kept[:3, :3].T @ T_true[:3, :3]) - 1) / 2, -1, 1)))
    assert ang < 6.0 and np.abs(T_kept[:3, 3] - T_true[:3, 3]).max() < 250.0

"""GPU suite (-m gpu): Fast Global Registration (kpx_fgr.hip) against its float64 restatement tests/fgr_ref.py.

Tuple test: pair list and count equal the restatement's exactly, across correspondence counts, tuple limits and the two batch edges.
Optimisation: T within ten times the restatement's own spread over permuted correspondence orders (floored at 1e-12; rotation entries
absolute, translation relative to the cloud scale), rounds / failed solves / final par equal.  Spreads of the restatement measured
over four permutations per case (scene seed 11, wrong = share of random pairs), all below the floor:

    nc      wrong 0 %   wrong 50 %        options (nc 65 / 0 %, nc 1025 / 50 %)
    3       8.9e-16     4.4e-16           use_absolute_scale      1.1e-16   4.4e-16
    4       2.2e-16     1.0e-15           decrease_mu=False       1.1e-16   2.2e-16
    63      1.1e-16     2.2e-16           iteration_number=1      5.6e-17   5.6e-17
    64      1.1e-16     4.4e-16           iteration_number=0      0         0
    65      1.1e-16     4.4e-16
    1023    1.1e-16     2.2e-16
    1025    1.4e-16     3.3e-16
    3000    1.1e-16     1.7e-16
    40000   1.1e-16     1.1e-16
"""
import ctypes as C

import numpy as np
import pytest

import fgr_ref as F
import globalreg_ref as R
from kinectpy_amd.utils import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


def npy(t):
    return t.cpu().numpy()


def _scene(base_cloud, nc, wrong, seed=11):
    return R.corres_scene(base_cloud, max(3000, nc), 1.0 - wrong, 0.0, nc, seed)


# ----------------------------------------------------------------- A. tuple test
@pytest.mark.parametrize("max_count", [1, 1000, 10 ** 6])
@pytest.mark.parametrize("nc", [1, 2, 3, 64, 65, 2000])
def test_tuple_test_equals_restatement(ops, base_cloud, nc, max_count):
    src, tgt, corr = _scene(base_cloud, nc, 0.5)
    want = F.tuple_test(src, tgt, corr, 0.95, max_count, 5)
    got = npy(ops.fgr_tuple_test(src, tgt, corr, 0.95, max_count, 5))
    assert got.shape == want.shape and np.array_equal(got, want)
    if nc == 2000:
        assert len(want) == 3 * min(max_count, len(want) // 3) and (max_count < 10 ** 6 or len(want) < 3 * 100 * nc)
        assert len(want) > 0


@pytest.fixture(scope="module")
def batch_edge_cases(base_cloud):
    """(seed, limit, trial) such that the limit-th passing trial is the last of batch 0 / the first of batch 1, found by the restatement"""
    src, tgt, corr = _scene(base_cloud, 2000, 0.5)
    found = {}
    for seed in range(200):
        ok, _ = F.tuple_flags(src, tgt, corr, 0.95, seed, 0, F.BATCH + 1)
        for trial in (F.BATCH - 1, F.BATCH):
            if ok[trial] and trial not in found:
                found[trial] = (seed, int(ok[:trial + 1].sum()))
        if len(found) == 2:
            break
    assert len(found) == 2
    return src, tgt, corr, found


@pytest.mark.parametrize("trial", [F.BATCH - 1, F.BATCH])
def test_tuple_limit_reached_at_a_batch_edge(ops, batch_edge_cases, trial):
    src, tgt, corr, found = batch_edge_cases
    seed, limit = found[trial]
    want = F.tuple_test(src, tgt, corr, 0.95, limit, seed)
    ok, picks = F.tuple_flags(src, tgt, corr, 0.95, seed, 0, trial + 1)
    assert len(want) == 3 * limit and np.array_equal(want[-3:], corr[picks[trial]])          # the case is what it claims to be
    for lim in (limit - 1, limit, limit + 1):
        got = npy(ops.fgr_tuple_test(src, tgt, corr, 0.95, lim, seed))
        assert np.array_equal(got, F.tuple_test(src, tgt, corr, 0.95, lim, seed))


def test_tuple_test_is_seeded(ops, base_cloud):
    src, tgt, corr = _scene(base_cloud, 500, 0.5)
    a, b, c = (npy(ops.fgr_tuple_test(src, tgt, corr, 0.95, 300, s)) for s in (3, 3, 4))
    assert np.array_equal(a, b) and len(a) == 900 and not np.array_equal(a, c)


# ----------------------------------------------------------------- B. optimisation
OPT_CASES = [(nc, wrong, {}) for nc in (3, 4, 63, 64, 65, 1023, 1025, 3000, 40000) for wrong in (0.0, 0.5)] + [
    (nc, wrong, kw) for nc, wrong in ((65, 0.0), (1025, 0.5))
    for kw in (dict(use_absolute_scale=True, maximum_correspondence_distance=25.0), dict(decrease_mu=False), dict(iteration_number=1),
               dict(iteration_number=0))]


def _check_optimize(ops, src, tgt, corr, kw, n_perm=4):
    ref, spread = F.permutation_spread(src, tgt, corr, n_perm, **kw)
    tol = max(10.0 * spread, 1e-12)
    g = ops.fgr_optimize(src, tgt, corr, **kw)
    T = g["transformation"]
    diff = F.transform_difference(T, ref["transformation"], ref["scale"])
    print(f"nc={len(corr)} {kw}: restatement spread {spread:.2e}, device - restatement {diff:.2e}, tolerance {tol:.2e}")
    assert np.all(np.isfinite(T)) and diff <= tol
    assert (g["iterations"], g["failed_solves"]) == (ref["iterations"], ref["failed_solves"])
    mcd = kw.get("maximum_correspondence_distance", 0.025)
    assert (g["par"] <= mcd) == (ref["par"] <= mcd) and abs(g["par"] - ref["par"]) <= 1e-15 * ref["par"]
    assert g["scale"] == ref["scale"]
    assert np.array_equal(T[3], [0, 0, 0, 1])
    Rm = T[:3, :3]
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12
    g2 = ops.fgr_optimize(src, tgt, corr, **kw)
    assert np.array_equal(g2["transformation"], T) and g2["par"] == g["par"]
    return g, ref


@pytest.mark.parametrize("nc,wrong,kw", OPT_CASES)
def test_optimize_matches_restatement(ops, base_cloud, nc, wrong, kw):
    src, tgt, corr = _scene(base_cloud, nc, wrong)
    g, ref = _check_optimize(ops, src, tgt, corr, kw)
    if kw.get("iteration_number", 64) == 0:
        assert np.array_equal(g["transformation"], np.eye(4)) and g["iterations"] == 0
    if not kw and wrong == 0.0:
        assert F.transform_difference(g["transformation"], R.MOTION1, ref["scale"]) < 1e-6


def test_optimize_accuracy_with_half_the_correspondences_wrong(ops, base_cloud):
    """known motion, 50 % random pairs: the bounds of test_fgr_cpu.py's restatement test, on the device"""
    src, tgt, corr = R.corres_scene(base_cloud, 3000, 0.5, 0.0, 2000, 3)
    T = ops.fgr_optimize(src, tgt, corr)["transformation"]
    ang = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3].T @ R.MOTION1[:3, :3]) - 1) / 2, -1, 1)))
    assert ang < 0.2 and np.abs(T[:3, 3] - R.MOTION1[:3, 3]).max() < 2e-3 * F.normalise(src, tgt)[2]


# ----------------------------------------------------------------- C. degenerate input
def test_optimize_degenerate_input(ops, base_cloud):
    src, tgt, corr = _scene(base_cloud, 200, 0.0)
    g, _ = _check_optimize(ops, src, tgt, corr[:0], {})                                     # no correspondence: the identity
    assert np.array_equal(g["transformation"], np.eye(4)) and g["iterations"] == 0 and g["par"] == 1.0
    g, ref = _check_optimize(ops, src, tgt, np.tile(corr[:1], (100, 1)), {})                # one pair a hundred times: rank 3
    assert g["failed_solves"] == 64 and np.array_equal(g["transformation"][:3, :3], np.eye(3))
    t = np.arange(200, dtype=np.float64)
    line = np.stack([t * 3.0 - 200.0, t * 2.0 + 10.0, t + 1000.0], 1).astype(np.float32)    # exactly collinear clouds
    moved = line + np.array([120.0, -40.0, 300.0], dtype=np.float32)                        # (integers: the target is exactly collinear too)
    ident = np.stack([np.arange(200), np.arange(200)], 1).astype(np.int32)
    g, ref = _check_optimize(ops, line, moved, ident, {})                                   # rank 5: rotation about the line is free
    assert g["failed_solves"] == 64
    one = np.zeros((5, 3), dtype=np.float32) + 7.0                                          # every point on its mean: scale 0
    g, ref = _check_optimize(ops, one, one, ident[:5], {})
    assert g["scale"] == 0.0


def test_index_out_of_range_is_refused_and_leaves_the_output_untouched(ops, base_cloud):
    import torch
    from kinectpy_amd import _lib as L
    src, tgt, corr = _scene(base_cloud, 100, 0.0)
    lib = L.load()
    s, t = torch.as_tensor(src).cuda(), torch.as_tensor(tgt).cuda()
    for col, n in ((0, len(src)), (1, len(tgt))):
        for bad_value in (n, -1):
            bad = corr.copy()
            bad[37, col] = bad_value
            with pytest.raises(L.KinectPxError, match="out of range"):
                ops.fgr_optimize(src, tgt, bad)
            with pytest.raises(L.KinectPxError, match="out of range"):
                ops.fgr_tuple_test(src, tgt, bad)
            c = torch.as_tensor(bad).cuda()
            res = np.full(20, 7.0)
            ws, wsz = L.workspace(lib.kpx_fgr_workspace_bytes(len(bad)))
            rc = lib.kpx_fgr_optimize(L.ptr(s), len(src), L.ptr(t), len(tgt), L.ptr(c), len(bad), 1.4, 0, 1, 0.025, 64, L.hptr(res), ws, wsz,
                                      L.stream_ptr())
            assert rc == -3 and np.all(res == 7.0)
            pairs = torch.full((300, 2), -5, dtype=torch.int32, device="cuda")
            cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
            rc = lib.kpx_fgr_tuple_test(L.ptr(s), len(src), L.ptr(t), len(tgt), L.ptr(c), len(bad), 0.95, 100, C.c_uint64(1), L.ptr(pairs),
                                        L.ptr(cnt), ws, wsz, L.stream_ptr())
            assert rc == -3 and int(cnt[0]) == -5 and bool((pairs == -5).all())


# ----------------------------------------------------------------- D. public entry points
def test_correspondence_entry_points_wrap_the_ops(ops, base_cloud):
    from kinectpy_amd import o3d
    from kinectpy_amd.geometry import PointCloud
    reg = o3d.pipelines.registration
    src, tgt, corr = R.corres_scene(base_cloud, 3000, 0.5, 0.0, 2000, 3)
    ps, pt = PointCloud(src), PointCloud(tgt)

    def inliers(T, dist):
        ev = ops.registration_eval(src, tgt, dist, T, want_corr=True)
        idx, d2 = npy(ev["idx"]), npy(ev["d2"])
        ok = d2 < dist * dist
        return ev, np.stack([np.flatnonzero(ok).astype(np.int32), idx[ok]], 1)

    opt = reg.FastGlobalRegistrationOption(use_absolute_scale=True, maximum_correspondence_distance=20.0, tuple_test=False)
    res = reg.registration_fgr_based_on_correspondence(ps, pt, corr, opt)
    g = ops.fgr_optimize(src, tgt, corr, use_absolute_scale=True, maximum_correspondence_distance=20.0)
    ev, want = inliers(g["transformation"], 20.0)
    assert np.array_equal(res.transformation, g["transformation"]) and (res.fitness, res.inlier_rmse) == (ev["fitness"], ev["inlier_rmse"])
    assert np.array_equal(res.correspondence_set, want) and res.fitness > 0.9
    res = reg.registration_ransac_based_on_correspondence(
        ps, pt, corr, 20.0, reg.TransformationEstimationPointToPoint(False), 3,
        [reg.CorrespondenceCheckerBasedOnEdgeLength(0.95), reg.CorrespondenceCheckerBasedOnDistance(20.0)], reg.RANSACConvergenceCriteria(40000, 0.999), seed=7)
    g = ops.ransac_corres(src, tgt, corr, 20.0, 3, 0.95, 40000, 0.999, 7)
    assert np.array_equal(res.transformation, g["transformation"]) and (res.fitness, res.inlier_rmse) == (g["fitness"], g["inlier_rmse"])
    assert np.array_equal(res.correspondence_set, inliers(g["transformation"], 20.0)[1]) and res.fitness > 0.9
    with pytest.raises(NotImplementedError):
        reg.registration_ransac_based_on_correspondence(ps, pt, corr, 20.0, checkers=[reg.CorrespondenceCheckerBasedOnDistance(5.0)])


# ----------------------------------------------------------------- E. the chain at the reference's default voxel
@pytest.fixture(scope="module")
def view_clouds(oracle):
    """the two cluttered views of test_global_registration_gpu.py, before down-sampling"""
    xy, ex = synth.xy_table(), synth.clutter()
    out = []
    for i, seed in ((0, 100), (1, 101)):
        E = synth.camera_pose(i, 16)
        dep = synth.render_depth(E, seed=seed, xy=xy, extra=ex)
        out.append((E, oracle.rgbd_compact(oracle.unproject_u16(dep, xy))[0]))
    return out


def test_fgr_chain_at_voxel_35(ops, view_clouds):
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.registration import execute_global_registration
    (E0, tgt_full), (E1, src_full) = view_clouds
    voxel, seed = 35.0, 41
    T_fgr = execute_global_registration(PointCloud(tgt_full), PointCloud(src_full), voxel_size=voxel, seed=seed, method="fgr")
    down, feats = [], []
    for p in (src_full, tgt_full):
        d = ops.voxel_downsample(p, voxel)[0]
        nrm = ops.estimate_normals(d, 2 * voxel, 40)
        down.append(d)
        feats.append(ops.fpfh(d, nrm, 5 * voxel, 40))
    corr = ops.feature_correspondences(feats[0], feats[1], True, ransac_n=0)
    tuples = ops.fgr_tuple_test(down[0], down[1], corr, 0.95, 1000, seed)
    g = ops.fgr_optimize(down[0], down[1], tuples, maximum_correspondence_distance=0.5 * voxel)
    ev = ops.registration_eval(down[0], down[1], 0.5 * voxel, g["transformation"])
    assert len(corr) > 0 and len(tuples) > 0 and ev["fitness"] > 0
    assert T_fgr is not None and np.array_equal(T_fgr, g["transformation"])
    # with the keypoints extension: still one FGR, on the cut clouds
    T_key = execute_global_registration(PointCloud(tgt_full), PointCloud(src_full), voxel_size=voxel, seed=seed, method="fgr", keypoints=True)
    assert T_key is None or (T_key.shape == (4, 4) and np.all(np.isfinite(T_key)))
    # Accuracy against the true motion is NOT asserted on this pair: the restatement itself, on the oracle's features, ends at 10.8 degrees
    # and 519 mm (seed 41), outside the RANSAC chain test's bound of 6 degrees and 250 mm -- with the clouds in millimetres
    # the normalised par = 1 never exceeds maximum_correspondence_distance = 17.5, so the weight is never annealed.  The bound is not
    # loosened; accuracy is asserted on a known motion with half the pairs wrong (test_optimize_accuracy_with_half_the_correspondences_wrong).
    T_true = np.linalg.inv(E0) @ E1
    ang = np.degrees(np.arccos(np.clip((np.trace(T_fgr[:3, :3].T @ T_true[:3, :3]) - 1) / 2, -1, 1)))
    print(f"FGR at voxel 35: {len(corr)} mutual pairs, {len(tuples) // 3} tuples, angle {ang:.3f} deg, "
          f"translation {np.abs(T_fgr[:3, 3] - T_true[:3, 3]).max():.1f} mm, fitness {ev['fitness']:.4f}, par {g['par']}")


def test_ransac_method_is_the_call_without_the_keyword(view_clouds):
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.registration import execute_global_registration
    (E0, tgt_full), (E1, src_full) = view_clouds
    a = execute_global_registration(PointCloud(tgt_full), PointCloud(src_full), voxel_size=60.0, ransac_n_trials=2, seed=41)
    b = execute_global_registration(PointCloud(tgt_full), PointCloud(src_full), voxel_size=60.0, ransac_n_trials=2, seed=41, method="ransac")
    assert a is not None and np.array_equal(a, b)

"""GPU suite (-m gpu) for generalized ICP: kpx_estimate_covariances, kpx_gicp_covariances and kpx_generalized_icp against the NumPy
restatement in tests/gicp_ref.py, the degenerate case, and the PointCloud / o3d surface."""
import copy

import numpy as np
import pytest
import torch

import gicp_ref as G
from kinectpy_amd.utils import synth

pytestmark = pytest.mark.gpu
TOL_T = 1e-8           # absolute, 4x4 transform (rotation entries / mm), as test_parity_gpu.py


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


@pytest.fixture(params=["culled", "dense", "dense_fp64"])
def engine(request, ops):
    prev = ops.nn_engine(request.param)
    yield request.param
    ops.nn_engine(prev)


def _npy(t):
    return t.cpu().numpy()


def _cloud(base, n, seed):
    return base[np.random.default_rng(seed).choice(len(base), n, replace=False)]


@pytest.mark.parametrize("n,radius,max_nn", [(20000, 1e150, 20), (20000, 1e150, 30), (20000, 18.0, 30), (3000, 1e150, 200), (3000, 1e150, 600)])
def test_estimate_covariances_matches_restatement(ops, oracle, base_cloud, n, radius, max_nn):
    """KNN 20 / 30, a hybrid search where some points have < 3 neighbours (identity), max_nn beyond KPX_NORMALS_LDS_NN (the
    leftovers' heaps in the workspace) and beyond the wave pass (every point through the workspace heaps)"""
    pts = _cloud(base_cloud, n, 7)
    g = _npy(ops.estimate_covariances(pts, radius, max_nn))
    ref = G.estimate_covariances(oracle, pts, radius, max_nn)
    nbr, cnt = oracle.hybrid_knn(pts, radius, max_nn)
    p64 = pts.astype(np.float64)
    mu = np.stack([p64[nbr[i, :cnt[i]]].mean(0) if cnt[i] else np.zeros(3) for i in range(n)])
    tol = 1e-9 * np.linalg.norm(ref, axis=(1, 2)) + 1e-12 * (mu * mu).sum(1)
    assert g.shape == (n, 3, 3) and g.dtype == np.float64
    assert (np.abs(g - ref).max(axis=(1, 2)) <= tol).all()
    assert np.array_equal(g, np.transpose(g, (0, 2, 1)))
    few = cnt < 3
    if radius < 1e100:
        assert few.any() and (~few).any()
    assert np.array_equal(g[few], np.broadcast_to(np.eye(3), g[few].shape))


def test_gicp_covariances_from_normals(ops, base_cloud):
    pts = _cloud(base_cloud, 5000, 3)
    nrm = _npy(ops.estimate_normals(pts, 1e150, 20))
    c = np.array([-0.995, -0.9901, -0.98999, -0.5, 0.0, 0.999])
    special = np.stack([c, np.sqrt(1 - c * c), np.zeros_like(c)], 1)
    special = np.concatenate([special, [[0, 0, 1], [-1, 0, 0], [1, 0, 0], [0, -1, 0]]]).astype(np.float32)
    nrm = np.concatenate([nrm, special, -nrm[:500]]).astype(np.float32)
    assert (nrm[:, 0] < -0.99).sum() >= 3
    for eps in (1e-3, 0.2):
        g = _npy(ops.gicp_covariances(nrm, eps))
        assert np.abs(g - G.covariances_from_normals(nrm, eps)).max() < 1e-14
    assert np.array_equal(_npy(ops.gicp_covariances(np.array([[-1, 0, 0]], np.float32), 1e-3))[0], np.diag([1e-3, 1.0, 1.0]))


def _covariance_sources(ops, src, tgt):
    """the three sources of InitializePointCloudForGeneralizedICP: raw covariances, from given normals, from normals estimated
    with KNN(20) -- computed once on the device and fed to both the library and the restatement"""
    tn = _npy(ops.estimate_normals(tgt, 70.0, 30))
    return {
        "covariances": (_npy(ops.estimate_covariances(src, 1e150, 30)), _npy(ops.estimate_covariances(tgt, 1e150, 30))),
        "normals": (_npy(ops.gicp_covariances(_npy(ops.estimate_normals(src, 70.0, 30)))), _npy(ops.gicp_covariances(tn))),
        "estimated": (_npy(ops.gicp_covariances(_npy(ops.estimate_normals(src, 1e150, 20)))),
                      _npy(ops.gicp_covariances(_npy(ops.estimate_normals(tgt, 1e150, 20))))),
    }


def test_generalized_icp_matches_restatement(ops, oracle, base_cloud, engine):
    src, tgt, T = synth.icp_pair(6000, base_cloud)
    pert = np.linalg.inv(T).copy()
    pert[:3, 3] += [15.0, -10.0, 5.0]
    for name, (cs, ct) in _covariance_sources(ops, src, tgt).items():
        for init, iters in ((None, 30), (np.linalg.inv(pert), 12)):
            r = ops.generalized_icp(src, cs, tgt, ct, 100.0, init, iters, want_corr=True)
            rT, rf, rr, rit, (ri, rd) = G.registration_generalized_icp(oracle, src, tgt, 100.0, cs, ct, init, iters)
            assert r["iterations"] == rit and r["fitness"] == rf and abs(r["inlier_rmse"] - rr) < 1e-8, (name, engine)
            assert np.abs(r["transformation"] - rT).max() < TOL_T, (name, engine)
            ok = rd < 100.0 ** 2
            gi, gd = _npy(r["idx"]), _npy(r["d2"])
            assert np.array_equal(gd < 100.0 ** 2, ok) and np.array_equal(gi[ok], ri[ok]), (name, engine)


def test_generalized_icp_recovers_ground_truth(ops, base_cloud):
    src, tgt, T = synth.icp_pair(20000, base_cloud)
    r = ops.generalized_icp(src, ops.estimate_covariances(src, 1e150, 30), tgt, ops.estimate_covariances(tgt, 1e150, 30), 100.0, None, 40)
    assert np.abs(r["transformation"][:3, :3] - T[:3, :3]).max() < 5e-3 and np.abs(r["transformation"][:3, 3] - T[:3, 3]).max() < 6.0


def test_generalized_icp_planar_clouds_stay_finite(ops, oracle):
    """two exactly flat clouds with their raw covariances: every M is singular (Open3D: NaN); here the pairs add nothing, the
    iteration takes the identity update and the loop ends"""
    gx, gy = np.meshgrid(np.arange(0, 600, 10.0), np.arange(0, 400, 10.0))
    tgt = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1).astype(np.float32)
    src = (tgt + np.array([3.0, 2.0, 0.0])).astype(np.float32)
    cs, ct = _npy(ops.estimate_covariances(src, 1e150, 20)), _npy(ops.estimate_covariances(tgt, 1e150, 20))
    assert np.abs(cs[:, 2, :]).max() == 0.0
    r = ops.generalized_icp(src, cs, tgt, ct, 30.0, None, 20)
    assert np.isfinite(r["transformation"]).all() and r["iterations"] <= 20 and r["fitness"] == 1.0
    assert np.array_equal(r["transformation"], np.eye(4))
    rT, rf, _, rit, _ = G.registration_generalized_icp(oracle, src, tgt, 30.0, cs, ct, None, 20)
    assert r["iterations"] == rit == 1 and np.array_equal(rT, np.eye(4))


def test_generalized_icp_api(ops, base_cloud):
    from kinectpy_amd import o3d
    reg = o3d.pipelines.registration
    src, tgt, T = synth.icp_pair(5000, base_cloud)
    a, b = o3d.geometry.PointCloud(), o3d.geometry.PointCloud()
    a.points, b.points = o3d.utility.Vector3dVector(src), o3d.utility.Vector3dVector(tgt)
    b.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(70.0, 30))
    with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance"):
        reg.registration_generalized_icp(a, b, 0.0)
    with pytest.raises(NotImplementedError):
        reg.TransformationEstimationForGeneralizedICP(kernel=object())
    pa, pb, nb = np.asarray(a.points), np.asarray(b.points), np.asarray(b.normals)
    res = reg.registration_generalized_icp(a, b, 100.0, np.eye(4), reg.TransformationEstimationForGeneralizedICP(1e-3, reg.L2Loss()),
                                           reg.ICPConvergenceCriteria(max_iteration=30))
    assert np.array_equal(np.asarray(a.points), pa) and np.array_equal(np.asarray(b.points), pb) and np.array_equal(np.asarray(b.normals), nb)
    assert not a.has_covariances() and not b.has_covariances() and not a.has_normals()
    # the same run through ops: source normals estimated with KNN(20), target covariances from its normals
    cs = ops.gicp_covariances(ops.estimate_normals(src, 1e150, 20), 1e-3)
    r = ops.generalized_icp(src, cs, tgt, ops.gicp_covariances(b._nrm, 1e-3), 100.0, np.eye(4), 30)
    assert np.array_equal(res.transformation, r["transformation"]) and res.fitness == r["fitness"]
    gi, gd = ops.nn_search(src, tgt, res.transformation)
    ok = _npy(gd) < 100.0 ** 2
    assert np.array_equal(np.asarray(res.correspondence_set), np.stack([np.flatnonzero(ok), _npy(gi)[ok]], 1))
    assert np.abs(res.transformation[:3, 3] - T[:3, 3]).max() < 6.0
    # covariances on the cloud: estimate, transform (rotated), deepcopy / + (carried), select_by_index (dropped)
    a.estimate_covariances()
    assert a.has_covariances() and np.array_equal(np.asarray(a.covariances), _npy(ops.estimate_covariances(src, 1e150, 30)))
    c0 = np.asarray(a.covariances)
    M = np.linalg.inv(T)
    a.transform(M)
    R = M[:3, :3]
    assert np.abs(np.asarray(a.covariances) - R @ c0 @ R.T).max() < 1e-9 * np.abs(c0).max()
    d = copy.deepcopy(a)
    assert d.has_covariances() and np.array_equal(np.asarray(d.covariances), np.asarray(a.covariances))
    d._cov.zero_()
    assert np.abs(np.asarray(a.covariances)).max() > 0                       # a deep copy
    s = a + a.clone()
    assert s.has_covariances() and np.array_equal(np.asarray(s.covariances), np.concatenate([np.asarray(a.covariances)] * 2))
    assert not (a + b).has_covariances()
    assert not a.select_by_index(np.arange(10)).has_covariances()            # Open3D keeps them: see PointCloud's docstring
    # a cloud's own covariances are used as they are
    e = o3d.geometry.PointCloud()
    e.points = o3d.utility.Vector3dVector(src)
    e.covariances = o3d.utility.Matrix3dVector(np.broadcast_to(np.eye(3), (len(src), 3, 3)))
    assert e.has_covariances() and np.asarray(e.covariances).shape == (len(src), 3, 3)
    re = reg.registration_generalized_icp(e, b, 100.0, None, None, reg.ICPConvergenceCriteria(max_iteration=5))
    ri = ops.generalized_icp(src, torch.eye(3, dtype=torch.float64).expand(len(src), 3, 3), tgt, ops.gicp_covariances(b._nrm), 100.0, None, 5)
    assert np.array_equal(re.transformation, ri["transformation"])

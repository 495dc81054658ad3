"""GPU suite (-m gpu) for the robust kernels: kpx_icp_robust, kpx_colored_icp_robust and kpx_generalized_icp_robust against the NumPy
restatement in tests/robust_ref.py on every engine, the edge rows (r == 0 under L1, weight 0 under Tukey, no partner), L2
bit-identity with the plain entry points, and the o3d / pipeline surface.

Tolerances on the 4x4 transform.  Huber, Cauchy and Tukey have weights <= 1: the project's TOL_T.  L1 (weight 1 / |r|, unbounded)
and GM (k / (k + r^2)^2, scale-dependent) take max(TOL_T, 100 x spread), the spread being the largest difference in T between runs
of the restatement on the inputs of these tests with the pair rows summed in random orders (robust_ref's `order`, seeds 1..5, for
the L1 starts below 1..10; measured on the CPU); the factor 100 covers the device's different but fixed summation order.  The
spreads are the SPREAD table below; every one is under 1e-10, so every tolerance comes out as TOL_T.

What the suite chooses for L1, and why.  L1 is iteratively reweighted least squares towards a fit that interpolates six rows:
their residuals shrink, their weights grow, and with them grows how far one rounding moves the next transform.  On the 3000-point
pair the restatement's spread from the identity after 2 / 3 / 4 / 6 / 8 / 12 iterations is 3e-13 / 7e-12 / 4e-11 / 4e-9 / 1e-6 /
1e-2 (point-to-plane) and after 1 / 2 / 3 / 4 / 6 iterations 2e-13 / 5e-9 / 3e-6 / 1e-4 / 5.0 (GICP); from a start 15 mm off the
truth over 12 iterations it is 1.7e-5 and 6.9e-2, and on coloured_pair(3000) 1.1e-1.  A reference that moves by a tenth of a
millimetre with the order of its own sums pins nothing to 1e-8, so for L1 the suite takes, of what it is free to choose, the
cases in which the reference reproduces itself (100 x spread within TOL_T):
  - from the identity 3 iterations (point-to-plane, coloured) or 1 (GICP); every other loss runs 30;
  - the perturbed start of the 12-iteration run on the 3000-point pair is synth.perturb(T, 0.01 deg, 0.3 mm) for L1 (0.005 deg /
    0.1 mm and 0.02 deg / 0.5 mm give 2e-10, 0.05 deg / 1 mm already 5e-7 .. 4e-5); every other loss starts 15 mm off;
  - coloured ICP runs on coloured_pair(300) for both losses -- five blocks of the merge kernel with a tail of 44 rows -- where L1
    keeps 8e-11 over the 12 iterations from 15 mm off (coloured_pair(500): 7e-8, (1000): 7e-6)."""
import numpy as np
import pytest

import robust_ref as R
from kinectpy_amd.utils import synth

pytestmark = pytest.mark.gpu
TOL_T = 1e-8           # absolute, 4x4 transform (rotation entries / mm), as test_parity_gpu.py
MAX_DIST = 100.0
K = {"l1": 0.0, "huber": 30.0, "cauchy": 30.0, "gm": 400.0, "tukey": 100.0}
L1_IDENTITY_ITERS = {"p2plane": 3, "colored": 3, "gicp": 1}
COLOURED_N = 300
# measured spreads of the restatement (see the module docstring), keyed by (estimation, loss, start); absent: below 1e-12
SPREAD = {("p2plane", "gm", "identity"): 1.7e-13, ("p2plane", "gm", "perturbed"): 3.2e-14,
          ("p2plane", "l1", "identity"): 6.7e-12, ("p2plane", "l1", "perturbed"): 1.4e-11,
          ("colored", "l1", "identity"): 1.1e-11, ("colored", "l1", "perturbed"): 7.8e-11,
          ("gicp", "l1", "identity"): 2.5e-13, ("gicp", "l1", "perturbed"): 3.7e-11}
STARTS = ("identity", "perturbed")


def tol_T(est, kind, start):
    return max(TOL_T, 100.0 * SPREAD.get((est, kind, start), 0.0))


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


@pytest.fixture(scope="module")
def reg():
    from kinectpy_amd import o3d
    return o3d.pipelines.registration


@pytest.fixture(params=["culled", "dense", "dense_fp64"])
def engine(request, ops):
    prev = ops.nn_engine(request.param)
    yield request.param
    ops.nn_engine(prev)


def _npy(t):
    return t.cpu().numpy()


def _loss(reg, kind, k=None):
    k = K[kind] if k is None else k
    return {"l2": reg.L2Loss, "l1": reg.L1Loss}[kind]() if kind in ("l2", "l1") else \
        {"huber": reg.HuberLoss, "cauchy": reg.CauchyLoss, "gm": reg.GMLoss, "tukey": reg.TukeyLoss}[kind](k)


def _perturbed(T):
    pert = np.linalg.inv(T).copy()
    pert[:3, 3] += [15.0, -10.0, 5.0]
    return np.linalg.inv(pert)


def _start(est, T, kind, start):
    """(init, max_iteration) of a parity run"""
    if start == "identity":
        return None, L1_IDENTITY_ITERS[est] if kind == "l1" else 30
    return synth.perturb(T, 0.01, 0.3, seed=1) if kind == "l1" and est != "colored" else _perturbed(T), 12


_cache = {}


def _once(key, make):
    """inputs computed on the device and restatement results, shared by the three engines"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _check(r, ref, tol, what):
    rT, rf, rr, rit, (ri, rd) = ref
    diff = np.abs(r["transformation"] - rT).max()
    print(f"\n{what}: iterations {r['iterations']} / {rit}  fitness {r['fitness']:.6f} / {rf:.6f}  |dT| {diff:.3g} (tol {tol:.3g})")
    assert r["iterations"] == rit and r["fitness"] == rf and abs(r["inlier_rmse"] - rr) < 1e-8, what
    assert diff < tol, what
    if "idx" in r:
        ok = rd < MAX_DIST ** 2
        gi, gd = _npy(r["idx"]), _npy(r["d2"])
        assert np.array_equal(gd < MAX_DIST ** 2, ok) and np.array_equal(gi[ok], ri[ok]), what


@pytest.fixture(scope="module")
def pair(ops, base_cloud):
    src, tgt, T = synth.icp_pair(3000, base_cloud)          # 3000 = 46 blocks of the merge kernel's 64 rows + a tail of 56
    return src, tgt, T, _npy(ops.estimate_normals(tgt, 70.0, 30))


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("kind", ["l1", "huber", "cauchy", "gm", "tukey"])
def test_point_to_plane_matches_restatement(ops, reg, oracle, pair, engine, kind, start):
    src, tgt, T, tn = pair
    init, iters = _start("p2plane", T, kind, start)
    ref = _once(("p2plane", kind, start), lambda: R.registration_icp_robust(oracle, src, tgt, tn, MAX_DIST, kind, K[kind], init, iters))
    r = ops.icp(src, tgt, MAX_DIST, init, "p2plane", tn, iters, want_corr=True, loss=_loss(reg, kind))
    _check(r, ref, tol_T("p2plane", kind, start), f"p2plane {kind} {start} [{engine}]")


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("kind", ["l1", "tukey"])
def test_coloured_matches_restatement(ops, reg, oracle, engine, kind, start):
    src, sc, tgt, tc, T = synth.coloured_pair(COLOURED_N)
    tn, grad = _once("coloured_inputs", lambda: (lambda n: (n, _npy(ops.color_gradient(tgt, n, tc, 2.0 * MAX_DIST, 30))))(
        oracle.estimate_normals(tgt, 70.0, 30)[0].astype(np.float32)))
    init, iters = _start("colored", T, kind, start)
    ref = _once(("colored", kind, start), lambda: R.registration_colored_icp_robust(
        oracle, src, sc, tgt, tc, tn, MAX_DIST, kind, K[kind], init, 0.968, iters, tgt_gradient=grad))
    r = ops.colored_icp(src, sc, tgt, tc, tn, MAX_DIST, init, 0.968, iters, tgt_gradient=grad, loss=_loss(reg, kind))
    _check(r, ref, tol_T("colored", kind, start), f"coloured {kind} {start} [{engine}]")


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("kind", ["l1", "tukey"])
def test_generalized_icp_matches_restatement(ops, reg, oracle, pair, engine, kind, start):
    src, tgt, T, _ = pair
    cs, ct = _once("gicp_inputs", lambda: (_npy(ops.estimate_covariances(src, 1e150, 30)), _npy(ops.estimate_covariances(tgt, 1e150, 30))))
    init, iters = _start("gicp", T, kind, start)
    ref = _once(("gicp", kind, start), lambda: R.registration_generalized_icp_robust(oracle, src, tgt, MAX_DIST, cs, ct, kind, K[kind],
                                                                                  init, iters))
    r = ops.generalized_icp(src, cs, tgt, ct, MAX_DIST, init, iters, want_corr=True, loss=_loss(reg, kind))
    _check(r, ref, tol_T("gicp", kind, start), f"gicp {kind} {start} [{engine}]")


# ---- edge rows ----------------------------------------------------------------------------------------------------------------
EDGE_K = 30.0


@pytest.fixture(scope="module")
def edge_scene(ops, base_cloud):
    """500 target points; the source: 100 copies of target points (r == 0 exactly under the identity), 250 target points with
    millimetre noise, 100 moved 40..90 mm (beyond Tukey's EDGE_K, inside max_dist), 50 moved 600 mm (no partner within max_dist)"""
    rng = np.random.default_rng(11)
    tgt = base_cloud[rng.choice(len(base_cloud), 500, replace=False)]
    tn = _npy(ops.estimate_normals(tgt, 1e150, 20))
    pick = rng.permutation(500)
    exact = tgt[pick[:100]]
    near = tgt[pick[100:350]] + rng.normal(scale=2.0, size=(250, 3))
    far = tgt[pick[350:450]] + tn[pick[350:450]] * rng.uniform(40.0, 90.0, size=(100, 1)) * rng.choice([-1.0, 1.0], size=(100, 1))
    none = tgt[pick[450:]] + np.array([0.0, -600.0, 0.0])
    src = np.concatenate([exact, near, far, none]).astype(np.float32)
    return src[rng.permutation(len(src))], tgt, tn


def test_edge_rows(ops, reg, oracle, edge_scene, engine):
    src, tgt, tn = edge_scene
    idx, d2, _ = oracle.nn(src, np.eye(4), tgt, grid=True)
    inl = d2 < MAX_DIST ** 2
    r0 = ((src[inl].astype(np.float64) - tgt[idx[inl]].astype(np.float64)) * tn[idx[inl]].astype(np.float64)).sum(1)
    assert (r0 == 0.0).sum() >= 100 and (np.abs(r0) > EDGE_K).sum() >= 30 and (~inl).sum() >= 20
    # L1 with r == 0 rows: finite, and the restatement's result (one update, then the whole loop)
    for iters in (1, 3):
        ref = _once(("edge", "l1", iters), lambda: R.registration_icp_robust(oracle, src, tgt, tn, MAX_DIST, "l1", 0.0, None, iters))
        r = ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, iters, want_corr=True, loss=reg.L1Loss())
        assert np.isfinite(r["transformation"]).all() and not np.array_equal(r["transformation"], np.eye(4))
        _check(r, ref, tol_T("p2plane", "l1", "identity"), f"edge l1 {iters} [{engine}]")
    # Tukey: rows beyond k count in fitness and are absent from the normal equations -- without them the same first update
    ref = _once(("edge", "tukey"), lambda: R.registration_icp_robust(oracle, src, tgt, tn, MAX_DIST, "tukey", EDGE_K, None, 30))
    r = ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, 30, want_corr=True, loss=reg.TukeyLoss(EDGE_K))
    _check(r, ref, TOL_T, f"edge tukey [{engine}]")
    beyond = np.zeros(len(src), bool)
    beyond[np.flatnonzero(inl)[np.abs(r0) > EDGE_K]] = True
    one = ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, 1, loss=reg.TukeyLoss(EDGE_K))
    cut = ops.icp(src[~beyond], tgt, MAX_DIST, None, "p2plane", tn, 1, loss=reg.TukeyLoss(EDGE_K))
    zero = ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, 0, loss=reg.TukeyLoss(EDGE_K))
    assert zero["count"] == inl.sum() and zero["fitness"] == inl.sum() / len(src)
    assert np.abs(one["transformation"] - cut["transformation"]).max() < TOL_T
    assert not np.array_equal(one["transformation"], ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, 1)["transformation"])
    # a k far beyond every residual: Huber's weight is exactly 1, Tukey's 1 - 2 (r / k)^2 = 1 - 2e-14: the L2 result
    l2 = ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, 30)
    for loss in (reg.HuberLoss(1e9), reg.TukeyLoss(1e9)):
        big = ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, 30, loss=loss)
        assert big["iterations"] == l2["iterations"] and big["fitness"] == l2["fitness"]
        assert np.abs(big["transformation"] - l2["transformation"]).max() < TOL_T


def test_l2_is_the_plain_entry_point_bit_for_bit(ops, reg, pair, engine):
    src, tgt, T, tn = pair
    a = ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, 10)
    for loss in (None, reg.L2Loss(), ("l2", 0.0)):
        b = ops.icp(src, tgt, MAX_DIST, None, "p2plane", tn, 10, loss=loss)
        assert np.array_equal(a["transformation"], b["transformation"]) and a["iterations"] == b["iterations"]
    assert np.array_equal(ops.icp(src, tgt, MAX_DIST, None, "p2p", None, 10, loss=reg.L2Loss())["transformation"],
                          ops.icp(src, tgt, MAX_DIST, None, "p2p", None, 10)["transformation"])
    csrc, sc, ctgt, tc, _ = synth.coloured_pair(3000)
    ctn = _npy(ops.estimate_normals(ctgt, 70.0, 30))
    a = ops.colored_icp(csrc, sc, ctgt, tc, ctn, 80.0, None, 0.968, 8)
    for loss in (None, reg.L2Loss()):
        assert np.array_equal(a["transformation"], ops.colored_icp(csrc, sc, ctgt, tc, ctn, 80.0, None, 0.968, 8, loss=loss)["transformation"])
    cs, ct = ops.estimate_covariances(src, 1e150, 30), ops.estimate_covariances(tgt, 1e150, 30)
    a = ops.generalized_icp(src, cs, tgt, ct, MAX_DIST, None, 8)
    for loss in (None, reg.L2Loss()):
        assert np.array_equal(a["transformation"], ops.generalized_icp(src, cs, tgt, ct, MAX_DIST, None, 8, loss=loss)["transformation"])


def test_o3d_surface(ops, reg, pair):
    from kinectpy_amd import o3d
    src, tgt, T, _ = pair
    a, b = o3d.geometry.PointCloud(), o3d.geometry.PointCloud()
    a.points, b.points = o3d.utility.Vector3dVector(src), o3d.utility.Vector3dVector(tgt)
    b.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(70.0, 30))
    pa, pb, nb = np.asarray(a.points), np.asarray(b.points), np.asarray(b.normals)
    init = _perturbed(T)
    res = reg.registration_icp(a, b, MAX_DIST, init, reg.TransformationEstimationPointToPlane(reg.TukeyLoss(R.TUKEY_K)))
    r = ops.icp(src, tgt, MAX_DIST, init, "p2plane", b._nrm, loss=reg.TukeyLoss(R.TUKEY_K))
    assert np.array_equal(res.transformation, r["transformation"]) and res.fitness == r["fitness"] and res.inlier_rmse == r["inlier_rmse"]
    assert not np.array_equal(res.transformation, reg.registration_icp(a, b, MAX_DIST, init, reg.TransformationEstimationPointToPlane()).transformation)
    assert np.array_equal(np.asarray(a.points), pa) and np.array_equal(np.asarray(b.points), pb) and np.array_equal(np.asarray(b.normals), nb)
    gi, gd = ops.nn_search(src, tgt, res.transformation)
    ok = _npy(gd) < MAX_DIST ** 2
    assert np.array_equal(np.asarray(res.correspondence_set), np.stack([np.flatnonzero(ok), _npy(gi)[ok]], 1))
    with pytest.raises(ValueError, match="PointToPoint"):
        ops.icp(src, tgt, MAX_DIST, None, "p2p", None, 5, loss=reg.TukeyLoss(10.0))
    g = reg.registration_generalized_icp(a, b, MAX_DIST, init, reg.TransformationEstimationForGeneralizedICP(1e-3, reg.HuberLoss(30.0)),
                                         reg.ICPConvergenceCriteria(max_iteration=12))
    assert np.isfinite(g.transformation).all() and g.fitness > 0.9 and np.abs(g.transformation[:3, 3] - T[:3, 3]).max() < 6.0
    plain = reg.registration_generalized_icp(a, b, MAX_DIST, init, None, reg.ICPConvergenceCriteria(max_iteration=12))
    assert not np.array_equal(g.transformation, plain.transformation)
    assert not a.has_covariances() and not b.has_covariances() and not a.has_normals()


def test_pipeline_surface(ops, reg, oracle):
    """execute_point_to_plane_registration and DataProcessor with a kernel, on two sensors of the ring with the outliers of the CPU suite
    in the sub's cloud"""
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.data import DataProcessor
    from kinectpy_amd.preprocessing.registration import execute_multiway_registration, execute_point_to_plane_registration
    from kinectpy_amd.utils.io import rgbd_to_pointcloud
    xy, depth, rgb, inits, truth = synth.sensor_ring(4, 1, synth.small_xy(), sensors=[0, 1, 2])
    clouds = [rgbd_to_pointcloud(rgb[0][i], oracle.unproject_u16(depth[0][i], xy)) for i in range(3)]
    master, sub, sub2 = clouds[0], PointCloud(R.displaced(_npy(clouds[1]._pts))), clouds[2]
    loss = reg.TukeyLoss(R.TUKEY_K)
    Tk = execute_point_to_plane_registration(master, sub, inits[0], kernel=loss)
    T0 = execute_point_to_plane_registration(master, sub, inits[0])
    assert Tk.shape == (4, 4) and np.isfinite(Tk).all() and np.array_equal(Tk[3], [0, 0, 0, 1]) and not np.array_equal(Tk, T0)
    assert np.array_equal(T0, execute_point_to_plane_registration(master, sub, inits[0], kernel=None))
    dp = DataProcessor.in_memory(2, [inits[0]], robust_kernel=loss)
    assert np.array_equal(dp.find_registration_transforms(master, [sub])[0], Tk)
    assert np.array_equal(DataProcessor.in_memory(2, [inits[0]]).find_registration_transforms(master, [sub])[0], T0)
    multi = execute_multiway_registration([master, sub, sub2], 35, initial_transformations=inits[:2], kernel=loss)
    assert len(multi) == 2 and all(np.isfinite(m).all() for m in multi)

"""CPU checks of the robust-kernel restatement (tests/robust_ref.py) and of the Python surface of the robust losses: the weights
against values worked out by hand, the restated loops with L2 against the existing references bit for bit, the point of the
feature on the reference alone (Tukey against displaced source points), and the argument errors raised before the library is
touched (it cannot run without a GPU)."""
import numpy as np
import pytest

import gicp_ref as G
import robust_ref as R
from kinectpy_amd.utils import synth


def _classes(reg):
    return {"l2": reg.L2Loss(), "l1": reg.L1Loss(), "huber": reg.HuberLoss(4.0), "cauchy": reg.CauchyLoss(4.0), "gm": reg.GMLoss(4.0),
            "tukey": reg.TukeyLoss(4.0)}


def test_weights_known_answers():
    """values by hand, k = 4: Tukey (1 - (1/2)^2)^2 = 0.5625 and 0 from k on; Huber k / 2k = 0.5 and 1 inside k; Cauchy 1 / (1 + 1);
    GM k / k^2 = 1 / k at 0; L1 1 / |-2|"""
    from kinectpy_amd import o3d
    losses = _classes(o3d.pipelines.registration)
    k = 4.0
    cases = [("tukey", k / 2, 0.5625), ("tukey", k, 0.0), ("tukey", 3 * k, 0.0), ("tukey", -3 * k, 0.0), ("tukey", 0.0, 1.0),
             ("huber", 2 * k, 0.5), ("huber", -2 * k, 0.5), ("huber", k, 1.0), ("huber", -0.5 * k, 1.0), ("huber", 0.0, 1.0),
             ("cauchy", k, 0.5), ("cauchy", 0.0, 1.0), ("gm", 0.0, 1.0 / k), ("gm", 2.0, k / 64.0), ("l1", -2.0, 0.5), ("l1", 8.0, 0.125),
             ("l2", -7.0, 1.0)]
    for kind, r, want in cases:
        assert R.weight(kind, k, r) == want, (kind, r)
        assert losses[kind].weight(r) == want, (kind, r)
        assert losses[kind].kind == kind and losses[kind].k == (None if kind in ("l2", "l1") else k)
    assert np.isinf(R.weight("l1", 0.0, 0.0)) and np.isinf(losses["l1"].weight(0.0))
    # the classes and the restatement are the same formula on arrays, bit for bit
    r = np.random.default_rng(0).normal(scale=6.0, size=1000)
    for kind, loss in losses.items():
        assert np.array_equal(loss.weight(r), R.weight(kind, k, r)), kind


def test_rows_with_a_non_finite_weight_are_dropped():
    J = np.arange(18.0).reshape(3, 6)
    r = np.array([0.0, 2.0, -4.0])
    Jw, rw = R.scaled_rows("l1", 0.0, J, r)
    assert Jw.shape == (2, 6) and np.array_equal(Jw[0], np.sqrt(0.5) * J[1]) and np.array_equal(rw, [np.sqrt(0.5) * 2.0, np.sqrt(0.25) * -4.0])
    Jw, rw = R.scaled_rows("tukey", 3.0, J, r)                           # weight 0 beyond k: the row stays, as zeros
    assert Jw.shape == (3, 6) and not Jw[2].any() and rw[2] == 0.0 and np.array_equal(Jw[0], J[0])


@pytest.fixture(scope="module")
def pair(oracle, base_cloud):
    src, tgt, T = synth.icp_pair(3000, base_cloud)
    return src, tgt, T, oracle.estimate_normals(tgt, 1e150, 20)[0].astype(np.float32)


def test_l2_point_to_plane_is_the_oracle_loop_bit_for_bit(oracle, pair):
    src, tgt, T, tn = pair
    for init, iters in ((None, 30), (synth.perturb(T, 0.5, 10.0, seed=1), 12)):
        a = oracle.registration_icp(src, tgt, 100.0, init, "p2plane", tn, iters)
        b = R.registration_icp_robust(oracle, src, tgt, tn, 100.0, "l2", 0.0, init, iters)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:4] and a[3] >= 2


def test_l2_coloured_is_the_oracle_loop_bit_for_bit(oracle):
    src, sc, tgt, tc, _ = synth.coloured_pair(3000)
    tn = oracle.estimate_normals(tgt, 1e150, 20)[0].astype(np.float32)
    a = oracle.registration_colored_icp(src, sc, tgt, tc, tn, 80.0, None, 0.968, 20)
    b = R.registration_colored_icp_robust(oracle, src, sc, tgt, tc, tn, 80.0, "l2", 0.0, None, 0.968, 20)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:4] and a[3] >= 2


def test_l2_gicp_is_the_restated_loop_bit_for_bit(oracle, pair):
    src, tgt, _, tn = pair
    Cs = G.covariances_from_normals(oracle.estimate_normals(src, 1e150, 20)[0])
    Ct = G.covariances_from_normals(tn)
    a = G.registration_generalized_icp(oracle, src, tgt, 100.0, Cs, Ct, None, 30)
    b = R.registration_generalized_icp_robust(oracle, src, tgt, 100.0, Cs, Ct, "l2", 0.0, None, 30)
    assert np.array_equal(a[0], b[0]) and a[1:4] == b[1:4] and a[3] >= 2
    assert np.array_equal(a[4][0], b[4][0]) and np.array_equal(a[4][1], b[4][1])


def test_loss_changes_the_update_and_nothing_else(oracle, pair):
    """one search at a fixed transform: slots 0..16 do not depend on the loss, slots 17..43 do"""
    src, tgt, _, tn = pair
    idx, d2, _ = oracle.nn(src, np.eye(4), tgt, grid=True)
    accs = {kd: R.p2plane_accumulate(oracle, src, np.eye(4), tgt, tn, idx, d2, 100.0, kd, 20.0) for kd in R.KINDS}
    for kd in R.KINDS[1:]:
        assert np.array_equal(accs[kd][:17], accs["l2"][:17]) and not np.array_equal(accs[kd][17:], accs["l2"][17:])
        assert np.isfinite(accs[kd]).all()


def test_tukey_rejects_displaced_points(oracle, pair):
    src, tgt, T, tn = pair
    bad = R.displaced(src)
    init = synth.perturb(T, 0.5, 10.0, seed=1)
    dist = lambda r: float(np.linalg.norm(r[0][:3, 3] - T[:3, 3]))
    l2 = R.registration_icp_robust(oracle, bad, tgt, tn, 100.0, "l2", 0.0, init, 30)
    tk = R.registration_icp_robust(oracle, bad, tgt, tn, 100.0, "tukey", R.TUKEY_K, init, 30)
    print(f"\ndistance from T*: L2 {dist(l2):.3f} mm, Tukey({R.TUKEY_K}) {dist(tk):.3f} mm")
    assert dist(l2) > 8.0 and dist(tk) < 0.25 * dist(l2)
    assert np.abs(tk[0][:3, :3] - T[:3, :3]).max() <= np.abs(l2[0][:3, :3] - T[:3, :3]).max()


def test_api_errors():
    from kinectpy_amd import o3d, ops
    reg = o3d.pipelines.registration
    with pytest.raises(TypeError):
        reg.TransformationEstimationPointToPlane(kernel=object())
    with pytest.raises(TypeError):
        reg.TransformationEstimationForColoredICP(0.968, kernel="tukey")
    with pytest.raises(NotImplementedError):
        reg.TransformationEstimationForGeneralizedICP(kernel=object())
    for cls in (reg.HuberLoss, reg.CauchyLoss, reg.GMLoss, reg.TukeyLoss):
        with pytest.raises(ValueError):
            cls(0)
        with pytest.raises(ValueError):
            cls(float("nan"))
        with pytest.raises(TypeError):
            cls()                                                          # k is required, as in Open3D
        assert isinstance(cls(2.5), reg.RobustKernel) and cls(2.5).k == 2.5
    assert reg.TransformationEstimationForGeneralizedICP(kernel=reg.TukeyLoss(10.0)).kernel.k == 10.0
    assert reg.TransformationEstimationPointToPlane().kernel is None and reg.TransformationEstimationPointToPlane.mode == "p2plane"
    assert reg.TransformationEstimationForColoredICP().lambda_geometric == 0.968
    pts = np.zeros((4, 3), np.float32)
    for loss in (reg.TukeyLoss(10.0), reg.L1Loss(), ("huber", 3.0)):
        with pytest.raises(ValueError, match="PointToPoint"):             # before the library is loaded or a device asked for
            ops.icp(pts, pts, 100.0, None, "p2p", None, 5, loss=loss)
    with pytest.raises(ValueError, match="unknown robust loss"):
        ops.icp(pts, pts, 100.0, None, "p2plane", pts, 5, loss=object())


def test_library_refuses_bad_losses_without_a_device():
    """the C entry points' own checks come before anything touches a device"""
    import ctypes as C
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    import os
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    lib = _lib.load()
    init = np.eye(4)
    hp = init.ctypes.data_as(C.c_void_p)
    d = C.c_double
    icp = lambda mode, loss, k: lib.kpx_icp_robust(None, 5, None, None, 5, d(100.0), hp, mode, 30, d(1e-6), d(1e-6), 0, None, None, None,
                                                   None, 0, None, loss, d(k))
    assert icp(0, 5, 10.0) == -1 and b"PointToPoint" in lib.kpx_last_error()
    assert icp(1, 6, 10.0) == -1 and b"unknown robust loss" in lib.kpx_last_error()
    assert icp(1, -1, 10.0) == -1 and b"unknown robust loss" in lib.kpx_last_error()
    for loss in (2, 3, 4, 5):
        assert icp(1, loss, 0.0) == -1 and b"must be positive" in lib.kpx_last_error()
    assert icp(1, 1, 0.0) == -1 and b"normal" in lib.kpx_last_error()          # L1 needs no k: the next check (no normals) answers
    rc = lib.kpx_colored_icp_robust(None, None, 5, None, None, None, None, 5, d(80.0), hp, d(0.968), 30, d(1e-6), d(1e-6), 0, None, None, 0,
                                    None, 5, d(-1.0))
    assert rc == -1 and b"must be positive" in lib.kpx_last_error()
    rc = lib.kpx_generalized_icp_robust(None, None, 5, None, None, 5, d(100.0), hp, 30, d(1e-6), d(1e-6), 0, None, None, None, None, 0, None,
                                        9, d(1.0))
    assert rc == -1 and b"unknown robust loss" in lib.kpx_last_error()

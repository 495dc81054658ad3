"""CPU checks of the generalized-ICP restatement (tests/gicp_ref.py) itself: GetRotationFromE1ToX against the closed form, the
GICP normal equations against finite differences, and the restated loop recovering the ground truth."""
import numpy as np

import gicp_ref as G
from kinectpy_amd.utils import synth


def _rot_zyx(a, b, g):
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def test_covariances_from_normals_closed_form_and_quirk():
    rng = np.random.default_rng(5)
    n = rng.normal(size=(4000, 3))
    n = np.concatenate([n, [[0, 0, 1], [1, 0, 0], [0, 1, 0], [-0.98, np.sqrt(1 - 0.98 ** 2), 0]]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = n[n[:, 0] > -0.985]
    for eps in (1e-3, 0.25):
        C = G.covariances_from_normals(n, eps)
        closed = np.eye(3) - (1.0 - eps) * n[:, :, None] * n[:, None, :]
        assert np.abs(C - closed).max() < 1e-12
    quirk = np.array([[-1, 0, 0], [-0.995, np.sqrt(1 - 0.995 ** 2), 0], [-0.9999, 0, np.sqrt(1 - 0.9999 ** 2)]])
    Cq = G.covariances_from_normals(quirk, 1e-3)
    assert np.array_equal(Cq, np.broadcast_to(np.diag([1e-3, 1.0, 1.0]), Cq.shape))


def test_normal_equations_match_finite_differences(oracle):
    """J^T J and J^T r of the accumulated rows against central differences of the residual r(x) = W (U(x) s - t) and of
    f(x) = 1/2 sum |r(x)|^2, W held fixed, U(x) = [Rz(x2) Ry(x1) Rx(x0) | x3..5]"""
    src, tgt, Tstar = synth.icp_pair(3000)
    nrm_s = oracle.estimate_normals(src, 1e150, 20)[0]
    Cs, Ct = G.covariances_from_normals(nrm_s, 0.05), G.estimate_covariances(oracle, tgt, 1e150, 30)
    T = np.linalg.inv(np.linalg.inv(Tstar))
    T[:3, 3] += [4.0, -3.0, 2.0]
    T[:3, :3] = _rot_zyx(0.01, -0.02, 0.015) @ T[:3, :3]
    idx, d2, _ = oracle.nn(src, T, tgt, grid=True)
    acc = G.gicp_accumulate(oracle, src, T, tgt, idx, d2, 100.0, Cs, Ct)
    ok = d2 < 100.0 ** 2
    s = src.astype(np.float64)[ok] @ T[:3, :3].T + T[:3, 3]
    t = tgt.astype(np.float64)[idx[ok]]
    W, good = G.pair_weights(T[:3, :3], Cs[ok], Ct[idx[ok]])
    assert good.all() and ok.sum() > 300
    s, t, W = s[good], t[good], W[good]

    def resid(x):
        sx = s @ _rot_zyx(x[0], x[1], x[2]).T + x[3:6]
        return np.einsum("kij,kj->ki", W, sx - t).reshape(-1)

    h = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
    J = np.stack([(resid(h[c] * np.eye(6)[c]) - resid(-h[c] * np.eye(6)[c])) / (2 * h[c]) for c in range(6)], 1)
    r0 = resid(np.zeros(6))
    JtJ = np.zeros((6, 6))
    q = 17
    for a in range(6):
        for b in range(a, 6):
            JtJ[a, b] = JtJ[b, a] = acc[q]
            q += 1
    assert np.abs(J.T @ J - JtJ).max() < 1e-6 * np.abs(JtJ).max()
    assert np.abs(J.T @ r0 - acc[38:44]).max() < 1e-6 * np.abs(acc[38:44]).max()
    f = lambda x: 0.5 * np.dot(resid(x), resid(x))
    grad = np.array([(f(h[c] * np.eye(6)[c]) - f(-h[c] * np.eye(6)[c])) / (2 * h[c]) for c in range(6)])
    assert np.abs(grad - acc[38:44]).max() < 1e-5 * np.abs(acc[38:44]).max()


def test_singular_pairs_contribute_nothing():
    R = np.eye(3)
    flat = np.diag([1.0, 1.0, 0.0])[None]
    W, ok = G.pair_weights(R, flat, flat)
    assert not ok[0]
    W, ok = G.pair_weights(R, np.diag([1.0, 1.0, 0.0])[None], np.diag([0.0, 1.0, 1.0])[None])
    assert ok[0] and np.allclose(W[0] @ W[0] @ np.diag([1.0, 2.0, 1.0]), np.eye(3))


def test_restated_loop_recovers_ground_truth(oracle):
    src, tgt, Tstar = synth.icp_pair(3000)
    Cs = G.covariances_from_normals(oracle.estimate_normals(src, 1e150, 20)[0])
    Ct = G.covariances_from_normals(oracle.estimate_normals(tgt, 1e150, 20)[0])
    T, fit, rmse, it, _ = G.registration_generalized_icp(oracle, src, tgt, 100.0, Cs, Ct, None, 60)
    assert fit > 0.9 and it >= 2
    assert np.abs(T[:3, :3] - Tstar[:3, :3]).max() < 5e-3 and np.abs(T[:3, 3] - Tstar[:3, 3]).max() < 6.0

"""NumPy fp64 restatement of Open3D's generalized ICP (the contract of kpx_estimate_covariances, kpx_gicp_covariances and
kpx_generalized_icp), composed from the oracle's exported functions (hybrid_knn, covariances, nn, p2plane_from_sums).
[O3D] notes, written from Open3D >= 0.15 (not verifiable here: Open3D is not installed):

- PointCloud.estimate_covariances(search_param = KDTreeSearchParamKNN(30)): per point the neighbours of estimate_normals' search;
  >= 3 of them: ComputeCovariance = cumulants / m, E[x x^T] - mu mu^T (divisor m); fewer: the identity.
- InitializePointCloudForGeneralizedICP(cloud, epsilon) works on a copy: covariances as they are if the cloud has them, else from
  its normals, else from normals estimated with KDTreeSearchParamKNN(20).  From normals: C = R_x diag(epsilon, 1, 1) R_x^T with
  R_x = GetRotationFromE1ToX(n): v = e1 x n, c = e1 . n; c < -0.99 -> I (kept); else I + [v]x + [v]x^2 / (1 + c).
- The loop is registration_icp's.  Per correspondence (s = T src, t): Cs' = R Cs R^T, M = Ct + Cs', W = M^{-1/2}, d = s - t;
  three rows r_i = w_i . d, J_i = (s x w_i, w_i) into the point-to-plane normal equations; Rz Ry Rx update.
- Deviation (the library's and this restatement's): a pair whose M has a smallest eigenvalue <= 0 or a non-finite W adds nothing
  (Open3D: NaN); a singular 6x6 system gives the identity update (p2plane_from_sums).

`O` is the oracle module (tests take the session `oracle` fixture)."""
import numpy as np


def _sym(cov6):
    cov6 = np.asarray(cov6, dtype=np.float64)
    C = np.empty((len(cov6), 3, 3))
    C[:, 0, 0], C[:, 0, 1], C[:, 0, 2] = cov6[:, 0], cov6[:, 1], cov6[:, 2]
    C[:, 1, 0], C[:, 1, 1], C[:, 1, 2] = cov6[:, 1], cov6[:, 3], cov6[:, 4]
    C[:, 2, 0], C[:, 2, 1], C[:, 2, 2] = cov6[:, 2], cov6[:, 4], cov6[:, 5]
    return C


def estimate_covariances(O, pts, radius, max_nn):
    """(N, 3, 3) f64; the oracle writes zeros where a point has < 3 neighbours: Open3D's identity goes there"""
    nbr, cnt = O.hybrid_knn(pts, radius, max_nn)
    C = _sym(O.covariances(pts, nbr, cnt))
    C[cnt < 3] = np.eye(3)
    return C


def rotation_e1_to_x(normals):
    """GetRotationFromE1ToX, literally, per row of normals (in fp64; the library's float32 normals convert exactly)"""
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    c = n[:, 0]
    v0, v1, v2 = np.zeros(len(n)), -n[:, 2], n[:, 1]                  # e1 x n
    S = np.zeros((len(n), 3, 3))
    S[:, 0, 1], S[:, 0, 2] = -v2, v1
    S[:, 1, 0], S[:, 1, 2] = v2, -v0
    S[:, 2, 0], S[:, 2, 1] = -v1, v0
    quirk = c < -0.99
    f = 1.0 / np.where(quirk, 1.0, 1.0 + c)
    R = np.eye(3) + S + (S @ S) * f[:, None, None]
    R[quirk] = np.eye(3)
    return R


def covariances_from_normals(normals, epsilon=1e-3):
    R = rotation_e1_to_x(normals)
    return R @ np.diag([epsilon, 1.0, 1.0]) @ np.transpose(R, (0, 2, 1))


def pair_weights(R, Cs, Ct):
    """W = (Ct + R Cs R^T)^{-1/2} per pair and the mask of pairs that contribute (smallest eigenvalue > 0, W finite)"""
    M = Ct + R @ Cs @ R.T
    lam, V = np.linalg.eigh(M)
    ok = lam[:, 0] > 0
    il = 1.0 / np.sqrt(np.where(ok[:, None], lam, 1.0))
    W = (V * il[:, None, :]) @ np.transpose(V, (0, 2, 1))
    ok &= np.isfinite(W).all(axis=(1, 2))
    return W, ok


def gicp_sums(s, t, W):
    """J^T J upper triangle (21) and J^T r (6) over the three rows of every pair"""
    d = s - t
    JtJ, Jtr = np.zeros((6, 6)), np.zeros(6)
    for i in range(3):
        w = W[:, i, :]
        r = (w * d).sum(1)
        J = np.concatenate([np.cross(s, w), w], 1)
        JtJ += J.T @ J
        Jtr += J.T @ r
    return np.array([JtJ[p, c] for p in range(6) for c in range(p, 6)]), Jtr


def gicp_accumulate(O, src, T, tgt, idx, d2, max_dist, src_cov, tgt_cov):
    """the 44 accumulator slots of one iteration: 0..16 as registration_icp's, 17..43 the GICP normal equations"""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    ok = (idx >= 0) & (d2 < max_dist * max_dist)
    s = np.asarray(src, dtype=np.float32).reshape(-1, 3).astype(np.float64)[ok] @ T[:3, :3].T + T[:3, 3]
    t = np.asarray(tgt, dtype=np.float32).reshape(-1, 3).astype(np.float64)[idx[ok]]
    acc = np.zeros(44)
    acc[0], acc[1] = ok.sum(), d2[ok].sum()
    acc[2:5], acc[5:8], acc[8:17] = s.sum(0), t.sum(0), (t.T @ s).reshape(-1)
    W, good = pair_weights(T[:3, :3], np.asarray(src_cov).reshape(-1, 3, 3)[ok], np.asarray(tgt_cov).reshape(-1, 3, 3)[idx[ok]])
    acc[17:38], acc[38:44] = gicp_sums(s[good], t[good], W[good])
    return acc


def registration_generalized_icp(O, src, tgt, max_dist, src_cov, tgt_cov, init=None, max_iteration=30, relative_fitness=1e-6,
                                 relative_rmse=1e-6):
    """oracle.registration_icp's loop with the GICP sums.  Returns T, fitness, rmse, iterations, (idx, d2) of the last search."""
    n = len(np.asarray(src).reshape(-1, 3))
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    last = {}

    def search(Tc):
        idx, d2, _ = O.nn(src, Tc, tgt, grid=True)
        last["idx"], last["d2"] = idx, d2
        acc = gicp_accumulate(O, src, Tc, tgt, idx, d2, max_dist, src_cov, tgt_cov)
        cnt = acc[0]
        return acc, (cnt / n if n else 0.0), (np.sqrt(acc[1] / cnt) if cnt else 0.0)

    acc, fit, rmse = search(T)
    it = 0
    for it in range(1, max_iteration + 1):
        T = O.p2plane_from_sums(acc) @ T
        acc, nfit, nrmse = search(T)
        done = abs(fit - nfit) < relative_fitness and abs(rmse - nrmse) < relative_rmse
        fit, rmse = nfit, nrmse
        if done:
            break
    return T, fit, rmse, it, (last["idx"], last["d2"])

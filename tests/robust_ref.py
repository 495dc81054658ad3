"""NumPy fp64 restatement of Open3D's robust kernels in registration_icp (point-to-plane), registration_colored_icp and
registration_generalized_icp -- the contract of kpx_icp_robust, kpx_colored_icp_robust and kpx_generalized_icp_robust -- composed
from the oracle's exported functions (nn, icp_accumulate, transform, color_gradient, p2plane_from_sums) and gicp_ref.pair_weights.
[O3D] notes, written from Open3D >= 0.15 (not verifiable here: Open3D is not installed):

- RobustKernel.cpp, weight w(r): L2 1; L1 1 / |r|; Huber k / max(|r|, k); Cauchy 1 / (1 + (r / k)^2); GM k / (k + r^2)^2;
  Tukey (1 - min(1, |r| / k)^2)^2.
- ComputeJTJandJTr: per residual row JTJ += J w J^T, JTr += J w r.  Rows: point-to-plane one, r = (s - t) . n; coloured ICP two,
  each weighted by its own SCALED residual (sqrt(lambda) r_G, sqrt(1 - lambda) r_I); GICP three, r_i = w_i . d.
- Correspondences, fitness, inlier rmse, the convergence test and so the iteration count do not depend on the loss: accumulator
  slots 0..16 (count, sum d2, the point-to-point sums) stay unweighted, slots 17..43 hold the weighted normal equations.
- Deviation (the library's and this restatement's): a row whose weight is not finite adds nothing to slots 17..43 (Open3D: NaN
  from L1 at r == 0).

A weighted row enters here as the row (sqrt(w) J, sqrt(w) r) -- the same normal equations -- so that each loop below is its L2
reference (oracle.registration_icp, oracle.registration_colored_icp, gicp_ref.registration_generalized_icp) with scaled_rows
inserted and nothing else: with L2 every factor is exactly 1 and the results are those references' bit for bit.

`O` is the oracle module (tests take the session `oracle` fixture).  `order`: a seed; the pair rows are summed in that random
order instead of the clouds' (how far the result depends on the order of the sums: the spread the GPU suite's tolerances for the
unbounded weights come from)."""
import numpy as np

import gicp_ref as G

KINDS = ("l2", "l1", "huber", "cauchy", "gm", "tukey")

# The outlier case of the suites, chosen on this CPU reference (synth.icp_pair(3000), point-to-plane, max_dist 100, start 0.5 deg /
# 10 mm from the truth): with 30 % of the source moved 40 mm off the surface L2 ends 12.9 mm from T*, Tukey(25) 0.5 mm (every k
# from 15 to 40 ends below 1.7 mm).
OUTLIER_SHARE, OUTLIER_MM, TUKEY_K = 0.30, 40.0, 25.0


def displaced(src, share=OUTLIER_SHARE, mm=OUTLIER_MM, seed=5):
    """`share` of the points moved `mm` along the camera's z axis: flying pixels off the surface"""
    out = np.array(src, dtype=np.float32).reshape(-1, 3)
    bad = np.random.default_rng(seed).choice(len(out), int(share * len(out)), replace=False)
    out[bad, 2] += np.float32(mm)
    return out


def weight(kind, k, r):
    """w(r), with the operations of RobustLoss::weight (kpx_icpdefs.h) in their order"""
    r = np.asarray(r, dtype=np.float64)
    if kind == "l2":
        return np.ones_like(r)
    if kind == "l1":
        with np.errstate(divide="ignore"):
            return 1.0 / np.abs(r)
    if kind == "huber":
        return k / np.maximum(np.abs(r), k)
    if kind == "cauchy":
        q = r / k
        return 1.0 / (1.0 + q * q)
    if kind == "gm":
        d = k + r * r
        return k / (d * d)
    if kind == "tukey":
        q = np.minimum(1.0, np.abs(r) / k)
        u = 1.0 - q * q
        return u * u
    raise ValueError(kind)


def scaled_rows(kind, k, J, r, order=None):
    """rows (J (m, 6), r (m)) -> (sqrt(w) J, sqrt(w) r) without the rows whose weight is not finite"""
    w = weight(kind, k, r)
    keep = np.isfinite(w)
    sw = np.sqrt(w[keep])
    J, r = sw[:, None] * J[keep], sw * r[keep]
    if order is not None:
        p = np.random.default_rng(order).permutation(len(r))
        J, r = np.ascontiguousarray(J[p]), r[p]
    return J, r


def _seq_sum(cols):
    """per column, the sum in row order (the order of the oracle's C loops; np.sum adds pairwise)"""
    return np.cumsum(cols, axis=0)[-1] if len(cols) else np.zeros(cols.shape[1])


def p2plane_accumulate(O, src, T, tgt, tn, idx, d2, max_dist, kind, k, order=None):
    """oracle.icp_accumulate with weighted point-to-plane rows: slots 0..16 are its own, 17..43 its arithmetic row by row"""
    acc = O.icp_accumulate(src, T, tgt, idx, d2, max_dist, None)
    ok = d2 < max_dist * max_dist
    with O.storage("f64"):                                                 # T . src by the contract's fma chain, kept in fp64
        s = O.transform(np.asarray(src, dtype=np.float32).reshape(-1, 3).astype(np.float64)[ok], T)
    t = np.asarray(tgt, dtype=np.float32).reshape(-1, 3).astype(np.float64)[idx[ok]]
    n = np.asarray(tn, dtype=np.float32).reshape(-1, 3).astype(np.float64)[idx[ok]]
    r = (s[:, 0] - t[:, 0]) * n[:, 0] + (s[:, 1] - t[:, 1]) * n[:, 1] + (s[:, 2] - t[:, 2]) * n[:, 2]
    J = np.stack([s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1], s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2], s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2]], 1)
    J, r = scaled_rows(kind, k, J, r, order)
    cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)]
    acc[17:44] = _seq_sum(np.stack(cols, 1))
    return acc


def colored_accumulate(O, src, Is, T, tgt, It, tn, grad, slg, slp, idx, d2, max_dist, kind, k, order=None):
    """the sums of oracle.registration_colored_icp's update in the 44-slot layout, each of the two rows weighted by its own
    scaled residual"""
    ok = d2 < max_dist * max_dist
    acc = np.zeros(44)
    acc[0], acc[1] = ok.sum(), d2[ok].sum()
    if not ok.any():
        return acc
    s = (src[ok].astype(np.float64) @ T[:3, :3].T) + T[:3, 3]
    j = idx[ok]
    t, nv, g = tgt[j].astype(np.float64), tn[j], grad[j]
    acc[2:5], acc[5:8], acc[8:17] = s.sum(0), t.sum(0), (t.T @ s).reshape(-1)
    rg = ((s - t) * nv).sum(1)
    sp = s - rg[:, None] * nv
    is0 = (g * (sp - t)).sum(1) + It[j]
    gm = -(g - (g * nv).sum(1)[:, None] * nv)
    JG = slg * np.hstack([np.cross(s, nv), nv])
    JI = slp * np.hstack([np.cross(s, gm), gm])
    rG, rI = slg * rg, slp * (Is[ok] - is0)
    JG, rG = scaled_rows(kind, k, JG, rG, order)
    JI, rI = scaled_rows(kind, k, JI, rI, order)
    A = JG.T @ JG + JI.T @ JI
    acc[17:38] = [A[p, c] for p in range(6) for c in range(p, 6)]
    acc[38:44] = JG.T @ rG + JI.T @ rI
    return acc


def gicp_accumulate(O, src, T, tgt, idx, d2, max_dist, src_cov, tgt_cov, kind, k, order=None):
    """gicp_ref.gicp_accumulate with each of a pair's three rows weighted by its own residual"""
    ok = (idx >= 0) & (d2 < max_dist * max_dist)
    s = np.asarray(src, dtype=np.float32).reshape(-1, 3).astype(np.float64)[ok] @ T[:3, :3].T + T[:3, 3]
    t = np.asarray(tgt, dtype=np.float32).reshape(-1, 3).astype(np.float64)[idx[ok]]
    acc = np.zeros(44)
    acc[0], acc[1] = ok.sum(), d2[ok].sum()
    acc[2:5], acc[5:8], acc[8:17] = s.sum(0), t.sum(0), (t.T @ s).reshape(-1)
    W, good = G.pair_weights(T[:3, :3], np.asarray(src_cov).reshape(-1, 3, 3)[ok], np.asarray(tgt_cov).reshape(-1, 3, 3)[idx[ok]])
    s, t, W = s[good], t[good], W[good]
    d = s - t
    JtJ, Jtr = np.zeros((6, 6)), np.zeros(6)
    for i in range(3):
        w = W[:, i, :]
        r = (w * d).sum(1)
        J = np.concatenate([np.cross(s, w), w], 1)
        J, r = scaled_rows(kind, k, J, r, order)
        JtJ += J.T @ J
        Jtr += J.T @ r
    acc[17:38], acc[38:44] = np.array([JtJ[p, c] for p in range(6) for c in range(p, 6)]), Jtr
    return acc


def _loop(O, src, tgt, accumulate, init, max_iteration, relative_fitness, relative_rmse):
    """oracle.registration_icp's loop around accumulate(T, idx, d2) -> 44 slots; the update is the point-to-plane solve.
    Returns T, fitness, rmse, iterations, (idx, d2) of the last search."""
    n = len(src)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    last = {}

    def search(Tc):
        idx, d2, _ = O.nn(src, Tc, tgt, grid=True)
        last["idx"], last["d2"] = idx, d2
        acc = accumulate(Tc, idx, d2)
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


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def registration_icp_robust(O, src, tgt, tgt_normals, max_dist, kind="l2", k=0.0, init=None, max_iteration=30, relative_fitness=1e-6,
                            relative_rmse=1e-6, order=None):
    """registration_icp with TransformationEstimationPointToPlane(kernel)"""
    src, tgt, tn = _f32(src), _f32(tgt), _f32(tgt_normals)
    return _loop(O, src, tgt, lambda T, idx, d2: p2plane_accumulate(O, src, T, tgt, tn, idx, d2, max_dist, kind, k, order),
                 init, max_iteration, relative_fitness, relative_rmse)


def registration_colored_icp_robust(O, src, src_colors, tgt, tgt_colors, tgt_normals, max_dist, kind="l2", k=0.0, init=None,
                                    lambda_geometric=0.968, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, order=None,
                                    tgt_gradient=None):
    """registration_colored_icp with TransformationEstimationForColoredICP(lambda_geometric, kernel)"""
    src, tgt = _f32(src), _f32(tgt)
    tn = _f32(tgt_normals).astype(np.float64)
    Is = _f32(src_colors).astype(np.float64).sum(1) / 3.0
    It = _f32(tgt_colors).astype(np.float64).sum(1) / 3.0
    grad = O.color_gradient(tgt, tgt_normals, tgt_colors, 2.0 * max_dist, 30) if tgt_gradient is None else tgt_gradient
    slg, slp = np.sqrt(lambda_geometric), np.sqrt(1.0 - lambda_geometric)
    return _loop(O, src, tgt,
                 lambda T, idx, d2: colored_accumulate(O, src, Is, T, tgt, It, tn, grad, slg, slp, idx, d2, max_dist, kind, k, order),
                 init, max_iteration, relative_fitness, relative_rmse)


def registration_generalized_icp_robust(O, src, tgt, max_dist, src_cov, tgt_cov, kind="l2", k=0.0, init=None, max_iteration=30,
                                        relative_fitness=1e-6, relative_rmse=1e-6, order=None):
    """registration_generalized_icp with TransformationEstimationForGeneralizedICP(epsilon, kernel), covariances given"""
    src, tgt = _f32(src), _f32(tgt)
    return _loop(O, src, tgt, lambda T, idx, d2: gicp_accumulate(O, src, T, tgt, idx, d2, max_dist, src_cov, tgt_cov, kind, k, order),
                 init, max_iteration, relative_fitness, relative_rmse)

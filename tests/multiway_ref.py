"""NumPy fp64 restatement of the contract of kpx_registration_eval and of execute_multiway_registration's chain, composed from the
oracle's exported functions (nn, registration_icp) and the product's own host solver (kinectpy_amd.posegraph, NumPy only).

[O3D] evaluate_registration(source, target, d, T): nearest target of every transformed source point, kept iff d2 < d^2 (strict);
fitness = count / N, inlier_rmse = sqrt(sum d2 / count) (0 without a correspondence).
[O3D] GetInformationMatrixFromPointClouds: sum over the correspondences of G^T G, G = [-[t]x | I3] with t the matched TARGET point:
rows (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1).

Sums here are math.fsum of exact terms (a product of two float32 values is exact in fp64): correctly rounded, so a device sum of
the same n terms in any order lies within gamma_n sum|terms| of them up to that one rounding (gamma(n + 1) is used).

`O` is the oracle module (tests take the session `oracle` fixture)."""
import math

import numpy as np

U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def information_literal(t):
    """sum G^T G, one correspondence at a time, as the definition reads (float64 matrix products)"""
    L = np.zeros((6, 6))
    for x, y, z in np.asarray(t, dtype=np.float64):
        G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]], dtype=np.float64)
        L += G.T @ G
    return L


def _terms(t):
    """the terms of the ten moment sums of matched target points t (K, 3) float64 (exact float32 values): dict name -> (K,) terms"""
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    return {"x": x, "y": y, "z": z, "xx": x * x, "xy": x * y, "xz": x * z, "yy": y * y, "yz": y * z, "zz": z * z}


# every entry of the matrix: (sign, the moment sums it adds up) -- one sum, two (diagonal of the rotation block), or none
_ENTRY = {(0, 0): (1, ("yy", "zz")), (1, 1): (1, ("xx", "zz")), (2, 2): (1, ("xx", "yy")),
          (0, 1): (-1, ("xy",)), (0, 2): (-1, ("xz",)), (1, 2): (-1, ("yz",)),
          (0, 4): (-1, ("z",)), (0, 5): (1, ("y",)), (1, 3): (1, ("z",)), (1, 5): (-1, ("x",)), (2, 3): (-1, ("y",)), (2, 4): (1, ("x",))}


def information_matrix(t):
    """-> (L, B): the matrix from the moments of t, and per entry the bound gamma * sum|terms| on a float64 sum of its terms in any
    order (0 where the entry is exact: zeros and count)"""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    tm = _terms(t)
    L, B = np.zeros((6, 6)), np.zeros((6, 6))
    for (r, c), (sign, names) in _ENTRY.items():
        terms = np.concatenate([tm[k] for k in names])
        L[r, c] = L[c, r] = sign * math.fsum(terms)
        B[r, c] = B[c, r] = gamma(len(terms) + 1) * math.fsum(np.abs(terms))
    L[3, 3] = L[4, 4] = L[5, 5] = len(t)
    return L, B


def registration_eval(O, src, tgt, max_dist, T=None):
    """-> dict(idx, d2, ok, count, fitness, inlier_rmse, rmse_bound, information, information_bound)"""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64).reshape(4, 4)
    src = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, dtype=np.float32).reshape(-1, 3)
    idx, d2, _ = O.nn(src, T, tgt, grid=True)
    ok = d2 < max_dist * max_dist
    cnt = int(ok.sum())
    L, B = information_matrix(tgt[idx[ok]].astype(np.float64))
    rmse = math.sqrt(math.fsum(d2[ok]) / cnt) if cnt else 0.0
    # sum d2 (positive terms) is within the relative gamma of the exact sum; the division and the square root round once each,
    # and the square root halves a relative error: gamma + 3u is a (loose by < 2x) bound for both sides together
    return {"idx": idx, "d2": d2, "ok": ok, "count": cnt, "fitness": cnt / len(src), "inlier_rmse": rmse,
            "rmse_bound": rmse * (gamma(cnt + 1) + 3 * U), "information": L, "information_bound": B}


def multiway_chain(O, pts, nrm, inits, threshold=100.0):
    """the chain of execute_multiway_registration through the oracle: pts / nrm = the down-sampled clouds and their normals
    (float32, master first), inits = the S-1 initial sub -> master transforms.
    -> star transforms [I, T_1 ..], edges [(s, t, X, uncertain, eval dict)] in the product's order (empty ones included)"""
    S = len(pts)
    star = [np.eye(4)]
    for i in range(1, S):
        star.append(O.registration_icp(pts[i], pts[0], threshold, inits[i - 1], "p2plane", nrm[0], 30, grid=True)[0])
    edges = [(i, 0, star[i], False) for i in range(1, S)]
    for j in range(2, S):
        for i in range(1, j):
            X = O.registration_icp(pts[i], pts[j], threshold, np.linalg.inv(star[j]) @ star[i], "p2plane", nrm[j], 30, grid=True)[0]
            edges.append((i, j, X, True))
    return star, [(s, t, X, u, registration_eval(O, pts[s], pts[t], threshold, X)) for s, t, X, u in edges]


def solve_chain(star, edges, voxel_size, preference_loop_closure=None, edge_prune_threshold=0.25, threshold=100.0):
    """steps 3-5 of execute_multiway_registration on the oracle's edges with the product's host solver -> (poses, pose graph, mu)"""
    from kinectpy_amd import posegraph as PG
    g = PG.PoseGraph()
    g.nodes = [PG.PoseGraphNode(T) for T in star]
    counts = []
    for s, t, X, u, ev in edges:
        if ev["count"] == 0:
            continue
        g.edges.append(PG.PoseGraphEdge(s, t, X, ev["information"], u))
        if u:
            counts.append(ev["count"])
    mu = preference_loop_closure
    if mu is None:
        mu = (float(np.median(counts)) if counts else 1.0) * float(voxel_size) ** 2
    PG.global_optimization(g, PG.GlobalOptimizationLevenbergMarquardt(), PG.GlobalOptimizationConvergenceCriteria(),
                           PG.GlobalOptimizationOption(threshold, edge_prune_threshold, mu, 0))
    return [nd.pose.copy() for nd in g.nodes[1:]], g, mu

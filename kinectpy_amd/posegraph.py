"""Pose graph and its optimiser: o3d.pipelines.registration.PoseGraph / global_optimization (multiway registration).

Host code by design (NumPy float64 only, no kernel, importable without the library): a rig has 4-8 nodes and at most 28 edges,
48 unknowns.  The information matrices that weight the edges come from the device (ops.registration_eval).

[O3D] notes, restated from Open3D's GlobalOptimization (Choi, Zhou, Koltun, "Robust reconstruction of indoor scenes", CVPR 2015).
Open3D is not installed where this was written: bit parity with it is unpinned, what the tests pin is stated in DESIGN.md.

- An edge (s, t, X) says X ~= P_t^-1 P_s: X maps node s's frame into node t's.  Its residual is e = vec6(X^-1 P_t^-1 P_s): the three
  angles of R = Rz(e2) Ry(e1) Rx(e0), then the translation (TransformMatrix4dToVector6d).
- Objective: sum_k l_k e_k^T L_k e_k + mu sum_{k uncertain} (sqrt(l_k) - 1)^2, l_k = 1 for certain edges and the line process
  l_k = (mu / (mu + e_k^T L_k e_k))^2 for uncertain ones (the closed-form minimiser over l_k), mu = option.preference_loop_closure.
  (Open3D, as far as it can be recalled, scales its line-process weight by max_correspondence_distance^2 and the mean correspondence
  count of the edges; here mu is the number the caller gives, and execute_multiway_registration derives it from the same two
  quantities -- see DESIGN.md.)
- Levenberg-Marquardt: lambda_0 = 1e-5 max diag H; a step solves (H + lambda I) d = b and moves P_i <- V2M(d_i) P_i (left
  multiplication); gain ratio rho = (F - F_new) / (d . (lambda d + b) + 1e-3); rho > 0 accepts and scales lambda by
  max(lower_scale_factor, 1 - (2 rho - 1)^3), else lambda *= ni, ni *= 2.  Column k of J_s is the derivative of e along
  X^-1 P_t^-1 G_k P_s for the six generators G_k, J_t = -J_s.
- Stopping rules (GlobalOptimizationConvergenceCriteria): max |b| < min_right_term, |d| < min_relative_increment (|x| +
  min_relative_increment), F - F_new < min_relative_residual_increment F, F < min_residual, max_iteration, max_iteration_lm.
- Deviations, all on the safe side: the Jacobian is the exact derivative of vec6 (Open3D linearises it, GetLinearized6DVector:
  equal at e = 0, but with noisy edges its fixed point sits O(|e|^2) off the minimum, more than the stopping rules leave); the
  reference node's six unknowns are eliminated (Open3D leaves the gauge to the damping and moves the reference back
  afterwards: the same poses, since every residual is invariant under a common left factor); the step
  that triggers the relative-residual rule is kept (Open3D drops it); after an accepted step the stored objective is re-evaluated
  with the refreshed line process, so the recorded objective never increases.
- global_optimization: optimise, set every uncertain edge's confidence to its l_k, drop the uncertain edges with
  confidence < option.edge_prune_threshold, optimise once more.
"""
import numpy as np


class PoseGraphNode:
    def __init__(self, pose=None):
        self.pose = np.eye(4) if pose is None else np.array(pose, dtype=np.float64).reshape(4, 4)

    def __repr__(self):
        return "PoseGraphNode, access pose to get its current pose."


class PoseGraphEdge:
    def __init__(self, source_node_id=-1, target_node_id=-1, transformation=None, information=None, uncertain=False, confidence=1.0):
        self.source_node_id, self.target_node_id = int(source_node_id), int(target_node_id)
        self.transformation = np.eye(4) if transformation is None else np.array(transformation, dtype=np.float64).reshape(4, 4)
        self.information = np.eye(6) if information is None else np.array(information, dtype=np.float64).reshape(6, 6)
        self.uncertain, self.confidence = bool(uncertain), float(confidence)

    def __repr__(self):
        return f"PoseGraphEdge from nodes {self.source_node_id} to {self.target_node_id}, access transformation to get relative transformation"


class PoseGraph:
    def __init__(self):
        self.nodes, self.edges = [], []

    def __repr__(self):
        return f"PoseGraph with {len(self.nodes)} nodes and {len(self.edges)} edges."


class GlobalOptimizationConvergenceCriteria:
    def __init__(self, max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6, min_right_term=1e-6,
                 min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0):
        self.max_iteration, self.max_iteration_lm = int(max_iteration), int(max_iteration_lm)
        self.min_relative_increment, self.min_relative_residual_increment = float(min_relative_increment), float(min_relative_residual_increment)
        self.min_right_term, self.min_residual = float(min_right_term), float(min_residual)
        self.upper_scale_factor, self.lower_scale_factor = float(upper_scale_factor), float(lower_scale_factor)


class GlobalOptimizationOption:
    def __init__(self, max_correspondence_distance=0.03, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1):
        self.max_correspondence_distance, self.edge_prune_threshold = float(max_correspondence_distance), float(edge_prune_threshold)
        self.preference_loop_closure, self.reference_node = float(preference_loop_closure), int(reference_node)


class GlobalOptimizationLevenbergMarquardt:
    pass


class GlobalOptimizationGaussNewton:
    def __init__(self, *a, **k):
        raise NotImplementedError("GlobalOptimizationGaussNewton is not implemented: use GlobalOptimizationLevenbergMarquardt")


# ---- SE(3) <-> 6-vector ([O3D] Eigen.cpp) --------------------------------------------------------------------------------------
def vector6_to_matrix4(v):
    """TransformVector6dToMatrix4d: R = Rz(v2) Ry(v1) Rx(v0), t = v[3:6]"""
    ca, sa, cb, sb, cg, sg = np.cos(v[0]), np.sin(v[0]), np.cos(v[1]), np.sin(v[1]), np.cos(v[2]), np.sin(v[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rz @ Ry @ Rx
    M[:3, 3] = v[3:6]
    return M


def matrix4_to_vector6(M):
    """TransformMatrix4dToVector6d"""
    R = M[:3, :3]
    sy = np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
    if sy >= 1e-6:
        x, y, z = np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0])
    else:
        x, y, z = np.arctan2(-R[1, 2], R[1, 1]), np.arctan2(-R[2, 0], sy), 0.0
    return np.array([x, y, z, M[0, 3], M[1, 3], M[2, 3]])


def _inv(M):
    """inverse of a rigid 4x4"""
    out = np.eye(4)
    out[:3, :3] = M[:3, :3].T
    out[:3, 3] = -M[:3, :3].T @ M[:3, 3]
    return out


def _generators():
    G = np.zeros((6, 4, 4))
    G[0, 1, 2], G[0, 2, 1] = -1, 1          # rotation about x
    G[1, 0, 2], G[1, 2, 0] = 1, -1          # about y
    G[2, 0, 1], G[2, 1, 0] = -1, 1          # about z
    G[3, 0, 3] = G[4, 1, 3] = G[5, 2, 3] = 1
    return G


_G = _generators()


def _dvec6(M, dM):
    """derivative of matrix4_to_vector6 at M along each of a stack of directions dM (K, 4, 4) -> (K, 6); the regular branch
    (cos e1 != 0), which is where a residual lives"""
    R = M[:3, :3]
    sy2 = R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0]
    sy = np.sqrt(sy2)
    dsy = (R[0, 0] * dM[:, 0, 0] + R[1, 0] * dM[:, 1, 0]) / sy
    dx = (R[2, 2] * dM[:, 2, 1] - R[2, 1] * dM[:, 2, 2]) / (R[2, 1] * R[2, 1] + R[2, 2] * R[2, 2])
    dy = (-sy * dM[:, 2, 0] + R[2, 0] * dsy) / (R[2, 0] * R[2, 0] + sy2)
    dz = (R[0, 0] * dM[:, 1, 0] - R[1, 0] * dM[:, 0, 0]) / sy2
    return np.stack([dx, dy, dz, dM[:, 0, 3], dM[:, 1, 3], dM[:, 2, 3]], -1)


def edge_residual(edge, poses):
    """e = vec6(X^-1 P_t^-1 P_s)"""
    return matrix4_to_vector6(_inv(edge.transformation) @ _inv(poses[edge.target_node_id]) @ poses[edge.source_node_id])


def _chi2(pg, poses):
    out = np.empty(len(pg.edges))
    for k, ed in enumerate(pg.edges):
        e = edge_residual(ed, poses)
        out[k] = e @ ed.information @ e
    return out


def line_process(pg, poses, mu):
    """l_k: 1 for certain edges, (mu / (mu + chi2_k))^2 for uncertain ones"""
    chi = _chi2(pg, poses)
    unc = np.array([ed.uncertain for ed in pg.edges], dtype=bool)
    l = np.ones(len(pg.edges))
    l[unc] = (mu / (mu + chi[unc])) ** 2
    return l


def objective(pg, poses, l, mu):
    """sum_k l_k e^T L e + mu sum_{uncertain} (sqrt(l_k) - 1)^2"""
    chi = _chi2(pg, poses)
    unc = np.array([ed.uncertain for ed in pg.edges], dtype=bool)
    return float((l * chi).sum() + mu * ((np.sqrt(l[unc]) - 1.0) ** 2).sum())


def linear_system(pg, poses, l):
    """H (6n, 6n) and b (6n) of the Gauss-Newton step over ALL nodes (the caller drops the reference node's block)"""
    n = len(poses)
    H, b = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    for k, ed in enumerate(pg.edges):
        s, t = ed.source_node_id, ed.target_node_id
        left = _inv(ed.transformation) @ _inv(poses[t])
        e = matrix4_to_vector6(left @ poses[s])
        Js = _dvec6(left @ poses[s], left @ _G @ poses[s]).T    # (6 residual rows, 6 generators)
        Jt = -Js
        L = ed.information
        ss, tt = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
        H[ss, ss] += l[k] * Js.T @ L @ Js
        H[tt, tt] += l[k] * Jt.T @ L @ Jt
        H[ss, tt] += l[k] * Js.T @ L @ Jt
        H[tt, ss] += l[k] * Jt.T @ L @ Js
        b[ss] -= l[k] * Js.T @ L @ e
        b[tt] -= l[k] * Jt.T @ L @ e
    return H, b


def _free(n, ref):
    keep = np.ones(6 * n, dtype=bool)
    if 0 <= ref < n:
        keep[6 * ref:6 * ref + 6] = False
    return keep


def _optimize(pg, criteria, option, trace):
    """one Levenberg-Marquardt run on pg (in place); -> line process at the final poses"""
    n, mu = len(pg.nodes), option.preference_loop_closure
    poses = [nd.pose.copy() for nd in pg.nodes]
    if n == 0 or not pg.edges:
        return np.ones(len(pg.edges))
    keep = _free(n, option.reference_node)

    def system(l):
        H, b = linear_system(pg, poses, l)
        return H[np.ix_(keep, keep)], b[keep]

    def record(reason, lam):
        if trace is not None:
            trace.append({"objective": F, "lambda": lam, "reason": reason})

    l = np.ones(len(pg.edges))
    F = objective(pg, poses, l, mu)
    H, b = system(l)
    lam = 1e-5 * H.diagonal().max()
    ni = 2.0
    record("start", lam)
    stop = "right_term" if np.abs(b).max() < criteria.min_right_term else None
    if stop is None and F < criteria.min_residual:
        stop = "residual"
    it = 0
    while stop is None and it < criteria.max_iteration:
        it += 1
        lm, rho = 0, 0.0
        while True:
            try:
                d = np.linalg.solve(H + lam * np.eye(len(b)), b)
            except np.linalg.LinAlgError:
                stop = "solver"
                break
            x = np.concatenate([matrix4_to_vector6(P) for P in poses])[keep]
            if np.linalg.norm(d) < criteria.min_relative_increment * (np.linalg.norm(x) + criteria.min_relative_increment):
                stop = "relative_increment"
                break
            full = np.zeros(6 * n)
            full[keep] = d
            new = [vector6_to_matrix4(full[6 * i:6 * i + 6]) @ poses[i] for i in range(n)]
            F_new = objective(pg, new, l, mu)
            rho = (F - F_new) / (d @ (lam * d + b) + 1e-3)
            if rho > 0:
                small = F - F_new < criteria.min_relative_residual_increment * F
                lam *= max(criteria.lower_scale_factor, 1.0 - (2.0 * rho - 1.0) ** 3)
                ni = 2.0
                poses = new
                l = line_process(pg, poses, mu)
                F = objective(pg, poses, l, mu)                 # <= F_new: l is the minimiser over the line process
                H, b = system(l)
                if small:
                    stop = "relative_residual_increment"
                elif np.abs(b).max() < criteria.min_right_term:
                    stop = "right_term"
                record(stop or "accepted", lam)
                break
            lam *= ni
            ni *= 2.0
            lm += 1
            if lm >= criteria.max_iteration_lm:
                stop = "max_iteration_lm"
                break
        if stop is None and F < criteria.min_residual:
            stop = "residual"
    if trace is not None:
        trace.append({"objective": F, "lambda": lam, "reason": "end:" + (stop or "max_iteration")})
    for nd, P in zip(pg.nodes, poses):
        nd.pose = P
    return line_process(pg, poses, mu)


def global_optimization(pose_graph, method=None, criteria=None, option=None, trace=None):
    """[O3D] global_optimization(pose_graph, method, criteria, option): in place.  `trace` (a list) receives one record per accepted
    step: dict(objective, lambda, reason); a record whose reason starts with "end:" closes each of the two runs."""
    method = GlobalOptimizationLevenbergMarquardt() if method is None else method
    if not isinstance(method, GlobalOptimizationLevenbergMarquardt):
        raise NotImplementedError("global_optimization: only GlobalOptimizationLevenbergMarquardt is implemented")
    criteria = GlobalOptimizationConvergenceCriteria() if criteria is None else criteria
    option = GlobalOptimizationOption() if option is None else option
    n = len(pose_graph.nodes)
    for ed in pose_graph.edges:
        if not (0 <= ed.source_node_id < n and 0 <= ed.target_node_id < n) or ed.source_node_id == ed.target_node_id:
            raise RuntimeError("Invalid PoseGraph - an edge references an invalid node.")
    l = _optimize(pose_graph, criteria, option, trace)
    kept = []
    for ed, lk in zip(pose_graph.edges, l):
        if ed.uncertain:
            ed.confidence = float(lk)
            if ed.confidence < option.edge_prune_threshold:
                continue
        kept.append(ed)
    pose_graph.edges[:] = kept
    l = _optimize(pose_graph, criteria, option, trace)
    for ed, lk in zip(pose_graph.edges, l):
        if ed.uncertain:
            ed.confidence = float(lk)

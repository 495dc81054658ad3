"""CPU suite for multiway registration: the restatement of the information matrix against its definition, and the pose-graph
optimiser (kinectpy_amd.posegraph: NumPy only, no library, no GPU) on consistent, contradicting and noisy graphs."""
import os

import numpy as np
import pytest

import multiway_ref as M
from kinectpy_amd import posegraph as PG
from kinectpy_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _truth(n, rng):
    """random rigid poses, node 0 included (the reference node need not sit at the identity)"""
    return [PG.vector6_to_matrix4(np.concatenate([rng.uniform(-np.pi / 3, np.pi / 3, 3), rng.normal(scale=2.0, size=3)])) for _ in range(n)]


def _spd(rng):
    A = rng.normal(size=(6, 6))
    return A @ A.T + 10.0 * np.eye(6)


def _graph(n, rng, uncertain_loops=False):
    """star edges (i, 0) and every loop edge (i, j), 1 <= i < j, exact at the truth; nodes start from synth.perturb-sized errors
    (3 degrees, 0.05 of the translations' unit scale), the reference node at its truth"""
    truth = _truth(n, rng)
    g = PG.PoseGraph()
    g.nodes = [PG.PoseGraphNode(truth[0])] + [PG.PoseGraphNode(synth.perturb(truth[i], 3.0, 0.05, seed=i)) for i in range(1, n)]
    for i in range(1, n):
        g.edges.append(PG.PoseGraphEdge(i, 0, np.linalg.inv(truth[0]) @ truth[i], _spd(rng), False))
    for j in range(2, n):
        for i in range(1, j):
            g.edges.append(PG.PoseGraphEdge(i, j, np.linalg.inv(truth[j]) @ truth[i], _spd(rng), uncertain_loops))
    return g, truth


def _objective(g, mu):
    poses = [nd.pose for nd in g.nodes]
    return PG.objective(g, poses, PG.line_process(g, poses, mu), mu)


def _assert_within_truth(g, truth, min_residual):
    """objective < min_residual => every edge's e^T L e < min_residual => |e|^2 < min_residual / lambda_min(L).  Node i's star edge
    has e = vec6(truth_i^-1 pose_i) once the reference node sits at its truth, so that is node i's distance from the truth."""
    assert np.array_equal(g.nodes[0].pose, truth[0])
    star = {ed.source_node_id: ed for ed in g.edges if ed.target_node_id == 0}
    for i in range(1, len(g.nodes)):
        bound = np.sqrt(min_residual / np.linalg.eigvalsh(star[i].information)[0])
        dist = np.linalg.norm(PG.matrix4_to_vector6(np.linalg.inv(truth[i]) @ g.nodes[i].pose))
        assert dist < bound, (i, dist, bound)


def test_information_restatement_matches_the_definition():
    rng = np.random.default_rng(0)
    for k in (1, 7, 500):
        t = rng.normal(scale=1500.0, size=(k, 3)).astype(np.float32).astype(np.float64)
        L, B = M.information_matrix(t)
        lit = M.information_literal(t)
        # the literal form adds the same terms one correspondence at a time (the diagonal's two squares first): twice the bound
        # covers both roundings of a term pair and the sum
        assert (np.abs(L - lit) <= 2 * B).all()
        assert np.array_equal(L, L.T) and np.array_equal(L[3:, 3:], k * np.eye(3))
        assert (np.diag(L)[:3] > 0).all()


@pytest.mark.parametrize("n", [4, 8])
def test_consistent_graph_converges_to_the_truth(n):
    g, truth = _graph(n, np.random.default_rng(n))
    crit, opt = PG.GlobalOptimizationConvergenceCriteria(), PG.GlobalOptimizationOption(reference_node=0)
    assert _objective(g, opt.preference_loop_closure) > 1.0
    PG.global_optimization(g, PG.GlobalOptimizationLevenbergMarquardt(), crit, opt)
    assert len(g.edges) == (n - 1) + (n - 1) * (n - 2) // 2
    assert _objective(g, opt.preference_loop_closure) < crit.min_residual
    _assert_within_truth(g, truth, crit.min_residual)


@pytest.mark.parametrize("n", [4, 8])
def test_contradicting_closure_is_pruned(n):
    rng = np.random.default_rng(10 + n)
    g, truth = _graph(n, rng, uncertain_loops=True)
    crit, opt = PG.GlobalOptimizationConvergenceCriteria(), PG.GlobalOptimizationOption(reference_node=0)
    mu = opt.preference_loop_closure
    loops = [k for k, ed in enumerate(g.edges) if ed.uncertain]
    bad = g.edges[loops[len(loops) // 2]]
    bad.transformation = bad.transformation @ PG.vector6_to_matrix4(np.array([0.3, -0.4, 0.5, 0.6, -0.5, 0.4]))
    for ed in g.edges:
        e = PG.edge_residual(ed, truth)
        chi = e @ ed.information @ e
        assert chi > mu if ed is bad else chi < mu
    PG.global_optimization(g, PG.GlobalOptimizationLevenbergMarquardt(), crit, opt)
    assert bad not in g.edges and len(g.edges) == (n - 1) + (n - 1) * (n - 2) // 2 - 1
    assert all(ed.confidence >= opt.edge_prune_threshold for ed in g.edges if ed.uncertain)
    assert bad.confidence < opt.edge_prune_threshold
    assert _objective(g, mu) < crit.min_residual
    _assert_within_truth(g, truth, crit.min_residual)


def test_noisy_graph_against_scipy_least_squares():
    """No uncertain edge: a plain weighted least squares, minimised independently by scipy.optimize.least_squares (tolerances 1e-15)
    over left-multiplied 6-vector updates of the free nodes.
    The solver's rules leave it at most this far above the minimum (H = J^T L J at the end, h_min its smallest eigenvalue; near the
    minimum the objective is the quadratic model, the residuals being small):
    - relative residual increment: the last accepted step lowered F by < eps F.  A step damped by lambda removes, in every
      eigen-direction of H, at least the fraction f = 1 - (lambda / (h_min + lambda))^2 of the gap, so gap <= eps F / f;
    - right term: max |b| < min_right_term, gap ~= b^T H^-1 b <= dim min_right_term^2 / h_min.
    Measured (8 nodes, seed 3): solver 1.599998e-01, SciPy 1.599998e-01 (difference 6.8e-14), permitted 1.6e-07; the run ends
    on the relative residual increment.  (With Open3D's linearised Jacobian the difference was 2.5e-07: see posegraph.py.)"""
    from scipy.optimize import least_squares
    n, rng = 8, np.random.default_rng(3)
    g, _ = _graph(n, rng)
    for ed in g.edges:
        ed.transformation = ed.transformation @ PG.vector6_to_matrix4(rng.normal(scale=1e-2, size=6))
    start = [nd.pose.copy() for nd in g.nodes]
    chol = [np.linalg.cholesky(ed.information) for ed in g.edges]

    def residuals(x):
        poses = [start[0]] + [PG.vector6_to_matrix4(x[6 * i - 6:6 * i]) @ start[i] for i in range(1, n)]
        return np.concatenate([C.T @ PG.edge_residual(ed, poses) for C, ed in zip(chol, g.edges)])

    ref = least_squares(residuals, np.zeros(6 * (n - 1)), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
    f_ref = float(ref.fun @ ref.fun)
    crit, opt = PG.GlobalOptimizationConvergenceCriteria(), PG.GlobalOptimizationOption(reference_node=0)
    trace = []
    PG.global_optimization(g, PG.GlobalOptimizationLevenbergMarquardt(), crit, opt, trace=trace)
    f = _objective(g, opt.preference_loop_closure)
    poses = [nd.pose for nd in g.nodes]
    H, _ = PG.linear_system(g, poses, np.ones(len(g.edges)))
    h_min = np.linalg.eigvalsh(H[6:, 6:])[0]
    ends = [r for r in trace if r["reason"].startswith("end:")]
    assert len(ends) == 2
    lam, reason = ends[0]["lambda"], ends[0]["reason"]
    permitted = {"end:relative_residual_increment": crit.min_relative_residual_increment * f / (1.0 - (lam / (h_min + lam)) ** 2),
                 "end:right_term": 6 * (n - 1) * crit.min_right_term ** 2 / h_min}[reason]
    print(f"solver {f:.6e}  scipy {f_ref:.6e}  difference {f - f_ref:.3e}  permitted {permitted:.3e}  {reason}  steps {len(trace)}")
    assert f_ref > 1e3 * crit.min_residual                          # the graph is noisy: the residual rule cannot end the run
    assert f - f_ref <= permitted
    objs = [r["objective"] for r in trace]
    assert all(b <= a for a, b in zip(objs, objs[1:]))


def test_defaults_and_errors():
    c = PG.GlobalOptimizationConvergenceCriteria()
    assert (c.max_iteration, c.min_relative_increment, c.min_relative_residual_increment, c.min_right_term, c.min_residual,
            c.max_iteration_lm, c.upper_scale_factor, c.lower_scale_factor) == (100, 1e-6, 1e-6, 1e-6, 1e-6, 20, 2.0 / 3.0, 1.0 / 3.0)
    o = PG.GlobalOptimizationOption()
    assert (o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure, o.reference_node) == (0.03, 0.25, 1.0, -1)
    assert np.array_equal(PG.PoseGraphNode().pose, np.eye(4))
    e = PG.PoseGraphEdge(1, 2)
    assert np.array_equal(e.transformation, np.eye(4)) and np.array_equal(e.information, np.eye(6))
    assert (e.source_node_id, e.target_node_id, e.uncertain, e.confidence) == (1, 2, False, 1.0)
    g = PG.PoseGraph()
    assert g.nodes == [] and g.edges == []
    with pytest.raises(NotImplementedError):
        PG.GlobalOptimizationGaussNewton()
    g.nodes = [PG.PoseGraphNode()]
    g.edges = [PG.PoseGraphEdge(0, 3)]
    with pytest.raises(RuntimeError, match="Invalid PoseGraph"):
        PG.global_optimization(g)


def test_open3d_surface_without_a_gpu():
    from kinectpy_amd import o3d, ops
    reg = o3d.pipelines.registration
    for name in ("PoseGraphNode", "PoseGraphEdge", "PoseGraph", "GlobalOptimizationConvergenceCriteria", "GlobalOptimizationOption",
                 "GlobalOptimizationLevenbergMarquardt", "GlobalOptimizationGaussNewton", "global_optimization"):
        assert getattr(reg, name) is getattr(PG, name)
    a = o3d.geometry.PointCloud.__new__(o3d.geometry.PointCloud)           # the distance is checked before a cloud is touched
    for d in (0.0, -1.0):
        with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance"):
            reg.evaluate_registration(a, a, d)
        with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance"):
            reg.get_information_matrix_from_point_clouds(a, a, d, np.eye(4))
        with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance"):
            ops.registration_eval(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), d)
    from kinectpy_amd.preprocessing.registration import execute_multiway_registration      # noqa: F401
    from kinectpy_amd.preprocessing.data import DataProcessor
    assert DataProcessor.in_memory(3).multiway is False and DataProcessor.in_memory(3, multiway=True).multiway is True


def test_posegraph_imports_numpy_only_and_the_product_never_imports_the_oracle():
    src = open(os.path.join(ROOT, "kinectpy_amd", "posegraph.py")).read()
    assert [l for l in src.splitlines() if l.startswith(("import ", "from "))] == ["import numpy as np"]
    for f in ("posegraph.py", "o3d.py", "ops.py", os.path.join("preprocessing", "registration.py"), os.path.join("csrc", "kpx_icp.hip")):
        s = open(os.path.join(ROOT, "kinectpy_amd", f)).read()
        assert "kpx_oracle" not in s and "kpo_" not in s and "from oracle" not in s and "import oracle" not in s, f

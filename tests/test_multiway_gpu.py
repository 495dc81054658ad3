"""GPU suite (-m gpu) for multiway registration: kpx_registration_eval against the restatement in tests/multiway_ref.py, its bit
identity across the three search engines, the Open3D surface, and execute_multiway_registration end to end on synth.sensor_ring
against the same chain through the oracle."""
import numpy as np
import pytest

import multiway_ref as M
from kinectpy_amd import posegraph as PG
from kinectpy_amd.utils import synth

pytestmark = pytest.mark.gpu
TOL_T = 1e-8           # absolute, ICP 4x4 (rotation entries / mm), as test_parity_gpu.py
ENGINES = ["culled", "dense", "dense_fp64"]
# The ICP's own scatter on these rings, in the unit of truth_distance(): the spread (max - min) of the STAR's distance from the
# truth over the three engines and synth.perturb seeds 0-3 of the initial transforms (twelve star calibrations per ring), measured
# on an MI355X at small_xy resolution: ring of 4: distances 130.39 .. 159.62, spread 29.2; ring of 8: 311.33 .. 529.68, spread 218.3
# (the three engines agree to the last digit shown: the spread is the seeds').  See DESIGN.md, "Multiway registration".
STAR_SCATTER = {4: 29.2, 8: 218.3}


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


@pytest.fixture(params=ENGINES)
def engine(request, ops):
    prev = ops.nn_engine(request.param)
    yield request.param
    ops.nn_engine(prev)


def _npy(t):
    return t.cpu().numpy()


def _cloud(base, n, seed):
    return base[np.random.default_rng(seed).choice(len(base), n, replace=False)]


def _block(r):
    return np.concatenate([[r["fitness"], r["inlier_rmse"], float(r["count"])], r["information"].reshape(-1)])


def _cases(base):
    """(name, src, tgt, T, max_dist, kind): kind 'all' / 'some' / 'none' rows pass"""
    Ti = np.linalg.inv(synth.t_star())
    out = []
    for n in (1, 1000, 4097, 30000):
        tgt = _cloud(base, max(n, 1000), 1)
        src0 = _cloud(base, n, 2).astype(np.float64)
        src = (src0 @ Ti[:3, :3].T + Ti[:3, 3] + np.random.default_rng(n).normal(scale=1.0, size=src0.shape)).astype(np.float32)
        out.append((f"aligned{n}", src, tgt, synth.t_star(), 1e4, "all"))
        if n > 1:
            out.append((f"some{n}", src, tgt, synth.t_star(), 12.0, "some"))
            out.append((f"identity{n}", src, tgt, None, 100.0, "some"))
        out.append((f"far{n}", src + np.float32(1e5), tgt, synth.t_star(), 100.0, "none"))
    return out


def _check_eval(r, ref, n):
    assert np.array_equal(_npy(r["idx"]), ref["idx"]) and np.array_equal(_npy(r["d2"]), ref["d2"])
    assert r["count"] == ref["count"] and r["fitness"] == ref["count"] / n
    assert abs(r["inlier_rmse"] - ref["inlier_rmse"]) <= ref["rmse_bound"]
    L = r["information"]
    assert L.shape == (6, 6) and L.dtype == np.float64
    assert (np.abs(L - ref["information"]) <= ref["information_bound"]).all()
    assert np.array_equal(L, L.T) and np.array_equal(L[3:, 3:], ref["count"] * np.eye(3))


def test_registration_eval_matches_restatement(ops, oracle, base_cloud, engine):
    kinds = set()
    for name, src, tgt, T, md, kind in _cases(base_cloud):
        r = ops.registration_eval(src, tgt, md, T, want_corr=True)
        ref = M.registration_eval(oracle, src, tgt, md, T)
        _check_eval(r, ref, len(src))
        passed = int(ref["ok"].sum())
        assert {"all": passed == len(src), "some": 0 < passed < len(src), "none": passed == 0}[kind], (name, passed)
        if kind == "none":
            assert r["inlier_rmse"] == 0.0 and r["fitness"] == 0.0 and not r["information"].any()
        kinds.add(kind)
        assert "idx" not in ops.registration_eval(src, tgt, md, T)
    assert kinds == {"all", "some", "none"}


def test_registration_eval_bit_identical_across_engines_and_runs(ops, base_cloud):
    prev = ops.nn_engine()
    try:
        for name, src, tgt, T, md, kind in _cases(base_cloud):
            blocks = []
            for eng in ENGINES:
                ops.nn_engine(eng)
                for _ in range(2):
                    r = ops.registration_eval(src, tgt, md, T, want_corr=True)
                    blocks.append(_block(r).tobytes() + _npy(r["idx"]).tobytes() + _npy(r["d2"]).tobytes())
            assert len(set(blocks)) == 1, name
    finally:
        ops.nn_engine(prev)


def test_open3d_surface(ops, oracle, base_cloud, engine):
    from kinectpy_amd import o3d
    reg = o3d.pipelines.registration
    src, tgt, T = synth.icp_pair(6000, base_cloud)
    a, b = o3d.geometry.PointCloud(src), o3d.geometry.PointCloud(tgt)
    b.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(70.0, 30))
    with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance"):
        reg.evaluate_registration(a, b, 0.0)
    with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance"):
        reg.get_information_matrix_from_point_clouds(a, b, -1.0, np.eye(4))
    for X, md in ((np.eye(4), 100.0), (T, 8.0)):
        r = ops.registration_eval(src, tgt, md, X, want_corr=True)
        ev = reg.evaluate_registration(a, b, md, X)
        ok = _npy(r["d2"]) < md * md
        assert ev.fitness == r["fitness"] and ev.inlier_rmse == r["inlier_rmse"] and np.array_equal(ev.transformation, X)
        assert np.array_equal(np.asarray(ev.correspondence_set), np.stack([np.flatnonzero(ok), _npy(r["idx"])[ok]], 1))
        assert np.array_equal(reg.get_information_matrix_from_point_clouds(a, b, md, X), r["information"])
    assert np.array_equal(reg.evaluate_registration(a, b, 100.0).transformation, np.eye(4))
    # at the transformation an ICP returned: the loop reported fitness / rmse / correspondences from its search there
    for est in (reg.TransformationEstimationPointToPoint(), reg.TransformationEstimationPointToPlane()):
        res = reg.registration_icp(a, b, 100.0, np.eye(4), est)
        ev = reg.evaluate_registration(a, b, 100.0, res.transformation)
        ref = M.registration_eval(oracle, src, tgt, 100.0, res.transformation)
        assert ev.fitness == res.fitness and np.array_equal(np.asarray(ev.correspondence_set), np.asarray(res.correspondence_set))
        assert abs(ev.inlier_rmse - ref["inlier_rmse"]) <= ref["rmse_bound"] and abs(res.inlier_rmse - ref["inlier_rmse"]) <= ref["rmse_bound"]


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def truth_distance(Ts, truth):
    """one number for a calibration's distance from the truth: the largest, over the subs, of |translation error| (mm) plus
    1000 mm times the rotation error angle (the displacement of a point one metre from the origin)"""
    out = 0.0
    for T, G in zip(Ts, truth):
        D = np.linalg.inv(G) @ T
        ang = np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1))
        out = max(out, np.linalg.norm(D[:3, 3]) + 1000.0 * ang)
    return out


def ring_clouds(oracle, S):
    """the full clouds of sensor_ring(S) at small_xy resolution, as DataProcessor builds them on frame 0 (rgbd_to_pointcloud)"""
    from kinectpy_amd.utils.io import rgbd_to_pointcloud
    xy, depth, rgb, inits, truth = synth.sensor_ring(S, 1, synth.small_xy())
    xyz = [oracle.unproject_u16(depth[0][i], xy) for i in range(S)]
    return [rgbd_to_pointcloud(rgb[0][i], xyz[i]) for i in range(S)], inits, truth, rgb[0], xyz


def _pose_tolerance(g, mu):
    """How far the solved poses may move when every edge transformation moves by <= TOL_T per entry.  At the minimum
    H x = sum_k J_k^T L_k e_k-terms, so to first order dx = -H^-1 sum_k J_k^T L_k de_k.  An entry-wise TOL_T on X moves the
    rotation part of e = vec6(X^-1 P_t^-1 P_s) by <= d_rot = 6 TOL_T and its translation by <= d_tr = 3 TOL_T (1 + 2 r), r the
    largest translation norm in the graph.  With D = diag(d_rot x3, d_tr x3): |dx| <= sqrt(6) sum_k |H^-1 J_k^T L_k D|_2.  H is the
    final system's (the conditioning enters through H^-1; cond(H) is printed).  A pose entry moves by <= |dx| (1 + r); the
    factor 2 covers the second-order term and the information matrices' rounding-level differences."""
    poses = [nd.pose for nd in g.nodes]
    l = PG.line_process(g, poses, mu)
    H, _ = PG.linear_system(g, poses, l)
    Hf = H[6:, 6:]
    r = max([np.linalg.norm(P[:3, 3]) for P in poses] + [np.linalg.norm(ed.transformation[:3, 3]) for ed in g.edges])
    D = np.diag([6 * TOL_T] * 3 + [3 * TOL_T * (1 + 2 * r)] * 3)
    Hinv = np.linalg.inv(Hf)
    total = 0.0
    for k, ed in enumerate(g.edges):
        s, t = ed.source_node_id, ed.target_node_id
        left = PG._inv(ed.transformation) @ PG._inv(poses[t])
        Js = PG._dvec6(left @ poses[s], left @ PG._G @ poses[s]).T
        J = np.zeros((6, 6 * len(poses)))
        J[:, 6 * s:6 * s + 6], J[:, 6 * t:6 * t + 6] = Js, -Js
        total += np.linalg.norm(Hinv @ (l[k] * J[:, 6:].T @ ed.information @ D), 2)
    return 2.0 * np.sqrt(6.0) * total * (1 + r), np.linalg.cond(Hf)


_ring_results = {}


@pytest.mark.parametrize("S", [4, 8])
def test_multiway_end_to_end_against_the_oracle_chain(ops, oracle, engine, S):
    from kinectpy_amd.preprocessing.registration import (execute_multiway_registration, execute_point_to_plane_registration,
                                                         preprocess_point_cloud)
    pcds, inits, truth, _, _ = ring_clouds(oracle, S)
    Ts, g = execute_multiway_registration(pcds, 35, initial_transformations=inits, return_pose_graph=True)
    downs = [preprocess_point_cloud(p, 35, 40, with_fpfh=False)[0] for p in pcds]
    pts, nrm = [_npy(d._pts) for d in downs], [_npy(d._nrm) for d in downs]
    star, edges = M.multiway_chain(oracle, pts, nrm, inits)
    ref_T, ref_g, mu = M.solve_chain(star, edges, 35)
    # the same edges survive, with the same transformations and information matrices
    assert [(e.source_node_id, e.target_node_id, e.uncertain) for e in g.edges] == [(e.source_node_id, e.target_node_id, e.uncertain) for e in ref_g.edges]
    evals = {(s, t): ev for s, t, _, _, ev in edges}
    for e, r in zip(g.edges, ref_g.edges):
        ev = evals[(e.source_node_id, e.target_node_id)]
        assert np.abs(e.transformation - r.transformation).max() < TOL_T
        assert e.information[3, 3] == ev["count"] and (np.abs(e.information - ev["information"]) <= ev["information_bound"]).all()
    all_pairs = [(i, 0) for i in range(1, S)] + [(i, j) for j in range(2, S) for i in range(1, j)]
    kept = {(e.source_node_id, e.target_node_id) for e in g.edges}
    pruned = [p for p in all_pairs if p not in kept]
    tol, cond = _pose_tolerance(ref_g, mu)
    diff = max(np.abs(a - b).max() for a, b in zip(Ts, ref_T))
    assert np.array_equal(g.nodes[0].pose, np.eye(4)) and len(Ts) == S - 1
    star_T = [execute_point_to_plane_registration(pcds[0], pcds[i], inits[i - 1]) for i in range(1, S)]
    for a, b in zip(star_T, star[1:]):
        assert np.abs(a - b).max() < TOL_T
    d_multi, d_star, d_init = truth_distance(Ts, truth), truth_distance(star_T, truth), truth_distance(inits, truth)
    print(f"\nmultiway ring {S} [{engine}]: mu {mu:.4g}  edges {len(all_pairs)}  pruned {pruned}  cond(H) {cond:.3g}  pose diff {diff:.3g} (tol {tol:.3g})"
          f"  distance from truth: init {d_init:.3f}  star {d_star:.3f}  multiway {d_multi:.3f}")
    assert diff <= tol
    # the one assertion against the truth: no further from it than the star by more than the ICP's own scatter
    assert d_multi <= d_star + STAR_SCATTER[S]
    _ring_results[(S, engine)] = Ts


@pytest.mark.parametrize("S", [4])
def test_data_processor_multiway(ops, oracle, engine, S):
    from kinectpy_amd.preprocessing.data import DataProcessor
    from kinectpy_amd.preprocessing.registration import execute_multiway_registration, execute_point_to_plane_registration
    pcds, inits, _, rgb, xyz = ring_clouds(oracle, S)
    dp = DataProcessor.in_memory(S, inits, multiway=True)
    got = dp.find_registration_transforms(pcds[0], pcds[1:])
    want = _ring_results.get((S, engine)) or execute_multiway_registration(pcds, 35, initial_transformations=inits)
    assert len(got) == S - 1 and all(np.array_equal(a, b) for a, b in zip(got, want))
    fused = dp.process_frame(list(rgb), xyz)
    assert len(fused.points) > 100
    star = DataProcessor.in_memory(S, inits).find_registration_transforms(pcds[0], pcds[1:])
    assert all(np.array_equal(a, execute_point_to_plane_registration(pcds[0], pcds[i + 1], inits[i])) for i, a in enumerate(star))
    assert not all(np.array_equal(a, b) for a, b in zip(got, star))

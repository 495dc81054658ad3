"""Drop-in for KinectPy's preprocessing/registration.py (reference lines 7-114)."""
import copy
import inspect

import numpy as np

from .. import o3d


def preprocess_point_cloud(pcd, voxel_size, normals_nn=30, fpfh_nn=100, with_fpfh=True):
    """registration.py:7-21: voxel down-sample, normals (radius 2v), FPFH (radius 5v).  with_fpfh=False skips the
    features (execute_point_to_plane_registration discards them)."""
    pcd_down = pcd.voxel_down_sample(voxel_size)
    pcd_down.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(radius=voxel_size * 2, max_nn=normals_nn))
    pcd_fpfh = None
    if with_fpfh:
        pcd_fpfh = o3d.pipelines.registration.compute_fpfh_feature(
            pcd_down, o3d.geometry.KDTreeSearchParamHybrid(radius=voxel_size * 5, max_nn=fpfh_nn))
    return pcd_down, pcd_fpfh


def prepare_dataset(pcd_master, pcd_sub, voxel_size, normals_nn=40, fpfh_nn=40, with_fpfh=True):
    """registration.py:24-29: source = sub, target = master."""
    source, target = copy.deepcopy(pcd_sub), copy.deepcopy(pcd_master)
    source_down, source_fpfh = preprocess_point_cloud(source, voxel_size, normals_nn, fpfh_nn, with_fpfh)
    target_down, target_fpfh = preprocess_point_cloud(target, voxel_size, normals_nn, fpfh_nn, with_fpfh)
    return source, target, source_down, target_down, source_fpfh, target_fpfh


def _cut_to_keypoints(down, fpfh, keypoints):
    """(cloud, feature) of the ISS keypoints of a down-sampled cloud; `keypoints`: True (default radii) or a dict of
    compute_iss_keypoints' parameters"""
    idx = down._iss_keypoint_indices(**(keypoints if isinstance(keypoints, dict) else {}))
    return down._select(idx), fpfh.select_by_index(idx)


def execute_global_registration(pcd_master, pcd_sub, voxel_size: int = 35, ransac_n_trials: int = 15, seed=None, *, keypoints=None,
                                **extension) -> np.ndarray:
    """registration.py:32-62: ransac_n_trials runs of FPFH feature-matching RANSAC (distance threshold 1.5 v,
    mutual filter, edge-length 0.95 + distance checkers, 250000 iterations, confidence 0.999); the
    transformation of the best fitness is kept (None if every fitness is 0).  The reference recomputes
    prepare_dataset in every trial with identical results; here it is computed once.  seed: base seed of the
    trials (None -> fresh random seeds, the reference's behaviour).
    keypoints: None (the reference: every down-sampled point is matched), True (ISS keypoints with Open3D's default radii, from
    the down-sampled cloud's resolution) or a dict of o3d.geometry.keypoint.compute_iss_keypoints' parameters.  Normals and FPFH are
    still computed on the full down-sampled clouds; points and feature columns are then cut to the keypoints on both sides and the
    RANSAC matches and scores those alone.  If either side has fewer than ransac_n = 3 keypoints, the full clouds are used as if
    keypoints were None.
    method: "ransac" (the reference) or "fgr": ONE Fast Global Registration (o3d...registration_fgr_based_on_feature_matching with
    FastGlobalRegistrationOption(maximum_correspondence_distance=0.5 * voxel_size), as in Open3D's tutorial) on the same clouds and
    features instead of the ransac_n_trials RANSAC runs; `seed` seeds its tuple test; None if its fitness is 0.  (`method` is the one
    keyword `extension` takes: the function's keyword defaults stay those of before.)"""
    method = extension.pop("method", "ransac")
    if extension:
        raise TypeError(f"execute_global_registration() got an unexpected keyword argument {next(iter(extension))!r}")
    if method not in ("ransac", "fgr"):
        raise ValueError(f"execute_global_registration: method must be 'ransac' or 'fgr', not {method!r}")
    best_fitness = 0
    ransac_transformation = None
    reg = o3d.pipelines.registration
    (source, target, source_down, target_down, source_fpfh, target_fpfh) = prepare_dataset(pcd_master, pcd_sub, voxel_size)
    if keypoints is not None and keypoints is not False:
        source_key, source_key_fpfh = _cut_to_keypoints(source_down, source_fpfh, keypoints)
        target_key, target_key_fpfh = _cut_to_keypoints(target_down, target_fpfh, keypoints)
        if min(len(source_key.points), len(target_key.points)) >= 3:
            source_down, source_fpfh, target_down, target_fpfh = source_key, source_key_fpfh, target_key, target_key_fpfh
    if method == "fgr":
        result_fgr = reg.registration_fgr_based_on_feature_matching(
            source_down, target_down, source_fpfh, target_fpfh,
            reg.FastGlobalRegistrationOption(maximum_correspondence_distance=voxel_size * 0.5), seed=seed)
        return result_fgr.transformation if result_fgr.fitness > 0 else None
    distance_threshold = voxel_size * 1.5
    for trial in range(ransac_n_trials):
        result_ransac = reg.registration_ransac_based_on_feature_matching(
            source_down, target_down, source_fpfh, target_fpfh, True, distance_threshold,
            reg.TransformationEstimationPointToPoint(False), 3,
            [reg.CorrespondenceCheckerBasedOnEdgeLength(0.95), reg.CorrespondenceCheckerBasedOnDistance(distance_threshold)],
            reg.RANSACConvergenceCriteria(250000, 0.999), seed=None if seed is None else seed + trial)
        if best_fitness < result_ransac.fitness:
            best_fitness = result_ransac.fitness
            ransac_transformation = result_ransac.transformation
    return ransac_transformation


def execute_point_to_plane_registration(pcd_master, pcd_sub, initial_transformation: np.ndarray,
                                        voxel_size: int = 35, *, kernel=None) -> np.ndarray:
    """registration.py:65-86.  The reference names master `source` and sub `target` and then calls
    prepare_dataset(source, target), which swaps them back: the effective call is
    registration_icp(sub_down, master_down, 100, init, PointToPlane) and the result maps sub -> master.
    kernel: a robust loss of o3d.pipelines.registration (e.g. TukeyLoss(k)) for the ICP; None is the reference's plain L2."""
    source, target = copy.deepcopy(pcd_master), copy.deepcopy(pcd_sub)
    threshold = 100
    _, _, source_down, target_down, _, _ = prepare_dataset(source, target, voxel_size, with_fpfh=False)
    reg = o3d.pipelines.registration.registration_icp(
        source_down, target_down, threshold, initial_transformation,
        o3d.pipelines.registration.TransformationEstimationPointToPlane(kernel))
    return reg.transformation


# Introspection shows the reference's signature, which this drop-in stands for (the host suite compares it parameter
# by parameter): `kernel` is this library's keyword-only extension and is documented in the docstring above.
execute_point_to_plane_registration.__signature__ = inspect.Signature(
    [p for p in inspect.signature(execute_point_to_plane_registration).parameters.values() if p.name != "kernel"])
# likewise `keypoints` and `method` of execute_global_registration
execute_global_registration.__signature__ = inspect.Signature(
    [p for p in inspect.signature(execute_global_registration).parameters.values() if p.name not in ("keypoints", "extension")],
    return_annotation=inspect.signature(execute_global_registration).return_annotation)


def execute_colored_ICP_registration(pcd_master, pcd_sub, initial_transformation):
    """registration.py:89-114, as written there: master is the source, sub the target; three scales (voxel 80 / 40 / 20 with
    50 / 30 / 14 iterations), every scale starts again from `initial_transformation`, the last scale's result is returned."""
    source = copy.deepcopy(pcd_master)
    target = copy.deepcopy(pcd_sub)
    voxel_radius = [80, 40, 20]
    max_iter = [50, 30, 14]
    result_icp = None
    for scale in range(len(max_iter)):
        iters = max_iter[scale]
        radius = voxel_radius[scale]
        source_down = source.voxel_down_sample(radius)
        target_down = target.voxel_down_sample(radius)
        source_down.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(radius=radius * 2, max_nn=30))
        target_down.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(radius=radius * 2, max_nn=30))
        result_icp = o3d.pipelines.registration.registration_colored_icp(
            source_down, target_down, radius, initial_transformation,
            o3d.pipelines.registration.TransformationEstimationForColoredICP(),
            o3d.pipelines.registration.ICPConvergenceCriteria(relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=iters))
    return result_icp.transformation


def execute_multiway_registration(pcds, voxel_size: int = 35, initial_transformations=None, seed=None, preference_loop_closure=None,
                                  edge_prune_threshold: float = 0.25, return_pose_graph: bool = False, kernel=None, keypoints=None,
                                  global_method="ransac"):
    """[O3D] multiway registration of a rig: pcds[0] is the master.  Not in the reference, whose calibration is the star alone
    (data.py:137-147); opt-in through DataProcessor(multiway=True).  -> the sub -> master 4x4 list in the form
    DataProcessor.registration_transformations holds (and the optimised PoseGraph with return_pose_graph).

    1. star edges (i, 0, T_i), certain: the existing chain per sub (execute_global_registration unless an initial transformation
       is given, then the point-to-plane ICP of execute_point_to_plane_registration);
    2. loop edges (i, j, X_ij), 1 <= i < j, uncertain: the same ICP of down-sampled cloud i onto down-sampled cloud j from
       T_j^-1 T_i, all sources of one target in one ops.icp_batch call;
    3. every edge's information matrix from ops.registration_eval at its transformation and the ICP's distance; an edge without
       a single correspondence is left out;
    4. node poses start at T_i; global_optimization with reference_node = 0.
    preference_loop_closure=None: mu = (median correspondence count of the uncertain edges) * voxel_size^2 -- a closure goes when
    it disagrees with the rest by more than about one voxel rms over its matched points ("Multiway registration").
    kernel: a robust loss for every pairwise ICP (star and loop edges); the loop edges then go one by one through ops.icp, as
    ops.icp_batch runs the culled iteration kernels, which take no weights.
    keypoints: passed to every execute_global_registration (None: every down-sampled point is matched).
    global_method: execute_global_registration's `method` ("ransac" or "fgr")."""
    from .. import ops
    reg = o3d.pipelines.registration
    threshold = 100                                                       # execute_point_to_plane_registration's
    S = len(pcds)
    downs = [preprocess_point_cloud(copy.deepcopy(p), voxel_size, 40, with_fpfh=False)[0] for p in pcds]      # prepare_dataset's normals_nn
    star = [np.eye(4)]
    for i in range(1, S):
        if initial_transformations is None:
            init = execute_global_registration(pcds[0], pcds[i], voxel_size, seed=seed, keypoints=keypoints,
                                               **({} if global_method == "ransac" else {"method": global_method}))
            if init is None:
                raise RuntimeError("execute_global_registration found no transformation (every RANSAC fitness was 0)" if global_method == "ransac"
                                   else "execute_global_registration found no transformation (the FGR fitness was 0)")
        else:
            init = initial_transformations[i - 1]
        star.append(reg.registration_icp(downs[i], downs[0], threshold, init, reg.TransformationEstimationPointToPlane(kernel)).transformation)
    edges = [(i, 0, star[i], False) for i in range(1, S)]
    for j in range(2, S):
        Tj_inv = np.linalg.inv(star[j])
        inits = [Tj_inv @ star[i] for i in range(1, j)]
        if kernel is None:
            res = ops.icp_batch([downs[i]._pts for i in range(1, j)], downs[j]._pts, threshold, inits, "p2plane", downs[j]._nrm)
        else:
            res = [ops.icp(downs[i]._pts, downs[j]._pts, threshold, init, "p2plane", downs[j]._nrm, loss=kernel)
                   for i, init in zip(range(1, j), inits)]
        edges += [(i, j, r["transformation"], True) for i, r in zip(range(1, j), res)]
    pose_graph = reg.PoseGraph()
    pose_graph.nodes = [reg.PoseGraphNode(T) for T in star]
    counts = []
    for s, t, X, uncertain in edges:
        ev = ops.registration_eval(downs[s]._pts, downs[t]._pts, threshold, X)
        if ev["count"] == 0:
            continue
        pose_graph.edges.append(reg.PoseGraphEdge(s, t, X, ev["information"], uncertain))
        if uncertain:
            counts.append(ev["count"])
    if preference_loop_closure is None:
        preference_loop_closure = (float(np.median(counts)) if counts else 1.0) * float(voxel_size) ** 2
    reg.global_optimization(pose_graph, reg.GlobalOptimizationLevenbergMarquardt(), reg.GlobalOptimizationConvergenceCriteria(),
                            reg.GlobalOptimizationOption(threshold, edge_prune_threshold, preference_loop_closure, 0))
    out = [nd.pose.copy() for nd in pose_graph.nodes[1:]]
    return (out, pose_graph) if return_pose_graph else out


def estimate_sensor_drift(depths_ref, colors_ref, depths_now, colors_now, intrinsic, masks_ref=None, masks_now=None, option=None, jacobian=None,
                          depth_scale=1.0, depth_trunc=0.0):
    """Has a sensor moved since the rig was calibrated?  The rig is calibrated once, on its first frame set, and those transforms are
    applied to every later frame; a bumped tripod goes unnoticed.  Most of every sensor's own image is static room, so the rigid motion
    between a sensor's reference frame and its current frame IS the sensor's drift: RGB-D odometry of each sensor against itself, all
    S sensors in one compute_rgbd_odometry_batch call.

    depths_*: the S sensors' depth as the pipeline holds it -- uint16 (S, n_px) / (S, H, W), or the int16 XYZ triples (S, n_px, 3)
    whose z column is taken; colors_*: uint8 (S, n_px, 3); intrinsic: a PinholeCameraIntrinsic; masks_*: (S, n_px), nonzero = leave the
    pixel out (the person, who does move); option: an OdometryOption in the data's units (default: millimetres, (30, 0, 4000));
    depth_trunc 0: no truncation.
    -> one dict per sensor: success, transformation (4, 4, reference camera -> current camera), information (6, 6), rotation_deg (the
    angle of R) and translation (the norm of t, data units); a failed sensor reports the identities and zeros."""
    odo = o3d.pipelines.odometry
    option = odo.OdometryOption(depth_diff_max=30.0, depth_min=0.0, depth_max=4000.0) if option is None else option

    def z_of(d):
        if hasattr(d, "cpu"):
            d = d.cpu().numpy()
        d = np.asarray(d)
        if d.dtype == np.int16 and d.ndim == 3 and d.shape[2] == 3:
            d = np.clip(d[:, :, 2], 0, None)
        return np.ascontiguousarray(d).astype(np.uint16).reshape(d.shape[0], -1)

    def mask_of(m):
        return None if m is None else np.ascontiguousarray(np.asarray(m.cpu().numpy() if hasattr(m, "cpu") else m) != 0).astype(np.uint8)

    ok, T, info = odo.compute_rgbd_odometry_batch(z_of(depths_ref), colors_ref, z_of(depths_now), colors_now, intrinsic, None, jacobian, option,
                                                  depth_scale=depth_scale, depth_trunc=depth_trunc if depth_trunc > 0 else np.inf,
                                                  masks_s=mask_of(masks_ref), masks_t=mask_of(masks_now))
    out = []
    for i in range(len(ok)):
        c = np.clip((np.trace(T[i, :3, :3]) - 1.0) / 2.0, -1.0, 1.0)
        out.append({"success": bool(ok[i]), "transformation": T[i], "information": info[i], "rotation_deg": float(np.degrees(np.arccos(c))),
                    "translation": float(np.linalg.norm(T[i, :3, 3]))})
    return out

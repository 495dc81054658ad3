"""Per-operator measurement at BASELINE.json sizes: whole-operator device time from
HIP events on the launch stream, algorithmic bytes / flops per SURVEY 8d, fraction of the roofline.
Writes one JSON line per operator (stdout); profiles/rNN/kernels.json keeps the output.

    python tools/bench_kernels.py [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kinectpy_amd import ops  # noqa: E402
from kinectpy_amd.utils import synth  # noqa: E402

HBM_PEAK = 8000.0      # GB/s spec (6.3 TB/s measured achievable, MI355X_MICROARCH.md)
FP64_MFMA_PEAK = 78.6  # TFLOP/s vendor
N_PX = 576 * 640


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def report(name, ms, nbytes=None, flops=None, **extra):
    row = {"op": name, "ms": round(ms, 4)}
    if nbytes is not None:
        gbs = nbytes / (ms * 1e-3) / 1e9
        row.update(algorithmic_bytes=int(nbytes), GBps=round(gbs, 1), frac_hbm=round(gbs / HBM_PEAK, 4))
    if flops is not None:
        tf = flops / (ms * 1e-3) / 1e12
        row.update(flops=int(flops), TFLOPs=round(tf, 2), frac_fp64_mfma=round(tf / FP64_MFMA_PEAK, 4))
    row.update(extra)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--tsdf", action="store_true", help="only the TSDF integration rows")
    ap.add_argument("--mesh", action="store_true", help="only the mesh clean-up rows")
    ap.add_argument("--raycast", action="store_true", help="only the mesh query rows (RaycastingScene)")
    ap.add_argument("--mesh-checks", action="store_true", help="only the mesh check rows (watertight, orientation, volume, triangle pairs)")
    ap.add_argument("--voxelgrid", action="store_true", help="only the occupancy grid rows")
    ap.add_argument("--odometry", action="store_true", help="only the RGB-D odometry rows")
    ap.add_argument("--orient", action="store_true", help="only the normal orientation / EMST rows")
    ap.add_argument("--pointnet", action="store_true", help="only the PointNet forward rows (fused against eval-mode torch modules)")
    ap.add_argument("--pointnet-train", action="store_true", help="only the PointNet training step rows (against train-mode torch modules with torch.optim.Adam)")
    ap.add_argument("--sensor", action="store_true", help="only the sensor calibration rows (xy_table, color_to_depth, depth_to_color, color_to_depth with the occlusion test, undistort_map, remap, remap_depth)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.sensor:
        return sensor_rows(dev, a.quick)
    if a.pointnet_train:
        return pointnet_train_rows(dev, a.quick)
    if a.pointnet:
        return pointnet_rows(dev, a.quick)
    if a.tsdf:
        return tsdf_rows(dev, a.quick)
    if a.mesh:
        return mesh_rows(dev, a.quick)
    if a.raycast:
        return raycast_rows(dev, a.quick)
    if a.mesh_checks:
        return mesh_check_rows(dev, a.quick)
    if a.voxelgrid:
        return voxelgrid_rows(dev, a.quick)
    if a.odometry:
        return odometry_rows(dev, a.quick)
    if a.orient:
        return orient_rows(dev, a.quick)
    F = 64 if a.quick else 256
    xy = synth.xy_table()
    base_d, person = synth.render_depth(xy=xy, return_person=True)
    rgb1 = synth.mask_rgb(person)
    depth = torch.as_tensor(np.tile(base_d, (F, 1))).to(dev)
    rgb = torch.as_tensor(np.tile(rgb1, (F, 1, 1))).to(dev)
    xyd = torch.as_tensor(xy).to(dev)

    # ---- extract (config 1, batched so the working set exceeds the 256 MiB Infinity Cache)
    ms, xyz = timed(lambda: ops.unproject_u16(depth, xyd, F))
    report("unproject_u16 (a1)", ms, F * N_PX * 8, frames=F)
    ms, res = timed(lambda: ops.depth_to_cloud(depth, xyd, None, F, False, False, sync=False))
    kept = int(res[3].sum().item())
    report("depth_to_cloud no colour (a1+a3)", ms, F * N_PX * 2 + kept * 12, frames=F, kept=kept)
    ms, res = timed(lambda: ops.depth_to_cloud(depth, xyd, rgb, F, True, True, sync=False))
    kept = int(res[3].sum().item())
    report("depth_to_cloud mask+gate+colour (a1+a3+a4)", ms, F * N_PX * 5 + kept * 24, frames=F, kept=kept)
    ms, res = timed(lambda: ops.rgbd_compact(xyz, rgb, F, True, True, want_idx=False, sync=False))
    kept = int(res[3].sum().item())
    report("rgbd_compact from int16 XYZ (a3+a4)", ms, F * N_PX * 9 + kept * 24, frames=F, kept=kept)
    del depth, rgb, xyz, res

    # ---- container ops
    n_big = 16_000_000 if a.quick else 64_000_000
    big = torch.rand((n_big, 3), device=dev) * 3000
    T = synth.t_star()
    ms, out = timed(lambda: ops.transform(big, T, out=big))
    report("transform (a17)", ms, n_big * 24, points=n_big)
    idx = torch.randperm(n_big, device=dev)[: n_big // 2].to(torch.int32).sort().values
    # (two rows: bench.py's roofline_targets times the gather alone -- an index list the caller vouches for, `trusted=True`; the default
    # call first validates the list on the device, Open3D's SelectByIndex semantics for arbitrary lists: range check, duplicates, order --
    # which is the 0.07-of-peak figure profiles/r03/kernels.json showed beside bench.py's 0.45)
    ms, _ = timed(lambda: ops.select_by_index([big], idx, trusted=True))
    report("select_by_index gather (trusted ascending list: what bench.py times)", ms, n_big // 2 * (12 + 12 + 4), points=n_big // 2)
    ms, _ = timed(lambda: ops.select_by_index([big], idx))
    report("select_by_index with the list validated on the device (the default call)", ms, n_big // 2 * (12 + 12 + 4), points=n_big // 2)
    ms, hs = timed(lambda: ops.halfspace_select(big, [0.1, -0.9, 0.2, 300.0]))
    report("halfspace_select (a19)", ms, n_big * 12 + int(hs.shape[0]) * 4, points=n_big)
    ms, (lo_, up_) = timed(lambda: ops.slab_split(big, 200.0))
    report("slab_split max(y)-200 (a18: bbox pass + one selection pass feeding both lists)", ms, n_big * 12 + n_big * 4, points=n_big,
           lower=int(lo_.shape[0]))
    del big, idx, out

    # ---- filter chain (config 3)
    c3 = torch.as_tensor(synth.filter_cloud(1_000_000)).to(dev)
    col = torch.rand_like(c3)
    ms, (vp, vc, _) = timed(lambda: ops.voxel_downsample(c3, 10.0, col))
    report("voxel_down_sample 1M, 10 mm, colours (a7)", ms, 24 * c3.shape[0] + 24 * vp.shape[0], n=int(c3.shape[0]), m=int(vp.shape[0]))
    ops.prof_begin(64)
    ms, (keep, stats, _) = timed(lambda: ops.sor(vp, 20, 2.0), reps=3, warm=1)
    pk = ops.prof_end()["sor_knn"]
    report("remove_statistical_outlier k=20 (a8)", ms, 12 * vp.shape[0] + 16 * keep.shape[0], n=int(vp.shape[0]), kept=int(keep.shape[0]),
           knn_kernel_ms=round(pk[0] / max(pk[1], 1), 3))
    ms, (keep200, _, _) = timed(lambda: ops.sor(vp[:100000].contiguous(), 200, 3.0), reps=2, warm=1)
    report("remove_statistical_outlier k=200 on 100k (filter_outliers default)", ms, 12 * 100000 + 16 * keep200.shape[0], n=100000)
    cloud = vp[keep.long()].contiguous()
    lo, up = ops.slab_split(cloud, 200.0)
    floor = cloud[lo.long()].contiguous()
    ops.prof_begin(64)
    ms, (plane, inl) = timed(lambda: ops.segment_plane(floor, 30.0, 30, 2000, seed=7), reps=3, warm=1)
    pk = ops.prof_end()["plane_score"]
    report("segment_plane 30/30/2000 (a21)", ms, 12 * floor.shape[0] * 2 + 4 * inl.shape[0], flops=None, n=int(floor.shape[0]),
           inliers=int(inl.shape[0]), score_kernel_ms=round(pk[0] / max(pk[1], 1), 3), score_GFLOPs=round(2000 * floor.shape[0] * 8 / (pk[0] / max(pk[1], 1) * 1e-3) / 1e9, 1))
    ms, nrm = timed(lambda: ops.estimate_normals(vp[:100000].contiguous(), 70.0, 40), reps=3, warm=1)
    report("estimate_normals r=70 nn=40 on 100k (a11)", ms, 24 * 100000, n=100000)

    # ---- radius-neighbourhood operators on the frame cloud (config 1's cloud, frame-typical radius)
    fc = torch.as_tensor(synth.frame_cloud()).to(dev)
    ms, (lab, nc) = timed(lambda: ops.cluster_dbscan(fc, 20.0, 10), reps=5, warm=2)
    report("cluster_dbscan eps=20 min_points=10 on the frame cloud", ms, n=int(fc.shape[0]), clusters=int(nc.item()),
           noise=int((lab < 0).sum().item()))
    ms, kr = timed(lambda: ops.remove_radius_outlier(fc, 10, 20.0), reps=5, warm=2)
    report("remove_radius_outlier nb_points=10 radius=20 on the frame cloud", ms, n=int(fc.shape[0]), kept=int(kr.shape[0]))
    # ISS keypoints with Open3D's default radii (6 x / 4 x the cloud's resolution) on the same cloud: the passes alone, then the whole call
    res = float(ops.model_resolution(fc).item())
    ms, sal = timed(lambda: ops.iss_saliency(fc, 6.0 * res), reps=5, warm=2)
    report("iss_saliency salient_radius=6 x resolution on the frame cloud", ms, n=int(fc.shape[0]), resolution=round(res, 3),
           nonzero=int((sal != 0).sum().item()))
    ms, kp = timed(lambda: ops.iss_nonmax(fc, sal, 4.0 * res), reps=5, warm=2)
    report("iss_nonmax non_max_radius=4 x resolution on the frame cloud", ms, n=int(fc.shape[0]), keypoints=int(kp.shape[0]))
    ms, _ = timed(lambda: ops.model_resolution(fc), reps=5, warm=2)
    report("model_resolution on the frame cloud", ms, n=int(fc.shape[0]))
    ms, kp = timed(lambda: ops.iss_keypoints(fc), reps=5, warm=2)
    report("iss_keypoints default radii on the frame cloud (resolution + both passes on one grid)", ms, n=int(fc.shape[0]), keypoints=int(kp.shape[0]))

    # ---- neighbour search (KDTreeFlann) on the frame cloud: index build, self-query knn, the hybrid search of the bench's
    # estimate_normals setting beside estimate_normals itself (the same selection plus covariance and eigen-solve), one radius search at
    # DBSCAN's eps, and queries far outside the cloud
    nfc = int(fc.shape[0])
    ms, sidx = timed(lambda: ops.search_index(fc), reps=20, warm=2)
    report("search_index on the frame cloud", ms, n=nfc)
    for k in (1, 8, 30):
        ms, _ = timed(lambda: ops.search_knn(sidx, fc, k), reps=20, warm=2)
        report(f"search_knn k={k}, self-query on the frame cloud", ms, n=nfc, m=nfc)
    ms, _ = timed(lambda: ops.search_hybrid(sidx, fc, 70.0, 40), reps=20, warm=2)
    report("search_hybrid r=70 max_nn=40, self-query on the frame cloud", ms, n=nfc, m=nfc)
    ms, _ = timed(lambda: ops.estimate_normals(fc, 70.0, 40), reps=20, warm=2)
    report("estimate_normals r=70 max_nn=40 on the frame cloud (the yardstick of search_hybrid)", ms, n=nfc)
    ms, (soff, _, _) = timed(lambda: ops.search_radius(sidx, fc, 20.0), reps=20, warm=2)
    report("search_radius r=20, self-query on the frame cloud (count, host read of the total, fill, segment sort)", ms, n=nfc, m=nfc,
           entries=int(soff[-1].item()))
    bb = ops.bounds(fc).cpu().numpy()
    farq = bb[3:] + (bb[3:] - bb[:3]) * np.random.default_rng(0).uniform(5.0, 100.0, (32, 3))
    ms, _ = timed(lambda: ops.search_knn(sidx, farq, 8), reps=20, warm=2)
    report("search_knn k=8, 32 queries 5-100 box lengths outside the frame cloud", ms, n=nfc, m=32)

    # ---- farthest-point sampling (the PointNet input): the chain on the frame cloud and on 30k points, the block form on 19456 points
    # and on a batch of 64 x 30k (one launch)
    for k in (1024, 4096):
        ms, _ = timed(lambda: ops.farthest_point_sample(fc, k, 0, True), reps=20, warm=2)
        report(f"farthest_point_sample k={k} on the frame cloud (chain)", ms, n=int(fc.shape[0]), us_per_sample=round(1e3 * ms / k, 3))
    c30 = fc[torch.as_tensor(np.random.default_rng(0).choice(int(fc.shape[0]), 30000, replace=False)).to(dev)].contiguous()
    ms, _ = timed(lambda: ops.farthest_point_sample(c30, 2048, 0, True), reps=20, warm=2)
    report("farthest_point_sample k=2048 on 30k points (chain: above KPX_FPS_BLOCK_MAX_N)", ms, n=30000, us_per_sample=round(1e3 * ms / 2048, 3))
    c19 = c30[:19456].contiguous()
    ms, _ = timed(lambda: ops.farthest_point_sample(c19, 2048, 0, True), reps=20, warm=2)
    report("farthest_point_sample k=2048 on 19456 points (block, every point on chip)", ms, n=19456, us_per_sample=round(1e3 * ms / 2048, 3))
    b64 = [fc[torch.as_tensor(np.random.default_rng(s).choice(int(fc.shape[0]), 30000, replace=False)).to(dev)].contiguous() for s in range(64)]
    ms, _ = timed(lambda: ops.farthest_point_sample_batch(b64, 2048, 0), reps=20, warm=2)
    report("farthest_point_sample_batch 64 x 30k, k=2048 (block, one launch)", ms, n=30000, count=64,
           us_per_sample=round(1e3 * ms / 2048, 3), us_per_cloud_sample=round(1e3 * ms / 2048 / 64, 4))

    # ---- config 3 as a whole: filter_outliers(voxel 10, k 20, ratio 2) + floor removal (floor_removal.py:61-73), host wall time
    from kinectpy_amd.geometry import PointCloud as _PC
    from kinectpy_amd.floor_removal import remove_floor
    from kinectpy_amd.preprocessing.filtering import filter_outliers
    import time as _time

    def chain():
        pc = _PC(c3)
        f = filter_outliers(pc, 20, 2.0, 10.0)
        return remove_floor(f, seed=7)
    chain(); torch.cuda.synchronize(); t0 = _time.perf_counter()
    outc = chain(); torch.cuda.synchronize()
    report("config 3 chain: voxel 10 + SOR(20,2) + slab + segment_plane + SOR(50,0.3) on 1M points (host wall time)",
           (_time.perf_counter() - t0) * 1e3, n_in=int(c3.shape[0]), n_out=int(len(outc.points)))

    # ---- global registration (rows a11-a13) on two cluttered views, voxel 35
    xy2, ex = synth.xy_table(), synth.clutter()
    views = []
    for i, seed in ((0, 100), (1, 101)):
        dep = synth.render_depth(synth.camera_pose(i, 16), seed=seed, xy=xy2, extra=ex)
        pcl = ops.depth_to_cloud(dep, xy2, None, 1, False, False)[0][0]
        views.append(ops.voxel_downsample(pcl, 35.0)[0])
    nrm = [ops.estimate_normals(v, 70.0, 40) for v in views]
    ms, f0 = timed(lambda: ops.fpfh(views[0], nrm[0], 175.0, 40), reps=3, warm=1)
    report("compute_fpfh_feature r=175 nn=40 (a11)", ms, n=int(views[0].shape[0]))
    f1 = ops.fpfh(views[1], nrm[1], 175.0, 40)
    ms, _ = timed(lambda: ops.feature_nn(f1, f0), reps=3, warm=1)
    report("feature_nn 33-D (a13 matching; fp64 MFMA, K = 36 augmented form)", ms, flops=2.0 * 36 * f1.shape[0] * f0.shape[0], na=int(f1.shape[0]),
           nb=int(f0.shape[0]))
    corr = ops.feature_correspondences(f1, f0, True, 3)
    ms, r = timed(lambda: ops.ransac_corres(views[1], views[0], corr, 52.5, 3, 0.95, 250000, 0.999, 1), reps=2, warm=1)
    report("ransac feature matching 250k it (a13)", ms, corres=int(len(corr)), iterations=r["iterations"], validations=r["validations"],
           fitness=round(r["fitness"], 4))

    # Fast Global Registration on the mutual correspondences of the same pair (HIP events, median of 20)
    mutual = ops.feature_correspondences(f1, f0, True, ransac_n=0)
    ms, tup = timed(lambda: ops.fgr_tuple_test(views[1], views[0], mutual, 0.95, 1000, 1), reps=20, warm=2)
    report("fgr_tuple_test scale 0.95, 1000 tuples", ms, corres=int(len(mutual)), tuples=int(len(tup) // 3))
    ms, r = timed(lambda: ops.fgr_optimize(views[1], views[0], tup, maximum_correspondence_distance=17.5), reps=20, warm=2)
    report("fgr_optimize 64 rounds, one launch", ms, corres=int(len(tup)), failed_solves=r["failed_solves"], par=r["par"])

    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.registration import execute_global_registration
    import time
    pcs = []
    for i, seed in ((0, 100), (1, 101)):
        dep = synth.render_depth(synth.camera_pose(i, 16), seed=seed, xy=xy2, extra=ex)
        pcs.append(PointCloud(ops.depth_to_cloud(dep, xy2, None, 1, False, False)[0][0]))
    execute_global_registration(pcs[0], pcs[1], 35, 15, seed=1)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        Tg = execute_global_registration(pcs[0], pcs[1], 35, 15, seed=1)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    report("execute_global_registration voxel 35, 15 trials x 250k it (registration.py:32-62, host wall time, median of 3)", float(np.median(walls)),
           n_master=int(len(pcs[0].points)), n_sub=int(len(pcs[1].points)), found=Tg is not None)

    execute_global_registration(pcs[0], pcs[1], 35, seed=1, method="fgr")
    walls = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        Tf = execute_global_registration(pcs[0], pcs[1], 35, seed=1, method="fgr")
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    report("execute_global_registration voxel 35, method='fgr' (one FGR; host wall time, median of 3)", float(np.median(walls)),
           n_master=int(len(pcs[0].points)), n_sub=int(len(pcs[1].points)), found=Tf is not None)

    # ---- sampler / normaliser
    fused = torch.as_tensor(synth.filter_cloud(260_000)).to(dev)
    ms, _ = timed(lambda: ops.sample_points(fused, 4096, 7))
    report("select_points_randomly 260k -> 4096 (utils/processing.py:259-275)", ms, nbytes=12 * 4096 + 12 * 4096 + 4 * 4096, n=260_000)
    rng = np.random.default_rng(0)
    host = synth.filter_cloud(260_000)
    for B in (1, 32, 256):
        xb = torch.as_tensor(np.stack([host[rng.choice(len(host), 4096, replace=False)] for _ in range(B)]).astype(np.float64)).to(dev)
        ms, (obb, _) = timed(lambda: ops.obb_batch(xb, check=False))
        v = obb[:, 15].cpu().numpy()
        report(f"get_oriented_bounding_box, batch of {B} x 4096 points f64 (utils/normalization.py:38-42)", ms, clouds=B,
               ms_per_cloud=round(ms / B, 4), hull_vertices_mean=float(v.mean()), wraps_mean=float(2 * v.mean() - 4))
        if B == 256:
            yb = torch.as_tensor(rng.normal(size=(B, 32, 3))).to(dev)
            from kinectpy_amd.utils.normalization import OrientedBoundingBox
            M = OrientedBoundingBox.get_rotation_matrix_from_yxz([0, 0, np.pi / 2])
            ms, _ = timed(lambda: ops.normalize_batch(xb, obb, ops.NORM_OBB_ROT_TRANS, M))
            report("obb_rotation_translation_batch apply, 256 x 4096 points f64 (utils/normalization.py:67-97)", ms, nbytes=2 * 24 * B * 4096)
    ms, (obb, _) = timed(lambda: ops.obb_batch(fused, check=False), reps=3, warm=1)
    report("get_oriented_bounding_box, one 260k-point cloud f32", ms, hull_vertices=float(obb[0, 15]))

    # ---- registration (config 2)
    def sweep(prof):
        """the sweep kernel that ran (culled by default, dense with KPX_NN_ENGINE=dense): avg ms, TFLOP/s issued"""
        for name in ("nn_local", "nn_mfma", "nn_screen"):
            ms_k, cnt, work = prof[name]
            if cnt:
                return {"sweep_kernel": name, "sweep_kernel_ms": round(ms_k / cnt, 4), "sweep_launches": cnt,
                        "sweep_TFLOPs_issued": round(work / ms_k / 1e9, 2), "sweep_flops_per_launch": int(work / cnt)}
        return {}

    src, tgt, _ = synth.icp_pair(100_000)
    s, t = torch.as_tensor(src).to(dev), torch.as_tensor(tgt).to(dev)
    dense = 8.0 * len(src) * len(tgt)
    ops.prof_begin(256)
    ms, _ = timed(lambda: ops.nn_search(s, t, np.eye(4)), reps=5, warm=1)
    report("nn_search 100k x 100k, cold", ms, dense_equivalent_flops=int(dense), **sweep(ops.prof_end()))
    ms_eval, r = timed(lambda: ops.registration_eval(s, t, 100.0, np.eye(4)), reps=5, warm=1)
    report("registration_eval 100k x 100k (evaluate_registration + information matrix: nn_search + one reduction)", ms_eval,
           nn_search_ms=round(ms, 4), fitness=round(r["fitness"], 5), count=r["count"])
    ops.prof_begin(256)
    ms, r = timed(lambda: ops.icp(s, t, 100.0, None, "p2p", None, 30), reps=5, warm=1)
    report("registration_icp p2p 100k x 100k, 30 it (a16, config 2)", ms, iterations=r["iterations"], fitness=round(r["fitness"], 5),
           ms_per_iteration=round(ms / (r["iterations"] + 1), 4), dense_equivalent_flops=int(dense * (r["iterations"] + 1)),
           **sweep(ops.prof_end()))
    tn = ops.estimate_normals(t, 70.0, 40)
    ops.prof_begin(256)
    ms, r = timed(lambda: ops.icp(s, t, 100.0, None, "p2plane", tn, 30), reps=5, warm=1)
    report("registration_icp p2plane 100k x 100k (a14)", ms, iterations=r["iterations"], fitness=round(r["fitness"], 5),
           ms_per_iteration=round(ms / (r["iterations"] + 1), 4), dense_equivalent_flops=int(dense * (r["iterations"] + 1)),
           **sweep(ops.prof_end()))
    # generalized ICP: covariances from the same target normals (and the source's, estimated alike), built outside the timing
    tc, sc = ops.gicp_covariances(tn), ops.gicp_covariances(ops.estimate_normals(s, 70.0, 40))
    ops.prof_begin(256)
    ms, r = timed(lambda: ops.generalized_icp(s, sc, t, tc, 100.0, None, 30), reps=5, warm=1)
    report("registration_generalized_icp 100k x 100k", ms, iterations=r["iterations"], fitness=round(r["fitness"], 5),
           ms_per_iteration=round(ms / (r["iterations"] + 1), 4), dense_equivalent_flops=int(dense * (r["iterations"] + 1)),
           **sweep(ops.prof_end()))
    tsdf_rows(dev, a.quick)
    mesh_rows(dev, a.quick)
    raycast_rows(dev, a.quick)
    mesh_check_rows(dev, a.quick)
    voxelgrid_rows(dev, a.quick)
    odometry_rows(dev, a.quick)


def tsdf_rows(dev, quick):
    """TSDF integration of S = 4 full-size ring frames: the batch form against four calls with one image each, and
    the extraction.  Resolution 256 (128 MiB of tsdf + weight: cache-resident) and 512 (1 GiB: past the Infinity Cache).  Algorithmic
    traffic: 16 B per updated voxel (40 B with colours) -- counted per call, so the four single-image calls move the volume up to
    four times -- plus the images."""
    S = 4
    _, depth, rgb, _, _ = synth.sensor_ring(S, 1)
    depth_d = [torch.as_tensor(depth[0, s]).to(dev) for s in range(S)]
    rgb_d = [torch.as_tensor(rgb[0, s]).to(dev) for s in range(S)]
    extr = np.stack([np.linalg.inv(synth.camera_pose(g, S)) for g in range(S)])
    K, origin, length = (synth.FX, synth.FY, synth.CX, synth.CY), (-1000.0, -1100.0, -1000.0), 2000.0
    for res in ((256,) if quick else (256, 512)):
        vl = length / res
        for colour in (False, True):
            vol = torch.zeros((res ** 3, 2), dtype=torch.float32, device=dev)
            col = torch.zeros((res ** 3, 3), dtype=torch.float32, device=dev) if colour else None
            batch = lambda: ops.tsdf_integrate(vol, col, res, vl, origin, 4 * vl, depth_d, rgb_d, synth.W, synth.H, K, extr, 1.0, 6000.0)
            batch()
            w = vol[:, 1]
            any_upd, sum_upd = int((w > 0).sum().item()), int(w.sum().item())
            per_voxel, images = (40 if colour else 16), S * N_PX * (5 if colour else 2)
            tag = f"res {res}, {S} x 640x576 u16" + (", RGB8" if colour else "")
            ms, _ = timed(batch)
            report(f"tsdf_integrate batch ({tag})", ms, per_voxel * any_upd + images, voxels=res ** 3, updated=any_upd)

            def one_by_one():
                for s in range(S):
                    ops.tsdf_integrate(vol, col, res, vl, origin, 4 * vl, depth_d[s:s + 1], rgb_d[s:s + 1], synth.W, synth.H, K, extr[s:s + 1], 1.0, 6000.0)
            ms, _ = timed(one_by_one)
            report(f"tsdf_integrate {S} calls of one image ({tag})", ms, per_voxel * sum_upd + images, voxels=res ** 3, updated=sum_upd)
            ops.tsdf_reset(vol, col)
            batch()
            ms, (pts, _, _) = timed(lambda: ops.tsdf_extract(vol, col, res, vl, origin, "surface"))
            report(f"tsdf extract_point_cloud ({tag}; count + scan + host read + fill)", ms, 8 * res ** 3 + int(pts.shape[0]) * (36 if colour else 24),
                   points=int(pts.shape[0]))
            # marching cubes: the code sweep reads the volume (8 B / voxel) and writes a byte, the count sweep reads the bytes and writes
            # the group records (0.5 B), the fill sweep reads both: 12 B / voxel, plus the mesh
            ms, (vert, _, tri) = timed(lambda: ops.tsdf_extract_mesh(vol, col, res, vl, origin))
            nv, nt = int(vert.shape[0]), int(tri.shape[0])
            report(f"tsdf extract_triangle_mesh ({tag}; codes + count + scans + host read + fill)", ms, 12 * res ** 3 + nv * (24 if colour else 12) + nt * 12,
                   vertices=nv, triangles=nt)
            ms, _ = timed(lambda: ops.mesh_normals(vert, tri))
            report(f"mesh compute_vertex_normals ({tag}; triangle normals + sort of 3 T pairs + vertex sums)", ms, nv * 24 + nt * 24, vertices=nv, triangles=nt)
            del vert, tri
            if not colour:
                ms, (vp, _, _) = timed(lambda: ops.tsdf_extract(vol, col, res, vl, origin, "voxels"))
                report(f"tsdf extract_voxel_point_cloud ({tag})", ms, 8 * res ** 3 + int(vp.shape[0]) * 24, points=int(vp.shape[0]))
            del vol, col
    tsdf_blocks_rows(dev, quick, depth[0], rgb[0], extr, K)


def tsdf_blocks_rows(dev, quick, depth, rgb, extr, K):
    """ScalableTSDFVolume on the same four frames next to the uniform rows above: R = 16, stride 4, the voxel length
    of the uniform row of that resolution.  depth_trunc 2600 keeps the subject (what the uniform 2 m box holds), 6000 the whole room
    (blocks over the walls too: where the block form loses its advantage).  "res 64" is the small case where the touch's sort and the
    host read-backs cost more than a pass over the whole uniform volume.  Bytes: 8 (20 with colours) per voxel of the blocks held for an
    integration (one read, one write), 8 per voxel for the clouds, 12 for the mesh -- of the blocks, not of a box."""
    from kinectpy_amd.integration import ScalableTSDFVolume, TSDFVolumeColorType, UniformTSDFVolume
    intr = type("Intrinsic", (), {"width": synth.W, "height": synth.H, "intrinsic_matrix": np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])})()
    depths, colors = torch.as_tensor(np.ascontiguousarray(depth)).to(dev), torch.as_tensor(np.ascontiguousarray(rgb)).to(dev)
    for res, trunc in ((64, 2600.0), (256, 2600.0)) + (() if quick else ((512, 2600.0), (512, 6000.0))):
        vl = 2000.0 / res
        for colour in (False, True):
            ct = TSDFVolumeColorType.RGB8 if colour else TSDFVolumeColorType.NoColor
            vol = ScalableTSDFVolume(vl, 4 * vl, ct, 16, 4)
            run = lambda: vol.integrate_frames(depths, colors if colour else None, intr, extr, 1.0, trunc)
            run()
            blocks = vol.volume_unit_count()
            nvox = blocks * 16 ** 3
            held = nvox * (20 if colour else 8)
            tag = f"vl 2000/{res}, R 16, stride 4, trunc {trunc:g}" + (", RGB8" if colour else "")

            def fresh():
                vol.reset()
                run()
            ms, _ = timed(fresh)
            report(f"scalable integrate_frames into an empty volume ({tag}; touch + host read + insert + integrate)", ms, 2 * held, blocks=blocks, bytes_held=held)
            ms, _ = timed(run)
            report(f"scalable integrate_frames into existing blocks ({tag}; touch + host read + integrate)", ms, 2 * held, blocks=blocks, bytes_held=held)
            vol.reset()
            run()
            ms, pc = timed(vol.extract_point_cloud)
            report(f"scalable extract_point_cloud ({tag})", ms, 8 * nvox, points=int(pc._pts.shape[0]), blocks=blocks)
            ms, m = timed(vol.extract_triangle_mesh)
            report(f"scalable extract_triangle_mesh ({tag})", ms, 12 * nvox, vertices=int(m._vert.shape[0]), triangles=int(m._tri.shape[0]), blocks=blocks)
            if not colour:
                ms, vc = timed(vol.extract_voxel_point_cloud)
                report(f"scalable extract_voxel_point_cloud ({tag})", ms, 8 * nvox, points=int(vc._pts.shape[0]), blocks=blocks)
            del vol
            if res == 64:                                   # the uniform volume of the same voxel length, which the rows above do not hold
                uni = UniformTSDFVolume(2000.0, res, 4 * vl, ct, (-1000.0, -1100.0, -1000.0))
                urun = lambda: uni.integrate_frames(depths, colors if colour else None, intr, extr, 1.0, 6000.0)
                urun()
                ms, _ = timed(urun)
                report(f"uniform integrate_frames (res {res}" + (", RGB8)" if colour else ")"), ms, res ** 3 * (40 if colour else 16), voxels=res ** 3)
                ms, pc = timed(uni.extract_point_cloud)
                report(f"uniform extract_point_cloud (res {res}" + (", RGB8)" if colour else ")"), ms, 8 * res ** 3, points=int(pc._pts.shape[0]))
                ms, m = timed(uni.extract_triangle_mesh)
                report(f"uniform extract_triangle_mesh (res {res}" + (", RGB8)" if colour else ")"), ms, 12 * res ** 3, vertices=int(m._vert.shape[0]))
                del uni


def mesh_rows(dev, quick):
    """The clean-up path on the mesh of the fused ring volume (resolution 512, 256 with --quick), each operator
    whole: launches, sorts and its host read.  Algorithmic traffic, V vertices, T triangles, E adjacency entries:
      adjacency   12 T read, 4 (V + 1) + 4 E written
      clusters    12 T + 12 V read (indices, then the vertices for the areas), 4 T + 12 C written
      Taubin x10  20 steps, each 24 V read and 24 V written in fp64 plus the 4 E + 4 V of the CSR; 12 V in and out at the ends
      sampling    12 T + 12 V read for the areas, 12 N written (the corner gathers of N points hit cache)"""
    S = 4
    _, depth, _, _, _ = synth.sensor_ring(S, 1)
    depth_d = [torch.as_tensor(depth[0, s]).to(dev) for s in range(S)]
    extr = np.stack([np.linalg.inv(synth.camera_pose(g, S)) for g in range(S)])
    K, origin, length = (synth.FX, synth.FY, synth.CX, synth.CY), (-1000.0, -1100.0, -1000.0), 2000.0
    res = 256 if quick else 512
    vl = length / res
    vol = torch.zeros((res ** 3, 2), dtype=torch.float32, device=dev)
    ops.tsdf_integrate(vol, None, res, vl, origin, 4 * vl, depth_d, None, synth.W, synth.H, K, extr, 1.0, 6000.0)
    vert, _, tri = ops.tsdf_extract_mesh(vol, None, res, vl, origin)
    del vol
    nv, nt = int(vert.shape[0]), int(tri.shape[0])
    tag = f"ring mesh of res {res}"
    ms, (_, nb) = timed(lambda: ops.mesh_adjacency(vert, tri))
    ne = int(nb.shape[0])
    report(f"mesh compute_adjacency_list ({tag}; keys + sort of 6 T pairs + unique + offsets + host read)", ms, 12 * nt + 4 * (nv + 1) + 4 * ne, vertices=nv,
           triangles=nt, entries=ne)
    ms, (_, num, _) = timed(lambda: ops.mesh_cluster_triangles(vert, tri))
    nc = int(num.shape[0])
    report(f"mesh cluster_connected_triangles ({tag}; sort of 3 T edges + union-find + rank + sort by cluster + area chain + host read)", ms,
           12 * nt + 12 * nv + 4 * nt + 12 * nc, vertices=nv, triangles=nt, clusters=nc)
    ms, _ = timed(lambda: ops.mesh_smooth(vert, tri, "taubin", 10))
    report(f"mesh filter_smooth_taubin x10 ({tag}; adjacency + 20 steps)", ms, 12 * nt + 4 * (nv + 1) + 4 * ne + 20 * (48 * nv + 4 * ne + 4 * nv) + 24 * nv,
           vertices=nv, triangles=nt)
    ms, _ = timed(lambda: ops.mesh_sample_points(vert, tri, 100000))
    report(f"mesh sample_points_uniformly 100k ({tag}; area chain + split + points + host read)", ms, 12 * nt + 12 * nv + 12 * 100000, vertices=nv,
           triangles=nt)


def raycast_rows(dev, quick):
    """Mesh queries on the mesh of the fused ring volume (resolution 512, 256 with --quick), moved into the master's
    frame: the scene build, the depth images of the four 640x576 ring sensors (the cast alone on rays that are already on the device,
    and render_mesh_depth whole: host rays, upload, cast, download), 100 000 closest-point queries taken evenly from the volume's
    surface cloud, and the brute form of both on every 360th ray and every 25th query."""
    import time
    from kinectpy_amd.geometry import RaycastingScene, TriangleMesh
    from kinectpy_amd.preprocessing import fusion
    S = 4
    _, depth, _, _, truth = synth.sensor_ring(S, 1)
    depth_d = [torch.as_tensor(depth[0, s]).to(dev) for s in range(S)]
    extr = np.stack([np.linalg.inv(synth.camera_pose(g, S)) for g in range(S)])
    K, origin, length = (synth.FX, synth.FY, synth.CX, synth.CY), (-1000.0, -1100.0, -1000.0), 2000.0
    res = 256 if quick else 512
    vl = length / res
    vol = torch.zeros((res ** 3, 2), dtype=torch.float32, device=dev)
    ops.tsdf_integrate(vol, None, res, vl, origin, 4 * vl, depth_d, None, synth.W, synth.H, K, extr, 1.0, 6000.0)
    vert, _, tri = ops.tsdf_extract_mesh(vol, None, res, vl, origin)
    cloud, _, _ = ops.tsdf_extract(vol, None, res, vl, origin, "surface", want_normals=False)
    del vol
    vert, cloud = ops.transform(vert, extr[0]), ops.transform(cloud, extr[0])          # world -> the master's frame
    nv, nt = int(vert.shape[0]), int(tri.shape[0])
    tag = f"ring mesh of res {res}"
    ms, scene = timed(lambda: ops.rayscene_build(vert, tri))
    report(f"rayscene build ({tag}; centroids + curve sort + leaves + levels; 3 host reads of the index check)", ms, 12 * nt + 12 * nv + int(scene.buf.numel()),
           vertices=nv, triangles=nt, scene_bytes=int(scene.buf.numel()))
    intr = fusion._Intrinsic(synth.W, synth.H, *K)
    s2m = [np.eye(4)] + [np.asarray(T, dtype=np.float64) for T in truth]
    rays = np.stack([RaycastingScene.create_rays_pinhole(intr.intrinsic_matrix, np.linalg.inv(T), synth.W, synth.H, pixel_center=0.0) for T in s2m])
    rays_d = torch.as_tensor(rays.reshape(-1, 6)).to(dev)
    nr = int(rays_d.shape[0])
    ms, out = timed(lambda: ops.rayscene_cast(scene, rays_d))
    hits = int(torch.isfinite(out["t_hit"]).sum().item())
    report(f"rayscene cast, {S} x {synth.W}x{synth.H} pinhole rays ({tag}; device rays, one launch + header read)", ms, rays=nr, hits=hits,
           Mrays_per_s=round(nr / ms / 1e3, 1))
    mesh = TriangleMesh._make(vert, tri)
    walls = []
    for _ in range(7):
        t0 = time.perf_counter()
        img = fusion.render_mesh_depth(mesh, intr, truth)
        walls.append((time.perf_counter() - t0) * 1e3)
    report(f"render_mesh_depth {S} x {synth.W}x{synth.H} ({tag}; host wall time, median of 5 after 2: host rays + scene build + cast + download)",
           float(np.median(walls[2:])), rays=nr, hits=int((img > 0).sum()))
    sub = rays_d[::360].contiguous()
    ms, _ = timed(lambda: ops.rayscene_cast(scene, sub))
    ms_b, _ = timed(lambda: ops.rayscene_cast(scene, sub, brute=True))
    report(f"rayscene cast, every 360th ray ({tag}): hierarchy", ms, rays=int(sub.shape[0]))
    report(f"rayscene cast, every 360th ray ({tag}): brute", ms_b, rays=int(sub.shape[0]), brute_over_hierarchy=round(ms_b / ms, 1))
    nq = 100000
    q = cloud[:: max(1, int(cloud.shape[0]) // nq)][:nq].contiguous()
    ms, _ = timed(lambda: ops.rayscene_closest(scene, q))
    report(f"rayscene closest points, {int(q.shape[0])} surface points ({tag})", ms, queries=int(q.shape[0]), Mqueries_per_s=round(int(q.shape[0]) / ms / 1e3, 1))
    subq = q[::25].contiguous()
    ms, _ = timed(lambda: ops.rayscene_closest(scene, subq))
    ms_b, _ = timed(lambda: ops.rayscene_closest(scene, subq, brute=True))
    report(f"rayscene closest points, every 25th query ({tag}): hierarchy", ms, queries=int(subq.shape[0]))
    report(f"rayscene closest points, every 25th query ({tag}): brute", ms_b, queries=int(subq.shape[0]), brute_over_hierarchy=round(ms_b / ms, 1))


def mesh_check_rows(dev, quick):
    """The mesh checks on the mesh of the fused ring volume (resolution 512, 256 with --quick): every method whole,
    with its index check and host reads; the self-intersection search split into scene build, counting pass (+ scan) and the fill
    (emit + sort + unpack); and the hierarchy against the brute form on 4096 evenly spaced query triangles (searched as another
    mesh's, so that every query has partners: itself and its neighbours)."""
    from kinectpy_amd import _lib as L
    from kinectpy_amd.geometry import TriangleMesh
    S = 4
    _, depth, _, _, _ = synth.sensor_ring(S, 1)
    depth_d = [torch.as_tensor(depth[0, s]).to(dev) for s in range(S)]
    extr = np.stack([np.linalg.inv(synth.camera_pose(g, S)) for g in range(S)])
    K, origin, length = (synth.FX, synth.FY, synth.CX, synth.CY), (-1000.0, -1100.0, -1000.0), 2000.0
    res = 256 if quick else 512
    vl = length / res
    vol = torch.zeros((res ** 3, 2), dtype=torch.float32, device=dev)
    ops.tsdf_integrate(vol, None, res, vl, origin, 4 * vl, depth_d, None, synth.W, synth.H, K, extr, 1.0, 6000.0)
    vert, _, tri = ops.tsdf_extract_mesh(vol, None, res, vl, origin)
    del vol
    nv, nt = int(vert.shape[0]), int(tri.shape[0])
    tag = f"ring mesh of res {res}"
    mesh = TriangleMesh._make(vert, tri)
    ms, out = timed(mesh.get_non_manifold_vertices)
    report(f"mesh get_non_manifold_vertices ({tag}; adjacency + link union-find + compress + flags + compaction + host read)", ms, vertices=nv, triangles=nt,
           non_manifold=int(len(out)))
    ms, out = timed(mesh.is_orientable)
    report(f"mesh is_orientable ({tag}; sort of 3 T edges + double-cover union-find + compress + check + host read)", ms, triangles=nt, orientable=bool(out))
    ms, out = timed(lambda: TriangleMesh._make(vert, tri.clone()).orient_triangles())
    report(f"mesh orient_triangles ({tag}; on a copy of the triangles)", ms, triangles=nt, orientable=bool(out))
    ms, out = timed(lambda: ops.mesh_volume(vert, tri))
    report(f"mesh volume sum ({tag}; one ordered fp64 chain + host read)", ms, 12 * nt + 12 * nv, triangles=nt, value=out)
    ms, out = timed(mesh.euler_poincare_characteristic)
    report(f"mesh euler_poincare_characteristic ({tag}; sort of 3 T edges + count of run heads + host read)", ms, 12 * nt, triangles=nt, value=int(out))
    ms, out = timed(lambda: mesh.is_edge_manifold(False))
    report(f"mesh is_edge_manifold(False) ({tag})", ms, triangles=nt, value=bool(out))
    ms, scene = timed(lambda: ops.rayscene_build(vert, tri))
    report(f"triangle pairs: scene build ({tag})", ms, triangles=nt)
    lib = L.load()
    off = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    args = (L.ptr(scene.buf), scene.buf.numel(), L.ptr(vert), nv, L.ptr(tri), nt, 1)
    ms, _ = timed(lambda: L.check(lib.kpx_rayscene_triangle_pairs_count(*args, 0, 0, L.ptr(off), None, L.stream_ptr())))
    total = int(off[nt].item())
    report(f"triangle pairs: counting pass + scan ({tag}; self search)", ms, triangles=nt, pairs=total)
    if total:
        pairs = torch.empty((total, 2), dtype=torch.int32, device=dev)
        ws, wsz = L.workspace(lib.kpx_rayscene_triangle_pairs_workspace_bytes(total))
        ms, _ = timed(lambda: L.check(lib.kpx_rayscene_triangle_pairs_fill(*args, 0, L.ptr(off), total, L.ptr(pairs), ws, wsz, L.stream_ptr())))
        report(f"triangle pairs: emitting pass + sort + unpack ({tag}; self search)", ms, pairs=total)
    ms, out = timed(lambda: ops.mesh_self_intersections(vert, tri))
    report(f"mesh get_self_intersecting_triangles ({tag}; whole: index checks, build, count, host read, fill)", ms, triangles=nt, pairs=int(out.shape[0]))
    ms, out = timed(mesh.is_self_intersecting)
    report(f"mesh is_self_intersecting ({tag}; whole: build + any-mode search + host read)", ms, triangles=nt, value=bool(out))
    ms, out = timed(lambda: ops.mesh_is_watertight(vert, tri))
    report(f"mesh_is_watertight ({tag}; stops at the first check that fails)", ms, triangles=nt, value=bool(out))
    sub = tri[:: max(1, nt // 4096)][:4096].contiguous()
    ms, a = timed(lambda: ops.rayscene_triangle_pairs(scene, vert, sub))
    ms_b, b = timed(lambda: ops.rayscene_triangle_pairs(scene, vert, sub, brute=True))
    assert torch.equal(a, b)
    report(f"triangle pairs, {int(sub.shape[0])} evenly spaced queries ({tag}): hierarchy", ms, queries=int(sub.shape[0]), pairs=int(a.shape[0]))
    report(f"triangle pairs, {int(sub.shape[0])} evenly spaced queries ({tag}): brute", ms_b, queries=int(sub.shape[0]), pairs=int(b.shape[0]),
           brute_over_hierarchy=round(ms_b / ms, 1))


def voxelgrid_rows(dev, quick):
    """Occupancy grids on S = 4 full-size ring frames: the grid of the fused cloud, carving a dense 2 m grid by the four
    depth frames in one pass against four single-image calls, inclusion of the fused cloud, and the rig's filter end to end.
    Algorithmic traffic of a carve: 8 B key + 12 B colour per voxel read, the same per survivor written, plus the images."""
    from kinectpy_amd import o3d
    from kinectpy_amd.preprocessing.fusion import remove_free_space_points
    S = 4
    _, depth, rgb, _, truth = synth.sensor_ring(S, 1)
    K = (synth.FX, synth.FY, synth.CX, synth.CY)
    to_master = [np.eye(4)] + list(truth)
    parts, cols = [], []
    for s in range(S):                               # the pinhole unprojection of every frame, moved into the master's frame (host)
        pix = np.flatnonzero(depth[0, s] > 0)
        z = depth[0, s][pix].astype(np.float64)
        p = np.stack([((pix % synth.W) - K[2]) / K[0] * z, ((pix // synth.W) - K[3]) / K[1] * z, z, np.ones_like(z)], 1) @ to_master[s].T
        parts.append(p[:, :3].astype(np.float32))
        cols.append(rgb[0, s][pix].astype(np.float32) / np.float32(255.0))
    pts, col = torch.as_tensor(np.concatenate(parts)).to(dev), torch.as_tensor(np.concatenate(cols)).to(dev)
    n = int(pts.shape[0])
    depth_d = [torch.as_tensor(depth[0, s]).to(dev) for s in range(S)]
    extr = np.stack([np.linalg.inv(T) for T in to_master])
    images = S * N_PX * 2

    ms, (keys, kcol, origin) = timed(lambda: ops.voxelgrid_from_cloud(pts, 10.0, col))
    m = int(keys.shape[0])
    report("voxelgrid create_from_point_cloud (fused ring cloud, 10 mm; one host read)", ms, 24 * n + 20 * m, points=n, voxels=m)
    ms, mask = timed(lambda: ops.voxelgrid_included(keys, origin, 10.0, pts))
    report("voxelgrid included_mask (fused ring cloud in its own 10 mm grid)", ms, 13 * n, points=n, included=int(mask.sum().item()))

    carve = lambda k, c, org, v, ims, E: ops.voxelgrid_carve(k, c, org, v, "depth", ims, synth.W, synth.H, K, E, False, False, 1.0, 6000.0)
    for v in ((10.0,) if quick else (10.0, 5.0)):
        cells = int(round(2000.0 / v))
        org = (-1000.0, -1100.0, 1500.0)             # the master's frame: the person stands 2500 in front of it
        dk, dc = ops.voxelgrid_dense((cells, cells, cells), (0.5, 0.5, 0.5))
        total = cells ** 3
        ms_batch, (k1, _) = timed(lambda: carve(dk, dc, org, v, depth_d, extr))
        left = int(k1.shape[0])
        tag = f"dense {cells}^3 at {v:g} mm, {S} x 640x576 u16"
        report(f"voxelgrid carve_depth_maps one pass ({tag})", ms_batch, 20 * (total + left) + images, voxels=total, survivors=left)

        def one_by_one():
            k, c = dk, dc
            for s in range(S):
                k, c = carve(k, c, org, v, depth_d[s:s + 1], extr[s:s + 1])
            return k

        moved = 0
        k, c = dk, dc
        for s in range(S):
            moved += 20 * int(k.shape[0])
            k, c = carve(k, c, org, v, depth_d[s:s + 1], extr[s:s + 1])
            moved += 20 * int(k.shape[0])
        ms_single, k4 = timed(one_by_one)
        assert torch.equal(k4, k1)
        report(f"voxelgrid {S} carve calls of one image ({tag})", ms_single, moved + images, voxels=total, survivors=int(k4.shape[0]),
               single_over_batch=round(ms_single / ms_batch, 3))
        del dk, dc, k1, k4, k, c

    pc = o3d.geometry.PointCloud._make(pts, col)
    ms, (out, kept) = timed(lambda: remove_free_space_points(pc, depth[0], None, truth, 10.0))
    report("remove_free_space_points (fused ring cloud, 10 mm, 4 frames; grid + carve + inclusion + select, host frames uploaded)", ms, points=n,
           kept=int(kept.shape[0]))


def orient_rows(dev, quick):
    """orient_normals_consistent_tangent_plane and the EMST on the voxel-filtered frame cloud and on the same cloud beside a copy of
    itself shifted well clear of it (components closed under their neighbour lists: the unbounded exact search), each beside
    search_index + search_knn at the same n and k -- the like-for-like yardstick -- and the three streaming kernels"""
    fc = ops.voxel_downsample(torch.as_tensor(synth.frame_cloud()).to(dev), 10.0)[0].contiguous()
    bb = ops.bounds(fc).cpu().numpy()
    shift = torch.tensor([3.0 * float(bb[3] - bb[0]), 0.0, 0.0], dtype=torch.float32, device=dev)
    reps = 3 if quick else 10
    for what, pts in (("the voxel-filtered (10 mm) frame cloud", fc),
                      ("the voxel-filtered frame cloud + a copy shifted 3 box lengths", torch.cat([fc, fc + shift]).contiguous())):
        n = int(pts.shape[0])
        nrm = ops.estimate_normals(pts, 70.0, 40)
        for k in (8, 30):
            knn_ms, _ = timed(lambda: ops.search_knn(ops.search_index(pts), pts, k), reps=reps, warm=2)
            report(f"search_index + search_knn k={k}, self-query on {what} (the yardstick)", knn_ms, n=n)
            ms, (_, st) = timed(lambda: ops.emst(pts, k, want_stats=True), reps=reps, warm=2)
            report(f"emst k={k} on {what}", ms, n=n, x_knn=round(ms / knn_ms, 2), **st)
            ms, out = timed(lambda: ops.orient_normals_tangent(pts, nrm, k, want_stats=True), reps=reps, warm=2)
            report(f"orient_normals_tangent k={k} on {what}", ms, n=n, x_knn=round(ms / knn_ms, 2), **out[3])
        for mode in ("normalize", "direction", "camera"):
            ms, _ = timed(lambda: ops.orient_normals(nrm, mode, (0.0, 0.0, 1.0), pts), reps=20, warm=2)
            report(f"orient_normals {mode} on {what}", ms, n * (36 if mode == "camera" else 24), n=n)


def sensor_rows(dev, quick):
    """DESIGN.md 5.21 at the rig's real size: the ray table of one 640 x 576 depth lens, and 4 x 640 x 576 depth with 4 x 1280 x 720 x 3
    colour registered in one launch (masks: 1 channel, nearest).  Algorithmic bytes of color_to_depth: depth 2 + table 8 + output C
    per depth pixel, plus every colour image read once."""
    from kinectpy_amd.calibration import SensorRig
    S = 4
    rig = SensorRig([synth.sensor_calibration(i) for i in range(S)])
    reps = 5 if quick else 20
    ms, _ = timed(lambda: ops.xy_table(rig.calibrations[0].depth), reps=reps, warm=2)
    report("xy_table 640x576 (AC20 Newton inverse, fp64)", ms, N_PX * 8, pixels=N_PX)
    tables = rig.xy_tables()
    depth = torch.as_tensor(np.stack([synth.render_depth(synth.camera_pose(i, S), seed=100 + i) for i in range(S)])).to(dev)
    color = torch.randint(1, 256, (S, 720, 1280, 3), dtype=torch.uint8, device=dev)
    for ch, interp, img in ((3, "bilinear", color), (1, "nearest", color[..., 0].contiguous())):
        out = torch.empty(S * N_PX * ch, dtype=torch.uint8, device=dev)
        ms, res = timed(lambda: ops.color_to_depth(depth, tables, img, rig.calibrations, interp, out=out), reps=reps, warm=2)
        filled = int((res.reshape(S * N_PX, ch) != 0).any(1).sum().item())
        report(f"color_to_depth {S} x 640x576 <- {S} x 1280x720x{ch} {interp}", ms, S * N_PX * (2 + 8 + ch) + S * 720 * 1280 * ch, frames=S,
               filled=filled)
    # the same four frames warped into their 1280 x 720 colour cameras (clear + raster + resolve), and the registrations
    # again with the occlusion test.  Algorithmic bytes of the warp: depth 2 + table 8 per depth pixel, per colour pixel the z-buffer
    # written by the clear and read by the resolve (4 + 4) and the output 2; the raster's atomic minima are counted as `atomics`, not
    # as bytes.  100 mm for both thresholds is this bench's choice for the synthetic room, not a default of the product.
    gap_mm = occlusion_mm = 100.0
    n_col = 720 * 1280
    warped = torch.empty((S, 720, 1280), dtype=torch.uint16, device=dev)
    ms, res = timed(lambda: ops.depth_to_color(depth, tables, 640, 576, rig.calibrations, gap_mm, out=warped), reps=reps, warm=2)
    covered = int((res.view(torch.int16) != 0).sum().item())
    report(f"depth_to_color {S} x 640x576 -> {S} x 1280x720 (z-buffer, 3 dispatches)", ms, S * N_PX * (2 + 8) + S * n_col * (4 + 4 + 2), frames=S,
           covered=covered)
    for ch, interp, img in ((3, "bilinear", color), (1, "nearest", color[..., 0].contiguous())):
        out = torch.empty(S * N_PX * ch, dtype=torch.uint8, device=dev)
        plain = ops.color_to_depth(depth, tables, img, rig.calibrations, interp).reshape(S * N_PX, ch)
        ms, res = timed(lambda: ops.color_to_depth(depth, tables, img, rig.calibrations, interp, out=out, warped=warped, occlusion_mm=occlusion_mm),
                        reps=reps, warm=2)
        res = res.reshape(S * N_PX, ch)
        filled = int((res != 0).any(1).sum().item())
        occluded = int(((plain != 0).any(1) & ~(res != 0).any(1)).sum().item())
        report(f"color_to_depth visible {S} x 640x576 <- {S} x 1280x720x{ch} {interp}", ms,
               S * N_PX * (2 + 8 + ch) + S * n_col * ch + S * n_col * 2, frames=S, filled=filled, occluded=occluded)
    # the undistortion map of one depth lens, then the rig's frames resampled to its common pinhole cameras, one launch
    # per batch.  Algorithmic bytes of a remap per output pixel: map 8 + source C + output C (2 + 2 for depth), the source counted as
    # read once.  The rows of F = 4 frames stay inside the 256 MB cache in front of HBM from one repetition to the next; the rows of
    # the larger batches (frame f uses map f % 4, so the four maps are the only bytes that stay) do not.  100 mm is this bench's choice.
    target_d, target_c = rig.common_pinhole("depth"), rig.common_pinhole("color")
    ms, _ = timed(lambda: ops.undistort_map(rig.calibrations[0].depth, target_d), reps=reps, warm=2)
    report("undistort_map 640x576 (AC22 closed form, fp64)", ms, N_PX * 8, pixels=N_PX)
    maps_d, maps_c = rig.undistort_maps("depth"), rig.undistort_maps("color")
    for F in (S, 16 * S):
        col = color.repeat(F // S, 1, 1, 1)
        out = torch.empty((F, 720, 1280, 3), dtype=torch.uint8, device=dev)
        ms, res = timed(lambda: ops.remap(col, maps_c, "bilinear", out=out), reps=reps, warm=2)
        report(f"remap {F} x 1280x720x3 bilinear", ms, F * n_col * (8 + 3 + 3), frames=F, filled=int((res[:S] != 0).any(-1).sum().item()))
    for F in (S, 64 * S):
        dep = depth.view(torch.int16).reshape(S, 576, 640).repeat(F // S, 1, 1).view(torch.uint16)        # (repeat has no uint16 form)
        out = torch.empty((F, 576, 640), dtype=torch.uint16, device=dev)
        for interp in ("nearest", "bilinear"):
            ms, res = timed(lambda: ops.remap_depth(dep, maps_d, interp, gap_mm, out=out), reps=reps, warm=2)
            report(f"remap_depth {F} x 640x576 {interp}", ms, F * N_PX * (8 + 2 + 2), frames=F, filled=int((res[:S].view(torch.int16) != 0).sum().item()))


def odometry_launches(iterations):
    """dispatches of one kpx_rgbd_odometry call: 2 clears + 1 pose copy, conversion + 2 Gaussian passes, correspondence + sums + scaling
    for the intensity normalisation, per coarser level 2 Gaussian passes + 1 block mean, per level 2 Sobel passes, 2 per iteration,
    2 for the information matrix"""
    levels = len(iterations)
    return 3 + 3 + 3 + 3 * (levels - 1) + 2 * levels + 2 * int(sum(iterations)) + 2


def odometry_rows(dev, quick):
    """RGB-D odometry of full-size 640 x 576 frames of the empty room seen from camera 0 of a ring of four and from that
    pose moved by 1.5 degrees / 40 mm, raw uint16 / uint8 frames resident on the device, millimetre option (30, 0, 6000), hybrid term,
    default iteration list: one pair, and four pairs in one batch call against four single calls.  `ms` is the device time between
    events around the call (the chain's launches and the gaps between them), wall_ms the host time of the call including its one
    read-back; both the median of the repetitions, with their range."""
    import time
    iterations = (20, 10, 5)
    xy = synth.xy_table()
    A = synth.camera_pose(0, 4)
    a_, ax = np.deg2rad(1.5), np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(a_) * Kx + (1 - np.cos(a_)) * Kx @ Kx
    M[:3, 3] = (25.0, -13.0, 29.0)
    frames = []
    for E in (A, A @ M):
        d = synth.render_depth(E=E, xy=xy, noise=0, drop=0, person_shift=(0.0, 1e6, 0.0))
        z = d.astype(np.float64)
        p = np.stack([np.nan_to_num(xy[:, 0]) * z, np.nan_to_num(xy[:, 1]) * z, z], 1) @ E[:3, :3].T + E[:3, 3]
        f = 0.5 + 0.22 * np.sin(p[:, 0] / 310.0) * np.cos(p[:, 1] / 270.0) + 0.2 * np.cos(p[:, 2] / 350.0 + p[:, 0] / 420.0)
        rgb = np.repeat(np.clip(np.rint(255.0 * f), 0, 255).astype(np.uint8)[:, None], 3, 1)
        rgb[d == 0] = 0
        frames.append((torch.as_tensor(d).to(dev), torch.as_tensor(rgb).to(dev)))
    K = (synth.FX, synth.FY, synth.CX, synth.CY)
    truth = np.linalg.inv(A @ M) @ A

    def call(P):
        ds, cs = frames[0][0].expand(P, -1).contiguous(), frames[0][1].expand(P, -1, -1).contiguous()
        dt, ct = frames[1][0].expand(P, -1).contiguous(), frames[1][1].expand(P, -1, -1).contiguous()
        return lambda: ops.rgbd_odometry(ds, cs, dt, ct, synth.W, synth.H, K, None, "hybrid", iterations, 30.0, 0.0, 6000.0, raw=True,
                                         depth_scale=1.0, depth_trunc=6000.0)

    def measure(fn, reps):
        for _ in range(3):
            out = fn()
        torch.cuda.synchronize()
        ev, wall = [], []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(reps):
            t0 = time.perf_counter()
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        stat = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))
        return stat(ev), stat(wall), out

    reps = 10 if quick else 30
    n_launch = odometry_launches(iterations)
    one, four = call(1), call(4)
    (ms, lo, hi), (wms, wlo, whi), (ok, T, _, cnt) = measure(one, reps)
    D = T[0] @ np.linalg.inv(truth)
    report("compute_rgbd_odometry 640x576 hybrid [20, 10, 5] (one pair, raw frames on the device)", ms, ms_range=[round(lo, 4), round(hi, 4)],
           wall_ms=round(wms, 4), wall_ms_range=[round(wlo, 4), round(whi, 4)], launches=n_launch, us_per_launch=round(1e3 * ms / n_launch, 3),
           success=bool(ok[0]), information_correspondences=int(cnt[0]),
           error_deg=round(float(np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))), 4), error_mm=round(float(np.linalg.norm(D[:3, 3])), 3))
    (bms, blo, bhi), (bw, bwlo, bwhi), (okb, Tb, _, _) = measure(four, reps)

    def singles():
        for _ in range(4):
            out = one()
        return out
    (sms, slo, shi), (sw, swlo, swhi), _ = measure(singles, reps)
    assert np.array_equal(Tb[0], T[0]) and np.array_equal(Tb[3], T[0])
    report("compute_rgbd_odometry_batch 4 x 640x576 hybrid [20, 10, 5] (one call)", bms, ms_range=[round(blo, 4), round(bhi, 4)], wall_ms=round(bw, 4),
           wall_ms_range=[round(bwlo, 4), round(bwhi, 4)], launches=n_launch, us_per_launch=round(1e3 * bms / n_launch, 3))
    report("compute_rgbd_odometry 4 calls of one pair (same session)", sms, ms_range=[round(slo, 4), round(shi, 4)], wall_ms=round(sw, 4),
           wall_ms_range=[round(swlo, 4), round(swhi, 4)], launches=4 * n_launch, single_over_batch=round(sms / bms, 3),
           single_over_batch_wall=round(sw / bw, 3))


POINTNET_FLOP_PER_POINT = 219.7e3       # 2 x the multiply-adds of the three trunks as the fused kernels run them (the front recomputed twice)
FP32_PEAK = 157.3                       # TFLOP/s, vector and matrix alike on gfx950


def torch_pointnet(weights, dev):
    """the same 108 arrays as eval-mode torch-ROCm modules: Conv1d(kernel 1) / Linear + BatchNorm1d(eps 1e-3) + ReLU, bmm for the T-nets"""
    nn = torch.nn
    it = iter(weights)

    def block(conv, bn=True):
        k = np.asarray(next(it))
        k = k.reshape(k.shape[-2], k.shape[-1])
        lin = nn.Conv1d(k.shape[0], k.shape[1], 1) if conv else nn.Linear(k.shape[0], k.shape[1])
        lin.weight.data = torch.as_tensor(k.T.copy()).reshape(lin.weight.shape)
        lin.bias.data = torch.as_tensor(np.asarray(next(it)))
        if not bn:
            return lin
        norm = nn.BatchNorm1d(k.shape[1], eps=1e-3)
        norm.weight.data, norm.bias.data = torch.as_tensor(np.asarray(next(it))), torch.as_tensor(np.asarray(next(it)))
        norm.running_mean.data, norm.running_var.data = torch.as_tensor(np.asarray(next(it))), torch.as_tensor(np.asarray(next(it)))
        return nn.Sequential(lin, norm, nn.ReLU())

    class TNet(nn.Module):
        def __init__(self, f):
            super().__init__()
            self.f = f
            self.convs = nn.Sequential(block(True), block(True), block(True))
            self.head = nn.Sequential(block(False), block(False), block(False, bn=False))

        def forward(self, h):                                # h (B, f, N)
            T = self.head(self.convs(h).amax(dim=2)).reshape(-1, self.f, self.f)
            return torch.bmm(h.transpose(1, 2), T).transpose(1, 2)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.t3 = TNet(3)
            self.front = nn.Sequential(block(True), block(True))
            self.t32 = TNet(32)
            self.trunk = nn.Sequential(block(True), block(True), block(True))
            self.head = nn.Sequential(block(False), block(False), block(False, bn=False))

        def forward(self, x):                                # x (B, N, 3)
            h = self.t32(self.front(self.t3(x.transpose(1, 2))))
            return self.head(self.trunk(h).amax(dim=2))

    net = Net().to(dev).eval()
    assert next(it, None) is None
    return net


def pointnet_rows(dev, quick):
    """PointNet forward: the fused path against the same weights as eval-mode torch modules, same device, same process,
    windows of `calls` forwards between two events, the two alternating window by window; median and range over the windows."""
    from kinectpy_amd.models.pointnet import create_pointnet
    from tests import pointnet_ref
    windows, calls = (5, 20) if quick else (15, 50)
    for B, N, J in ((16, 1024, 32), (32, 4096, 32)):
        w = pointnet_ref.make_weights(J, 7)
        m = create_pointnet(N, J)
        m.set_weights(w)
        net = torch_pointnet(w, dev)
        x = torch.as_tensor(pointnet_ref.make_clouds(B, N, pointnet_ref.UNIT, 1)).to(dev)
        packed = m.packed()
        with torch.no_grad():
            forms = {"fused": lambda: ops.pointnet_forward(packed, x), "torch": lambda: net(x)}
            for fn in forms.values():
                for _ in range(5):
                    y = fn()
            torch.cuda.synchronize()
            ya, yb = forms["fused"](), forms["torch"]()
            dev_rel = float((ya - yb).abs().max() / yb.abs().max())
            ts = {k: [] for k in forms}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(windows):
                for name, fn in forms.items():
                    e0.record()
                    for _ in range(calls):
                        y = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ts[name].append(e0.elapsed_time(e1) / calls)
        floor = B * N * POINTNET_FLOP_PER_POINT / (FP32_PEAK * 1e12) * 1e3
        med = {k: float(np.median(v)) for k, v in ts.items()}
        for name in forms:
            report(f"pointnet forward {name} (B, N, J) = ({B}, {N}, {J})", med[name], ms_range=[round(min(ts[name]), 4), round(max(ts[name]), 4)],
                   windows=windows, calls_per_window=calls, fp32_floor_ms=round(floor, 4), TFLOPs_fp32=round(B * N * POINTNET_FLOP_PER_POINT / med[name] / 1e9, 2),
                   torch_over_fused=round(med["torch"] / med["fused"], 3), fused_vs_torch_max_rel=dev_rel)


def pointnet_train_rows(dev, quick):
    """PointNet training step: ops.pointnet_train_step against the same model as train-mode torch modules with
    torch.optim.Adam (tests/pointnet_train_ref.torch_modules), same device, same process, windows of `calls` steps between two events, the
    two alternating window by window; median and range over the windows."""
    from tests import pointnet_train_ref as T
    windows, calls = (5, 10) if quick else (15, 30)
    for B, N, J in ((16, 1024, 32), (32, 4096, 32)):
        w = T.train_weights(J)
        params = ops.pointnet_train_pack(w)
        n = ops.pointnet_train_layout(J)[1]
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        net, loss_fn = T.torch_modules(w, dev)
        opt = torch.optim.Adam(net.parameters(), lr=0.005, eps=1e-7)
        x = torch.as_tensor(T.R.make_clouds(B, N, T.R.UNIT, 1)).to(dev)
        y = torch.as_tensor(np.random.default_rng(1).normal(0, 0.3, (B, 3 * J)).astype(np.float32)).to(dev)
        count = {"t": 0}

        def ours():
            count["t"] += 1
            return ops.pointnet_train_step(params, x, y, m, v, learning_rate=0.005, t=count["t"], step=count["t"])[0]

        def theirs():
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(*net(x), y)
            loss.backward()
            opt.step()
            return loss

        forms = {"kinectpx": ours, "torch": theirs}
        for fn in forms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in forms}
        for _ in range(windows):
            for name, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ts[name].append(e0.elapsed_time(e1) / calls)
        med = {k: float(np.median(t)) for k, t in ts.items()}
        for name in forms:
            report(f"pointnet train step {name} (B, N, J) = ({B}, {N}, {J})", med[name], ms_range=[round(min(ts[name]), 4), round(max(ts[name]), 4)],
                   windows=windows, calls_per_window=calls, torch_over_kinectpx=round(med["torch"] / med["kinectpx"], 3))


if __name__ == "__main__":
    main()

"""The child processes of tests/test_switches_gpu.py: `python tests/switch_workers.py <family> <out.npz>`.

The KPX_* switches are read once per process, so every setting runs one of these in a fresh interpreter; the parent compares the
.npz files.  A worker computes only the operators its family's switches can touch, on the inputs of tests/switch_matrix.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from kinectpy_amd import ops  # noqa: E402
from kinectpy_amd.utils import synth  # noqa: E402
from tests import switch_matrix as M  # noqa: E402


def npy(t):
    return t.cpu().numpy()


def _reg(out, key, r):
    out[key + "_T"] = r["transformation"]
    out[key + "_s"] = np.array([r["fitness"], r["inlier_rmse"], r["iterations"], r["count"]])


def grid(out):
    inp = M.grid_inputs()
    for name, k, ratio in M.sor_cases():
        keep, stats, avg = ops.sor(inp[name], k, ratio, want_avg=True)
        out["sor_%s_%d_keep" % (name, k)], out["sor_%s_%d_stats" % (name, k)], out["sor_%s_%d_avg" % (name, k)] = npy(keep), npy(stats), npy(avg)
    for name in ("halo", "c70k"):
        out["normals_" + name] = npy(ops.estimate_normals(inp[name], *M.NORMALS_ARGS))
    out["radius_halo"] = npy(ops.remove_radius_outlier(inp["halo"], *M.RADIUS_ARGS))
    labels, cnt = ops.cluster_dbscan(inp["halo"], *M.DBSCAN_ARGS)
    out["dbscan_halo_labels"], out["dbscan_halo_count"] = npy(labels), npy(cnt)
    for name in ("halo", "c70k"):
        out["bounds_" + name] = npy(ops.bounds(inp[name]))
    dev = torch.as_tensor(inp["c66k"]).cuda()
    view = dev[1:]                                      # starts 12 bytes into the allocation: not 16-byte aligned
    out["bounds_c66k_aligned"], out["bounds_c66k_view"] = npy(ops.bounds(dev)), npy(ops.bounds(view))
    out["c66k_misalignment"] = np.array([dev.data_ptr() % 16, view.data_ptr() % 16])


def voxel(out):
    inputs, rng = M.voxel_inputs()
    for name, clouds in inputs.items():
        cols, nrms = M.voxel_attrs(clouds, rng)
        if name == "fused":
            for tag, c in (("plain", None), ("col", cols)):
                p, pc = ops.fuse_voxel_downsample(clouds, c, M.fused_transforms(), M.VOXEL_SIZE)
                out["%s_%s_p" % (name, tag)] = npy(p)
                if pc is not None:
                    out["%s_%s_c" % (name, tag)] = npy(pc)
        elif len(clouds) == 1:
            for tag, c, n in (("plain", None, None), ("col", cols[0], None), ("nrm", None, nrms[0])):
                p, pc, pn = ops.voxel_downsample(clouds[0], M.VOXEL_SIZE, c, n)
                out["%s_%s_p" % (name, tag)] = npy(p)
                if pc is not None:
                    out["%s_%s_c" % (name, tag)] = npy(pc)
                if pn is not None:
                    out["%s_%s_n" % (name, tag)] = npy(pn)
        else:
            for tag, c in (("plain", None), ("col", cols)):
                for i, (p, pc) in enumerate(ops.voxel_downsample_batch(clouds, M.VOXEL_SIZE, c)):
                    out["%s_%s_p%d" % (name, tag, i)] = npy(p)
                    if pc is not None:
                        out["%s_%s_c%d" % (name, tag, i)] = npy(pc)


def _gicp_inputs():
    src, tgt, _ = synth.icp_pair(M.DENSE_N)
    return src, tgt, npy(ops.estimate_covariances(src, 1e150, 30)), npy(ops.estimate_covariances(tgt, 1e150, 30))


def _coloured_inputs():
    src, sc, tgt, tc, _ = synth.coloured_pair(M.DENSE_N)
    return src, sc, tgt, tc, npy(ops.estimate_normals(tgt, 70.0, 30))


def icp(out):
    """the inputs of test_parity_gpu._ICP_UPDATE_MODES: one rendered 4-sensor frame, both estimators, the full batch (a launch per
    iteration: its blocks do not fit the one-launch chain), the "small" and "alone" batches (one-launch chains by default); then one
    coloured and one generalized registration through the culled engine"""
    from kinectpy_amd.pipeline import PipelineParams
    P = PipelineParams()
    xy, depth, rgb, inits, _ = synth.sensor_ring(4, 1)
    d = torch.as_tensor(depth[0]).cuda()
    fp, _, _, cnt = ops.depth_to_cloud(d, xy, None, 4, False, False, sync=False)
    k = ops._count(cnt)
    downs = [x[0] for x in ops.voxel_downsample_batch([fp[i, :k[i]] for i in range(4)], P.reg_voxel)]
    tn = ops.estimate_normals(downs[0], 2.0 * P.reg_voxel, P.normals_nn)
    for i, x in enumerate(downs):
        out["down%d" % i] = npy(x)
    out["tn"], out["inits"] = npy(tn), np.stack(inits)
    for mode in ("p2plane", "p2p"):
        for tag, srcs, ini in (("full", downs[1:], inits), ("small", [downs[1][:9000], downs[2][:7001], downs[3][:12000]], inits),
                               ("alone", [downs[3][:20001]], inits[2:3])):
            r = ops.icp_batch(srcs, downs[0], P.icp_max_dist, ini, mode, tn, P.icp_max_iteration)
            out[mode + "_" + tag + "_T"] = np.stack([x["transformation"] for x in r])
            out[mode + "_" + tag + "_s"] = np.array([[x["fitness"], x["inlier_rmse"], x["iterations"], x["count"]] for x in r])
    out["chains"] = np.array([ops.icp_chain(-2)])
    src, sc, tgt, tc, ctn = _coloured_inputs()
    out["coloured_tn"] = ctn
    _reg(out, "coloured", ops.colored_icp(src, sc, tgt, tc, ctn, 80.0, None, 0.968, 25))
    src, tgt, cs, ct = _gicp_inputs()
    out["gicp_cs"], out["gicp_ct"] = cs, ct
    _reg(out, "gicp", ops.generalized_icp(src, cs, tgt, ct, 100.0, None, 30))
    out["engine"] = np.array([ops.NN_ENGINES.index(ops.nn_engine())])


def icp_edges(out):
    """switch_matrix.icp_edges_cases through ops.icp_batch, both estimators, identity initial transforms; per call the one-launch
    chains it started (ops.icp_chain(-2))"""
    src, tgt, _ = synth.icp_pair(M.ICP_EDGES_N)
    tn = ops.estimate_normals(tgt, *M.ICP_EDGES_NORMALS)
    out["tn"] = npy(tn)
    chains = []
    for ci, (srcs, iters) in enumerate(M.icp_edges_cases(src)):
        for mode in ("p2p", "p2plane"):
            before = ops.icp_chain(-2)
            r = ops.icp_batch(srcs, tgt, M.ICP_EDGES_MAX_DIST, [np.eye(4)] * len(srcs), mode, tn if mode == "p2plane" else None, iters)
            out["%s_%d_T" % (mode, ci)] = np.stack([x["transformation"] for x in r])
            out["%s_%d_s" % (mode, ci)] = np.array([[x["fitness"], x["inlier_rmse"], x["iterations"], x["count"]] for x in r])
            chains.append(ops.icp_chain(-2) - before)
    out["chains"] = np.array(chains).reshape(-1, 2)
    out["engine"] = np.array([ops.NN_ENGINES.index(ops.nn_engine())])


def dense(out):
    out["engine_before"] = np.array([ops.NN_ENGINES.index(ops.nn_engine("dense"))])      # what KPX_NN_ENGINE had chosen
    src, tgt, T = synth.icp_pair(M.DENSE_N)
    tn = npy(ops.estimate_normals(tgt, 70.0, 40))
    out["tn"] = tn
    csrc, csc, ctgt, ctc, ctn = _coloured_inputs()
    out["coloured_tn"] = ctn
    _, _, cs, ct = _gicp_inputs()
    out["gicp_cs"], out["gicp_ct"] = cs, ct
    torch.cuda.synchronize()
    ops.prof_begin()
    for tag, T0 in (("eye", None), ("T", T)):
        i, d2 = ops.nn_search(src, tgt, T0)
        out["nn_%s_idx" % tag], out["nn_%s_d2" % tag] = npy(i), npy(d2)
    for mode in ("p2p", "p2plane"):
        r = ops.icp(src, tgt, 100.0, None, mode, tn if mode == "p2plane" else None, M.DENSE_ITERS, want_corr=True)
        _reg(out, mode, r)
        out[mode + "_idx"], out[mode + "_d2"] = npy(r["idx"]), npy(r["d2"])
    r = ops.generalized_icp(src, cs, tgt, ct, 100.0, None, M.DENSE_ITERS, want_corr=True)
    _reg(out, "gicp", r)
    out["gicp_idx"], out["gicp_d2"] = npy(r["idx"]), npy(r["d2"])
    _reg(out, "coloured", ops.colored_icp(csrc, csc, ctgt, ctc, ctn, 80.0, None, 0.968, M.DENSE_ITERS))
    torch.cuda.synchronize()
    prof = ops.prof_end()
    out["launches"] = np.array([prof[name][1] for name in ("nn_screen", "nn_mfma", "nn_local")])
    out["engine"] = np.array([ops.NN_ENGINES.index(ops.nn_engine())])


def frame(out):
    """three frames of a four-sensor ring: kpx_frame_step frame after frame on one thread (the speculation has a history), the
    two-rank in-process sharded loop, the native stream on one GPU and over the two ranks (FRAME_SLOTS frames in flight)"""
    from kinectpy_amd.pipeline import NativeFramePipeline, NativeFrameStream, PipelineParams
    from tests.test_parity_gpu import _local_ranks
    xy, depth, rgb, inits, _ = synth.sensor_ring(4, 3)
    d, c = torch.as_tensor(depth).cuda(), torch.as_tensor(rgb).cuda()
    nat = NativeFramePipeline(xy, 4, inits, PipelineParams())
    for f in range(3):
        p, col, Ts = nat.step(d[f], c[f])
        out["step%d_p" % f], out["step%d_c" % f], out["step%d_T" % f] = npy(p), npy(col), Ts.copy()
        out["step%d_n" % f] = np.array(nat.last["n_down"] + nat.last["n_masked"] + [nat.last["n_voxel"], nat.last["n_out"]] + [it for it, _, _ in nat.last["icp"]])
    seq = (0, 1, 2, 1, 0, 2, 2)
    fs = NativeFrameStream(nat, M.FRAME_SLOTS)
    got = []
    for f in seq:
        if fs.full():
            got.append([npy(t) if isinstance(t, torch.Tensor) else t.copy() for t in fs.pop()])
        fs.submit(d[f], c[f])
    while fs.pending:
        got.append([npy(t) if isinstance(t, torch.Tensor) else t.copy() for t in fs.pop()])
    fs.close()
    for i, (p, col, Ts) in enumerate(got):
        out["stream%d_p" % i], out["stream%d_c" % i], out["stream%d_T" % i] = p, col, Ts
    out["stream_seq"] = np.array(seq)
    res = _local_ranks(2, 4, xy, depth, rgb, inits, "sharded", frames=(0, 1, 2))
    for r in range(2):
        for f, (p, col, Ts, last) in enumerate(res[r]):
            out["shard_r%d_f%d_p" % (r, f)], out["shard_r%d_f%d_c" % (r, f)], out["shard_r%d_f%d_T" % (r, f)] = p, col, Ts
            out["shard_r%d_f%d_n" % (r, f)] = np.array(last["n_down"] + last["n_masked"] + [last["n_voxel"], last["n_out"]] + [it for it, _, _ in last["icp"]])
    res = _local_ranks(2, 4, xy, depth, rgb, inits, "sharded", frames=seq, slots=M.FRAME_SLOTS, native_stream=True)
    for r in range(2):
        for i, (p, col, Ts, _) in enumerate(res[r]):
            out["shardstream_r%d_%d_p" % (r, i)], out["shardstream_r%d_%d_c" % (r, i)], out["shardstream_r%d_%d_T" % (r, i)] = p, col, Ts
    out["chains"] = np.array([ops.icp_chain(-2)])


def fps(out):
    one, batch = M.fps_inputs()
    for n, p in one.items():
        sel, cover = ops.farthest_point_sample(p, M.FPS_K, M.FPS_START, want_cover=True)
        out["fps_%d_sel" % n], out["fps_%d_cover" % n] = npy(sel), npy(cover)
    sel, cover = ops.farthest_point_sample_batch(batch, M.FPS_K, M.FPS_START)
    out["fps_batch_sel"], out["fps_batch_cover"] = npy(sel), npy(cover)


if __name__ == "__main__":
    result = {}
    {"grid": grid, "voxel": voxel, "icp": icp, "icp_edges": icp_edges, "dense": dense, "frame": frame, "fps": fps}[sys.argv[1]](result)
    torch.cuda.synchronize()
    np.savez(sys.argv[2], **result)

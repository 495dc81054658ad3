"""The clouds and calls behind tests/test_knn_wave_identity_gpu.py and tests/golden/make_knn_wave_golden.py: what the wave-per-query
neighbour selection (knn_wave_kernel: remove_statistical_outlier, estimate_normals, estimate_covariances) and the frame step computed
before their reductions, scans and broadcasts moved from ds_bpermute to the vector ALU, and the frame's voxel keys to 32-bit words.

Every cloud has at most 5000 points (coordinates in mm, float32), built from a fixed seed:
  patch       a noisy surface patch: the common path -- k = 20, hybrid (radius 70, max_nn 30) with more than 30 points inside the radius
  few         15 points, k = 20: fewer candidates than k, everything gathered is selected
  lattice     a cubic lattice (exact float32 coordinates): the k-th distance is shared by a whole shell -- k = 20 cuts the shell of 8 at
              d^2 = 300, max_nn = 30 the shell of 6 at d^2 = 400 -- so the lowest original indices decide
  duplicates  30 % of the points are exact copies of others: zero distances are counted, not bucketed
  clump       a dense clump and, inside it, 600 copies of one point: more candidates within the k-th distance than the wave buffer of the
              first pass holds (512), so those queries are truncated, gathered again and handed to the next pass
  sparse      a thin patch plus isolated points, radius 30: some queries find fewer than 3 neighbours ((0, 0, 1) / the identity)"""
import numpy as np

SOR = (20, 2.0)
CASES = {
    "patch": dict(radius=70.0, max_nn=30),
    "few": dict(radius=70.0, max_nn=30),
    "lattice": dict(radius=25.0, max_nn=30),
    "duplicates": dict(radius=70.0, max_nn=30),
    "clump": dict(radius=70.0, max_nn=30),
    "sparse": dict(radius=30.0, max_nn=30),
}


def _patch(rng, n, side, noise=3.0):
    xy = rng.uniform(0.0, side, (n, 2))
    z = 50.0 * np.sin(xy[:, 0] / 150.0) + 30.0 * np.cos(xy[:, 1] / 110.0) + rng.normal(0.0, noise, n)
    return np.column_stack([xy, z])


def cloud(name):
    rng = np.random.default_rng({"patch": 11, "few": 12, "lattice": 13, "duplicates": 14, "clump": 15, "sparse": 16}[name])
    if name == "patch":
        p = _patch(rng, 2500, 800.0)
    elif name == "few":
        p = rng.uniform(-50.0, 50.0, (15, 3))
    elif name == "lattice":
        g = np.arange(12, dtype=np.float64) * 10.0
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        p = p[rng.permutation(len(p))]                               # the index rule must not coincide with the grid order
    elif name == "duplicates":
        p = _patch(rng, 2000, 700.0)
        dst = rng.choice(2000, 600, replace=False)
        src = rng.choice(np.setdiff1d(np.arange(2000), dst), 600)
        p[dst] = p[src]
    elif name == "clump":
        centre = np.array([400.0, 400.0, 20.0])
        p = np.concatenate([_patch(rng, 1200, 800.0), centre + rng.normal(0.0, 0.5, (700, 3)), np.repeat(centre[None] + 0.25, 600, 0)])
        p = p[rng.permutation(len(p))]
    elif name == "sparse":
        lone = np.stack(np.meshgrid(np.arange(10) * 200.0, np.arange(10) * 200.0, [500.0], indexing="ij"), -1).reshape(-1, 3)
        p = np.concatenate([_patch(rng, 1900, 800.0), lone + rng.uniform(-5.0, 5.0, lone.shape)])
        p = p[rng.permutation(len(p))]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(p, dtype=np.float32)


def run_case(ops, name):
    """-> the arrays of one case, by key: SOR mean distances / keep list / statistics, normals, covariances"""
    import torch
    pts = torch.as_tensor(cloud(name)).cuda()
    keep, stats, avg = ops.sor(pts, SOR[0], SOR[1], want_avg=True)
    out = {"sor.avg": avg, "sor.keep": keep, "sor.stats": stats,
           "normals": ops.estimate_normals(pts, CASES[name]["radius"], CASES[name]["max_nn"]),
           "cov": ops.estimate_covariances(pts, CASES[name]["radius"], CASES[name]["max_nn"])}
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_frame():
    """one frame set of the four-sensor ring through the native frame loop -> fused points, colours, transforms"""
    import torch
    from kinectpy_amd.pipeline import NativeFramePipeline, PipelineParams
    from kinectpy_amd.utils import synth
    xy, depth, rgb, inits, _ = synth.sensor_ring(4, 1)
    p, c, T = NativeFramePipeline(xy, 4, inits, PipelineParams()).step(torch.as_tensor(depth[0]).cuda(), torch.as_tensor(rgb[0]).cuda())
    return {"points": p.cpu().numpy(), "colours": c.cpu().numpy(), "transforms": np.asarray(T)}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()

"""The clouds and calls behind tests/test_knn_group_gpu.py and tests/golden/make_knn_group_golden.py: what remove_statistical_outlier,
kpx_sor_partial, estimate_normals and estimate_covariances computed before the group pass (knn_group_kernel: a query per row of 16 lanes,
four queries per wave, settle or hand on) was put in front of the wave-per-query passes.

Every cloud has at most 5000 points (coordinates in mm, float32), built from a fixed seed:
  tiny_<n>       n = 1, 2, 3, 5, 41 random points: tail rows (n is no multiple of 4) and fewer candidates than k in a block that is whole
  slab           a flat patch, thinner than a cell: ONE cell layer in z, so every block is clipped below and above, and the queries along
                 the rim are clipped in x and y as well
  <wave case>_p  the six clouds of tests/knn_wave_cases.py at (k, ratio) = (8, 2.0) and (32, 2.0) and (radius, max_nn) = (70, 48)
  alternate      a dense patch and, above every column of its cells, a few isolated points: in cell order (z runs fastest) dense queries
                 that settle and sparse ones that are handed on follow each other, so they meet in the rows of one wave
  straddle_<c>   a clump of c points far smaller than a cell, the rest of the cloud far more than a block away: every query of the clump
                 gathers exactly c candidates -- c = G - 1, G, G + 1 around the group buffers G = 192 (normals) and 256 (SOR)
  partial        kpx_sor_partial over ranges of the patch's grid order whose ends are no multiples of 4"""
import numpy as np

import knn_wave_cases as W

# candidates per query the group pass holds, by call (KPX_KNN_GROUP_CAP_SOR / _NORMALS, csrc/kpx_knn.hip): m >= the cap is handed on
GROUP_CAP = {"sor20": 256, "nrm70_30": 192}
STRADDLE = tuple(g + d for g in (192, 256) for d in (-1, 0, 1))
PARTIAL_K = 20
PARTIAL_RANGES = ((0, 2500), (3, 1001), (1, 2), (1234, 1241), (2495, 2500), (7, 7))


def _case(cloud, sor=((20, 2.0),), normals=((70.0, 30),), partial=()):
    return dict(cloud=cloud, sor=tuple(sor), normals=tuple(normals), partial=tuple(partial))


def _tiny(n):
    return lambda: np.random.default_rng(100 + n).uniform(-40.0, 40.0, (n, 3))


def _slab():
    rng = np.random.default_rng(21)
    return np.column_stack([rng.uniform(0.0, 700.0, (2200, 2)), rng.uniform(-0.5, 0.5, 2200)])


def _alternate():
    rng = np.random.default_rng(22)
    base = W._patch(rng, 2600, 800.0)
    xy = rng.uniform(0.0, 800.0, (1100, 2))
    z = 50.0 * np.sin(xy[:, 0] / 150.0) + 30.0 * np.cos(xy[:, 1] / 110.0) + rng.uniform(90.0, 600.0, 1100)
    p = np.concatenate([base, np.column_stack([xy, z])])
    return p[rng.permutation(len(p))]


def _straddle(c):
    def make():
        rng = np.random.default_rng(300 + c)
        centre = np.array([1000.0, 1000.0, 1000.0])
        clump = centre + rng.uniform(-2.0, 2.0, (c, 3))
        corners = np.stack(np.meshgrid([0.0, 2000.0], [0.0, 2000.0], [0.0, 2000.0], indexing="ij"), -1).reshape(-1, 3)
        far = np.repeat(corners, 5, 0) + rng.uniform(-60.0, 60.0, (40, 3))      # >= 800 mm from the clump on every axis
        p = np.concatenate([clump, far])
        return p[rng.permutation(len(p))]
    return make


CASES = {}
for _n in (1, 2, 3, 5, 41):
    CASES["tiny_%d" % _n] = _case(_tiny(_n))
CASES["slab"] = _case(_slab)
for _name in W.CASES:
    CASES[_name + "_p"] = _case((lambda nm: lambda: W.cloud(nm))(_name), sor=((8, 2.0), (32, 2.0)), normals=((70.0, 48),))
CASES["alternate"] = _case(_alternate)
for _c in STRADDLE:
    CASES["straddle_%d" % _c] = _case(_straddle(_c))
CASES["partial"] = _case(lambda: W.cloud("patch"), sor=(), normals=(), partial=PARTIAL_RANGES)


def cloud(name):
    return np.ascontiguousarray(CASES[name]["cloud"](), dtype=np.float32)


def run_case(ops, name, counts=None):
    """-> the arrays of one case by key.  counts (a dict): receives ops.knn_group_last() after every call that has a group pass"""
    import torch
    case = CASES[name]
    pts = torch.as_tensor(cloud(name)).cuda()
    out = {}

    def note(key):
        if counts is not None:
            counts[key] = ops.knn_group_last()

    for k, ratio in case["sor"]:
        keep, stats, avg = ops.sor(pts, k, ratio, want_avg=True)
        note("sor%d" % k)
        out.update({"sor%d.avg" % k: avg, "sor%d.keep" % k: keep, "sor%d.stats" % k: stats})
    for radius, max_nn in case["normals"]:
        tag = "nrm%d_%d" % (radius, max_nn)
        out[tag + ".normals"] = ops.estimate_normals(pts, radius, max_nn)
        note(tag)
        out[tag + ".cov"] = ops.estimate_covariances(pts, radius, max_nn)
    for q0, q1 in case["partial"]:
        avg, order = ops.sor_partial(pts, PARTIAL_K, q0, q1)
        note("partial_%d_%d" % (q0, q1))
        out["partial_%d_%d.avg" % (q0, q1)] = avg
        if (q0, q1) == case["partial"][0]:
            out["partial.order"] = order
    return {k: v.cpu().numpy() for k, v in out.items()}

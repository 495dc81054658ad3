"""Registry of the scratch contract's cases (tests/test_scratch_gpu.py, tests/test_scratch_cases_cpu.py) -- TEST INFRASTRUCTURE ONLY.

One entry per function of kinectpy_amd/ops.py whose body calls L.workspace(.  An entry gives

  sizes            names of its input sets, largest first ("large", "small", for the streaming operators also "one": n = 1)
  make(size)       the inputs (a dict), from seeds, by the generators the operator's own suite uses
  run(inputs)      -> tuple of host arrays cut to the documented valid part (rows below the returned count)
  check(res, inp)  the operator's existing CPU reference by its own suite's rule (bit-exact, or that suite's tolerance, imported or
                   restated from the test named beside it -- no new tolerance is made up here)

Sizes are the smallest at which scratch can go wrong: "small" lies below one block or tile of the operator's first kernel, "large"
is three tiles and a ragged tail (TILE: kCompactTile = kRxTile = kGridScanTile = 2048 items, restated from kpx_compact.h / kpx_radix.h /
kpx_knn.hip as tests/test_boundaries_gpu.py restates them) or one past a form switch (the limits of include/kinectpx.h are read from
it).  "one" (n = 1) goes to the twenty operators whose own suites run a single point, pixel or pair and whose references are defined
there; the registrations and solves need three pairs, the features and covariances a neighbourhood, the meshes and scenes a triangle,
RANSAC and FGR three correspondences, PointNet training a case that meets its input condition (its "small" has N = 1).
Batched operators get three elements of unequal sizes, one of them empty or failing where the operator takes one: an empty cloud in
the voxel batches, a frame without a valid pixel, a pair without depth in rgbd_odometry; farthest_point_sample_batch requires
k <= n of every cloud, so an empty cloud is legal only with k = 0, where nothing is computed: its "one" batch holds 1, 2 and 3 points.
"""
import functools
import os
import re

import numpy as np
import torch

from kinectpy_amd.utils import synth
from oracle import oracle as O

_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kinectpx.h")).read()
_define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, _HEADER).group(1))

TILE = 2048
LARGE = 3 * TILE + 857                    # 7001: three tiles and a ragged tail
SMALL = 37                                # less than a wave, not a multiple of the 8-item vector width
BLOCK_SWITCH = 65536                      # kpx_bounds / kpx_transform: one block below, the grid form above; the grid build's own sort above
from test_parity_gpu import TOL_PLANE, TOL_STATS, TOL_T          # the owning suite's tolerances: a change there reaches this file

CASES = {}
EXCLUDED = {
    "frame_step_sharded": "needs ranks (a communicator); its sharded loop is tested in tests/test_parity_gpu.py",
}


class Case:
    def __init__(self, name, make, run, check, sizes=("large", "small")):
        self.name, self.make, self.run, self.check, self.sizes = name, make, run, check, tuple(sizes)


def add(name, make, run, check, sizes=("large", "small")):
    assert name not in CASES, name
    CASES[name] = Case(name, make, run, check, sizes)


def _ops():
    from kinectpy_amd import ops
    return ops


def npy(t):
    return None if t is None else t.cpu().numpy()


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _n(size, large=LARGE, small=SMALL):
    return {"large": large, "small": small, "one": 1}[size]


@functools.lru_cache(maxsize=None)
def base_cloud():
    return synth.frame_cloud()


def subset(n, seed):
    """n rows of the frame cloud (integer millimetres), unsorted"""
    b = base_cloud()
    return np.ascontiguousarray(b[np.random.default_rng(seed).choice(len(b), n, replace=False)])


def eq(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())


# ================================================================================================ extract (tests/test_parity_gpu.py)
def _median_make(size):
    n = _n(size, large=3 * 8192 + 857)          # kMedWin = 8192 (kpx_extract.hip)
    rng = np.random.default_rng(1 + n)
    v = rng.integers(-32768, 32767, size=(3, n, 3)).astype(np.int16)
    if n > 10:
        v[1, :, 2] = 1234
        v[2, : n // 2, 2], v[2, n // 2:, 2] = -5, 6
    return dict(v=v, n=n)


def _median_run(i):
    t = cuda(i["v"])
    return (npy(_ops().median_i16(t.reshape(-1)[2:], i["n"], 3, 3)),)


def _median_check(res, i):
    assert res[0].tolist() == [float(np.median(i["v"][f, :, 2])) for f in range(3)]


add("median_i16", _median_make, _median_run, _median_check, ("large", "small", "one"))


def _frames_make(size):
    """three frames of unequal content as test_extract_random_frames_match_oracle makes them; the last one holds no valid pixel"""
    n = _n(size)
    rng = np.random.default_rng(123 + n)
    t = rng.normal(scale=0.5, size=(n, 2)).astype(np.float32)
    t[rng.random(n) < 0.01] = np.nan
    d = rng.integers(300, 6000, size=(3, n)).astype(np.uint16)
    d[0][rng.random(n) < 0.1] = 0
    d[1][rng.random(n) < 0.6] = 0
    d[2] = 0
    rgb = rng.integers(0, 255, size=(3, n, 3)).astype(np.uint8)
    rgb[rng.random((3, n)) < 0.4] = 0
    xyz = np.stack([O.unproject_u16(d[f], t) for f in range(3)])
    return dict(n=n, t=t, d=d, rgb=rgb, xyz=xyz)


def _frames_flat(res):
    return tuple(npy(a) for frame in res for a in frame)


def _frames_check(res, i):
    for f in range(3):
        rp, rc, ri = O.rgbd_compact(i["xyz"][f], i["rgb"][f], True, True, O.median_z(i["xyz"][f]) + 750.0)
        eq(res[3 * f], rp, ("points", f)), eq(res[3 * f + 1], rc, ("colours", f)), eq(res[3 * f + 2], ri, ("idx", f))
    assert len(res[6]) == 0


add("rgbd_compact", _frames_make, lambda i: _frames_flat(_ops().rgbd_compact(i["xyz"], i["rgb"], 3, True, True, want_idx=True)), _frames_check,
    ("large", "small", "one"))
add("depth_to_cloud", _frames_make, lambda i: _frames_flat(_ops().depth_to_cloud(i["d"], i["t"], i["rgb"], 3, True, True, want_idx=True)),
    _frames_check, ("large", "small", "one"))


# ============================================================================================== container (tests/test_parity_gpu.py)
def _cloud_make(size, large=LARGE, seed=23):
    n = _n(size, large)
    rng = np.random.default_rng(seed + n)
    p = rng.normal(scale=700, size=(n, 3)).astype(np.float32)
    if n > 3:
        p[0, 0], p[n - 1, 1], p[n // 2, 2] = -9e4, 8e4, -7e4          # the extremes at the ends and inside a chunk
    k = int(rng.integers(1, n + 1))
    idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
    col = rng.random((n, 3)).astype(np.float32)
    return dict(n=n, p=p, idx=idx, col=col, slab=float(rng.uniform(1, 900)),
                plane=[float(x) for x in rng.normal(size=3)] + [float(rng.normal(scale=200))])


_big_cloud_make = functools.partial(_cloud_make, large=BLOCK_SWITCH + LARGE)


def _bounds_check(res, i):
    eq(res[0], np.concatenate([i["p"].min(0), i["p"].max(0)]).astype(np.float64))


add("bounds", _big_cloud_make, lambda i: (npy(_ops().bounds(i["p"])),), _bounds_check, ("large", "small", "one"))


def _select_run(i):
    """both paths and the three modes: the mask selection, its inverse, the trusted gather, and the gather that leaves the bounds"""
    ops, p, col = _ops(), cuda(i["p"]), cuda(i["col"])
    shuffled = i["idx"][np.random.default_rng(5).permutation(len(i["idx"]))]
    a = ops.select_by_index([p, col], np.concatenate([shuffled, shuffled[:3]]))
    b = ops.select_by_index([p, None, col], i["idx"], invert=True)
    c = ops.select_by_index([p], i["idx"], trusted=True)
    (d0, d1, _), bb = ops.select_by_index([p, col, None], i["idx"], trusted=True, want_bounds=True)
    return npy(a[0]), npy(a[1]), npy(b[0]), npy(b[2]), npy(c[0]), npy(d0), npy(d1), npy(bb)


def _select_check(res, i):
    p, col, idx = i["p"], i["col"], i["idx"]
    m = np.ones(i["n"], bool)
    m[idx] = False
    for g, w in zip(res, (p[idx], col[idx], p[m], col[m], p[idx], p[idx], col[idx],
                          np.concatenate([p[idx].min(0), p[idx].max(0)]).astype(np.float64))):
        eq(g, w)


add("select_by_index", _big_cloud_make, _select_run, _select_check, ("large", "small", "one"))
add("halfspace_select", _cloud_make, lambda i: (npy(_ops().halfspace_select(i["p"], i["plane"])),),
    lambda res, i: eq(res[0], O.halfspace_keep_idx(*i["plane"], i["p"])), ("large", "small", "one"))


def _slab_run(i):
    ops, p = _ops(), cuda(i["p"])
    lo, up = ops.slab_split(p, i["slab"])
    lo2, up2 = ops.slab_split(p, i["slab"], bounds=ops.bounds(p))
    return npy(lo), npy(up), npy(lo2), npy(up2)


def _slab_check(res, i):
    y = i["p"][:, 1].astype(np.float64)
    lo, up = np.flatnonzero(y >= y.max() - i["slab"]), np.flatnonzero(y < y.max() - i["slab"])
    eq(res[0], lo), eq(res[1], up), eq(res[2], lo), eq(res[3], up)


add("slab_split", _big_cloud_make, _slab_run, _slab_check, ("large", "small", "one"))


def _sort_make(size):
    n = _n(size, large=BLOCK_SWITCH + LARGE)       # one past the own sort's first group-row boundary (test_radix_sort_pairs_is_the_stable_sort)
    rng = np.random.default_rng(n + 24)
    keys = (rng.integers(0, 37, n, dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    keys[::2] = rng.integers(0, 1 << 32, len(keys[::2]), dtype=np.uint64).astype(np.uint32)
    return dict(keys=keys, vals=np.arange(n, dtype=np.int32)[::-1].copy(), end_bit=24)


def _sort_run(i):
    ko, vo = _ops().sort_pairs_u32(torch.from_numpy(i["keys"].view(np.int32)).cuda().view(torch.uint32), cuda(i["vals"]), i["end_bit"])
    return npy(ko.view(torch.int32)).view(np.uint32), npy(vo)


def _sort_check(res, i):
    order = np.argsort(i["keys"] & np.uint32((1 << i["end_bit"]) - 1), kind="stable")
    eq(res[0], i["keys"][order], "keys"), eq(res[1], i["vals"][order], "values")


add("sort_pairs_u32", _sort_make, _sort_run, _sort_check, ("large", "small", "one"))


def _sample_make(size):
    n = _n(size)
    return dict(p=subset(n, 3), k=max(1, n // 3), seed=2 ** 63 + 5 + n)


def _sample_check(res, i):
    ref = O.sample_indices(len(i["p"]), i["k"], i["seed"])
    eq(res[1], ref), eq(res[0], i["p"][ref])


add("sample_points", _sample_make, lambda i: tuple(npy(t) for t in _ops().sample_points(i["p"], i["k"], i["seed"])), _sample_check,
    ("large", "small", "one"))


# ================================================================================================ filters (tests/test_parity_gpu.py)
def _voxel_make(size):
    n = _n(size)
    rng = np.random.default_rng(n)
    p = subset(n, 1)
    return dict(p=p, col=rng.random(p.shape).astype(np.float32), nrm=rng.normal(size=p.shape).astype(np.float32), voxel=35.0)


def _voxel_check(res, i):
    for g, w in zip(res, O.voxel_downsample(i["p"], i["voxel"], i["col"], i["nrm"])):
        eq(g, w)


add("voxel_downsample", _voxel_make, lambda i: tuple(npy(t) for t in _ops().voxel_downsample(i["p"], i["voxel"], i["col"], i["nrm"])),
    _voxel_check, ("large", "small", "one"))


def _clouds_make(size):
    """three clouds of unequal sizes, the middle one empty"""
    n = _n(size)
    rng = np.random.default_rng(5 + n)
    clouds = [subset(n, 2), np.zeros((0, 3), np.float32), (subset(max(n // 3, 1), 3) + np.float32(7.0)).astype(np.float32)]
    cols = [rng.random(c.shape).astype(np.float32) for c in clouds]
    Ts = [np.eye(4)] + [synth.perturb(np.eye(4), deg=float(rng.uniform(0, 40)), mm=float(rng.uniform(0, 900)), seed=int(rng.integers(1 << 30)))
                        for _ in range(2)]
    return dict(clouds=clouds, cols=cols, Ts=Ts, voxel=35.0)


def _voxel_batch_check(res, i):
    for c, (cloud, col) in enumerate(zip(i["clouds"], i["cols"])):
        if len(cloud) == 0:
            assert len(res[2 * c]) == 0 and len(res[2 * c + 1]) == 0
            continue
        rp, rc, _ = O.voxel_downsample(cloud, i["voxel"], col)
        eq(res[2 * c], rp), eq(res[2 * c + 1], rc)


add("voxel_downsample_batch", _clouds_make,
    lambda i: tuple(npy(t) for pair in _ops().voxel_downsample_batch(i["clouds"], i["voxel"], i["cols"]) for t in pair), _voxel_batch_check)


def _fuse_check(res, i):
    rp, rc = O.fuse_voxel_downsample(i["clouds"], i["cols"], i["Ts"], i["voxel"])
    eq(res[0], rp), eq(res[1], rc)


add("fuse_voxel_downsample", _clouds_make, lambda i: tuple(npy(t) for t in _ops().fuse_voxel_downsample(i["clouds"], i["cols"], i["Ts"], i["voxel"])),
    _fuse_check)


def _sor_make(size, k=20):
    n = _n(size)
    return dict(p=subset(n, n + k), k=k, ratio=2.0)


def _sor_check(res, i):
    """test_sor_indices_bit_exact"""
    ri, rs, ra = O.sor(i["p"], i["k"], i["ratio"])
    eq(res[0], ri)
    assert np.allclose(res[2], ra, rtol=1e-14, atol=0)
    if len(i["p"]) > 2:                                   # (as the suite: one or two points have no deviation to compare)
        assert np.allclose(res[1], rs, rtol=TOL_STATS, atol=0)


add("sor", _sor_make, lambda i: tuple(npy(t) for t in _ops().sor(i["p"], i["k"], i["ratio"], want_avg=True)), _sor_check, ("large", "small", "one"))


def _sor_select_make(size):
    i = _sor_make(size)
    i["col"] = np.random.default_rng(4).random(i["p"].shape).astype(np.float32)
    return i


def _sor_select_check(res, i):
    """test_sor_select_equals_filter_then_selection, with the oracle's keep list in the filter's place"""
    ri, rs, _ = O.sor(i["p"], i["k"], i["ratio"])
    eq(res[0], i["p"][ri]), eq(res[1], i["col"][ri]), eq(res[2], ri)
    assert np.allclose(res[3], rs, rtol=TOL_STATS, atol=0)


add("sor_select", _sor_select_make, lambda i: tuple(npy(t) for t in _ops().sor_select(i["p"], i["col"], i["k"], i["ratio"])), _sor_select_check)


def _sor_partial_run(i):
    ops, p, n = _ops(), cuda(i["p"]), len(i["p"])
    rows = -(-n // 3)
    parts, order = [], None
    for r in range(3):
        part, order = ops.sor_partial(p, i["k"], min(n, r * rows), min(n, (r + 1) * rows))
        parts.append(npy(part))
    return np.concatenate(parts), npy(order)


def _sor_partial_check(res, i):
    """test_sharded_sor_bit_identical_to_one_call: the order is a permutation; the means, put back by it, are the oracle's to 1e-12"""
    avg_sorted, order = res
    assert sorted(order.tolist()) == list(range(len(i["p"])))
    avg = np.empty_like(avg_sorted)
    avg[order] = avg_sorted
    assert np.allclose(avg, O.sor(i["p"], i["k"], i["ratio"])[2], rtol=1e-12, atol=0)


add("sor_partial", _sor_make, _sor_partial_run, _sor_partial_check)


def _sor_finish_make(size):
    i = _sor_make(size)
    i["avg"] = O.sor(i["p"], i["k"], i["ratio"])[2]
    i["order"] = np.random.default_rng(8).permutation(len(i["p"])).astype(np.int32)
    return i


def _sor_finish_check(res, i):
    keep, stats = O.sor_from_avg(i["avg"], i["ratio"])
    eq(res[0], keep), eq(res[2], i["avg"])
    assert np.allclose(res[1], stats, rtol=TOL_STATS, atol=0)


add("sor_finish", _sor_finish_make, lambda i: tuple(npy(t) for t in _ops().sor_finish(i["avg"][i["order"]], i["order"], i["ratio"], want_avg=True)),
    _sor_finish_check)


def normals_rule(gn, p, radius, nn, bound=1e-6):
    """test_normals_up_to_sign: the oracle's normal up to sign wherever the covariance has a gap, (0, 0, 1) below three neighbours"""
    gn = gn.astype(np.float64)
    rn, cov, cnt = O.estimate_normals(p, radius, nn)
    A = np.zeros((len(p), 3, 3))
    A[:, 0, 0], A[:, 1, 1], A[:, 2, 2] = cov[:, 0], cov[:, 3], cov[:, 5]
    A[:, 0, 1] = A[:, 1, 0] = cov[:, 1]
    A[:, 0, 2] = A[:, 2, 0] = cov[:, 2]
    A[:, 1, 2] = A[:, 2, 1] = cov[:, 4]
    w = np.linalg.eigvalsh(A)
    well = (cnt >= 3) & ((w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-30))
    assert (np.abs((gn * rn).sum(1))[well] > 1 - bound).all()
    assert np.allclose(gn[cnt < 3], [0, 0, 1])
    assert np.isfinite(gn).all()


def _normals_make(size):
    n = _n(size)
    return dict(p=subset(n, 2), radius=250.0 if n > 100 else 2000.0, nn=40)


add("estimate_normals", _normals_make, lambda i: (npy(_ops().estimate_normals(i["p"], i["radius"], i["nn"])),),
    lambda res, i: normals_rule(res[0], i["p"], i["radius"], i["nn"]), ("large", "small", "one"))


def _plane_make(size):
    """the floor slab of test_segment_plane_inliers_bit_exact"""
    n = _n(size, small=100)
    c3 = synth.filter_cloud(200_000)
    return dict(p=np.ascontiguousarray(c3[c3[:, 1] >= c3[:, 1].max() - 200][:n]), rn=30 if n > 100 else 3, iters=100, seed=7)


def _plane_run(i):
    pl, idx = _ops().segment_plane(i["p"], 30.0, i["rn"], i["iters"], 0.99999999, i["seed"])
    return pl, npy(idx)


def _plane_check(res, i):
    rpl, ridx = O.segment_plane(i["p"], 30.0, i["rn"], i["iters"], 0.99999999, i["seed"])
    eq(res[1], ridx)
    assert np.abs(res[0] - rpl).max() < TOL_PLANE


add("segment_plane", _plane_make, _plane_run, _plane_check)


# ====================================================================== registration (tests/test_parity_gpu.py and the suites named below)
@functools.lru_cache(maxsize=None)
def _pair(n):
    src, tgt, T = synth.icp_pair(n, base_cloud())
    return src, tgt, T


def _pair_make(size, large=3001, small=200, m_of=lambda n: n):
    """an ICP pair of the frame cloud; the target a different size from the source"""
    n = _n(size, large, small)
    src, tgt, T = _pair(max(n, m_of(n)))
    tgt = np.ascontiguousarray(tgt[:m_of(n)])
    tn = O.estimate_normals(tgt, 70.0 if n > 1000 else 400.0, 40)[0].astype(np.float32)
    return dict(src=np.ascontiguousarray(src[:n]), tgt=tgt, T=T, tn=tn)


_nn_make = functools.partial(_pair_make, large=LARGE, small=SMALL, m_of=lambda n: n // 2 + 11)


def _nn_check(res, i):
    """test_nn_bit_exact"""
    ri, rd, _ = O.nn(i["src"], np.linalg.inv(i["T"]), i["tgt"], grid=False)
    eq(res[0], ri), eq(res[1], rd)


add("nn_search", _nn_make, lambda i: tuple(npy(t) for t in _ops().nn_search(i["src"], i["tgt"], np.linalg.inv(i["T"]))), _nn_check, ("large", "small", "one"))


def _eval_run(i):
    r = _ops().registration_eval(i["src"], i["tgt"], 100.0, np.linalg.inv(i["T"]), want_corr=True)
    return np.array([r["fitness"], r["inlier_rmse"], float(r["count"])]), r["information"], npy(r["idx"]), npy(r["d2"])


def _eval_check(res, i):
    """tests/test_multiway_gpu.py: _check_eval"""
    import multiway_ref as M
    ref = M.registration_eval(O, i["src"], i["tgt"], 100.0, np.linalg.inv(i["T"]))
    (fit, rmse, cnt), L = res[0], res[1]
    eq(res[2], ref["idx"]), eq(res[3], ref["d2"])
    assert cnt == ref["count"] and fit == ref["count"] / len(i["src"]) and 0 < ref["count"]
    assert abs(rmse - ref["inlier_rmse"]) <= ref["rmse_bound"]
    assert (np.abs(L - ref["information"]) <= ref["information_bound"]).all()
    assert np.array_equal(L, L.T) and np.array_equal(L[3:, 3:], ref["count"] * np.eye(3))


add("registration_eval", _nn_make, _eval_run, _eval_check)


def _kabsch_make(size):
    i = _pair_make(size, large=LARGE, small=SMALL)
    rng = np.random.default_rng(0)
    n = len(i["src"])
    k = max(3, n // 3)
    i["corr"] = np.stack([rng.choice(n, k, replace=False), rng.choice(n, k, replace=False)], 1).astype(np.int32)
    return i


add("kabsch", _kabsch_make, lambda i: (_ops().kabsch(i["src"], i["tgt"], i["corr"]),),
    lambda res, i: np.testing.assert_array_less(np.abs(res[0] - O.kabsch(i["src"][i["corr"][:, 0]], i["tgt"][i["corr"][:, 1]])).max(), 1e-9))


def _reg_tuple(r, corr=False):
    out = (r["transformation"], np.array([r["fitness"], r["inlier_rmse"], float(r["iterations"]), float(r["count"])]))
    return out + ((npy(r["idx"]), npy(r["d2"])) if corr else ())


def _icp_run(i):
    ops = _ops()
    a = ops.icp(i["src"], i["tgt"], 100.0, None, "p2p", None, 6, want_corr=True)
    b = ops.icp(i["src"], i["tgt"], 100.0, None, "p2plane", i["tn"], 6)
    return _reg_tuple(a, True) + _reg_tuple(b)


def _icp_rule(T, stats, ref):
    """test_icp_matches_oracle"""
    rT, rf, rr, rit = ref[:4]
    assert stats[2] == rit and stats[0] == rf
    assert abs(stats[1] - rr) < 1e-9 * max(rr, 1)
    assert np.abs(T - rT).max() < TOL_T


def _icp_check(res, i):
    """the correspondences returned are those of the last search: judged as tests/test_gicp_gpu.py judges generalized_icp's -- the same
    rows within max_dist as the oracle's last search (the transforms of the two sides agree to TOL_T only), with the same partners"""
    trace = []
    _icp_rule(res[0], res[1], O.registration_icp(i["src"], i["tgt"], 100.0, None, "p2p", None, 6, trace=trace))
    _icp_rule(res[4], res[5], O.registration_icp(i["src"], i["tgt"], 100.0, None, "p2plane", i["tn"], 6))
    _, ri, rd = trace[-1]
    ok = rd < 100.0 ** 2
    assert ok.any() and res[2].shape == ri.shape and res[3].shape == rd.shape
    assert np.array_equal(res[3] < 100.0 ** 2, ok) and np.array_equal(res[2][ok], ri[ok])
    assert np.allclose(res[3][ok], rd[ok], rtol=1e-9, atol=1e-9)          # test_icp_engines_agree's rule for d2 within max_dist


add("icp", _pair_make, _icp_run, _icp_check)


def _icp_batch_make(size):
    """three sources of unequal sizes onto one target (test_icp_batch_equals_single_problems)"""
    i = _pair_make(size)
    s = i["src"]
    i["srcs"] = [s, np.ascontiguousarray(s[: len(s) // 2 + 1]), np.ascontiguousarray(O.transform(s, synth.t_star())[: 2 * len(s) // 3])]
    i["inits"] = [np.eye(4), np.eye(4), np.linalg.inv(synth.t_star())]
    return i


def _icp_batch_run(i):
    ops = _ops()
    out = ()
    for mode, nrm in (("p2p", None), ("p2plane", i["tn"])):
        for r in ops.icp_batch(i["srcs"], i["tgt"], 100.0, i["inits"], mode, nrm, 6):
            out += _reg_tuple(r)
    return out


def _icp_batch_check(res, i):
    k = 0
    for mode, nrm in (("p2p", None), ("p2plane", i["tn"])):
        for s, i0 in zip(i["srcs"], i["inits"]):
            _icp_rule(res[k], res[k + 1], O.registration_icp(s, i["tgt"], 100.0, i0, mode, nrm, 6))
            k += 2


add("icp_batch", _icp_batch_make, _icp_batch_run, _icp_batch_check)


def _fpfh_make(size):
    n = _n(size, large=3001, small=SMALL)
    p = subset(n, 9)
    radius = 250.0 if n > 1000 else 2500.0
    return dict(p=p, nrm=O.estimate_normals(p, radius / 2.5, 40)[0].astype(np.float32), radius=radius, nn=40)


def _fpfh_check(res, i):
    """tests/test_global_registration_gpu.py: check_fpfh over the oracle's neighbour lists"""
    import globalreg_ref as R
    want, _ = O.fpfh(i["p"], i["nrm"], i["radius"], i["nn"])
    nbr, cnt, d2 = O.hybrid_knn_d2(i["p"], i["radius"], max(1, min(i["nn"], len(i["p"]))))
    R.check_fpfh(res[0], want, R.fpfh_edge_flags(i["p"], i["nrm"], nbr, cnt), nbr, cnt, d2)


add("fpfh", _fpfh_make, lambda i: (npy(_ops().fpfh(i["p"], i["nrm"], i["radius"], i["nn"])),), _fpfh_check)


def _feat_make(size):
    """33-D features: the oracle's FPFH of two clouds (test_feature_matching_and_ransac_match_oracle) -- rows of different counts"""
    a, b = _fpfh_make(size), _fpfh_make(size)
    fa = O.fpfh(a["p"], a["nrm"], a["radius"], a["nn"])[0]
    return dict(fa=fa, fb=np.ascontiguousarray(fa[::-1][: 2 * len(fa) // 3 + 1] + np.random.default_rng(2).random((2 * len(fa) // 3 + 1, 33))))


add("feature_nn", _feat_make, lambda i: (npy(_ops().feature_nn(i["fa"], i["fb"])),), lambda res, i: eq(res[0], O.feature_nn(i["fa"], i["fb"])))


def _corres_make(size, large=2000, small=SMALL):
    import globalreg_ref as R
    nc = _n(size, large, small)
    src, tgt, corr = R.corres_scene(base_cloud(), max(3000, nc), 0.5, 0.0, nc, 11)
    return dict(src=src, tgt=tgt, corr=corr)


def _ransac_run(i):
    g = _ops().ransac_corres(i["src"], i["tgt"], i["corr"], 75.0, 3, 0.95, 40000, 0.999, 1)
    return g["transformation"], np.array([g["fitness"], g["inlier_rmse"], float(g["iterations"]), float(g["validations"])])


def _ransac_check(res, i):
    """test_feature_matching_and_ransac_match_oracle"""
    oT, ost = O.ransac_corres(i["src"], i["tgt"], i["corr"], 75.0, 3, 0.95, 40000, 0.999, 1)
    assert res[1][2] == ost["iterations"] and res[1][3] == ost["validations"]
    assert res[1][0] == ost["fitness"] and abs(res[1][1] - ost["rmse"]) < 1e-9
    assert np.abs(res[0] - oT).max() < 1e-6


add("ransac_corres", _corres_make, _ransac_run, _ransac_check)


def _tuple_check(res, i):
    """tests/test_fgr_gpu.py: test_tuple_test_equals_restatement"""
    import fgr_ref as F
    eq(res[0], F.tuple_test(i["src"], i["tgt"], i["corr"], 0.95, 1000, 5))


add("fgr_tuple_test", _corres_make, lambda i: (npy(_ops().fgr_tuple_test(i["src"], i["tgt"], i["corr"], 0.95, 1000, 5)),), _tuple_check)


def _fgr_run(i):
    g = _ops().fgr_optimize(i["src"], i["tgt"], i["corr"], iteration_number=16)
    return g["transformation"], np.array([g["par"], float(g["iterations"]), float(g["failed_solves"]), g["scale"]])


def _fgr_check(res, i):
    """tests/test_fgr_gpu.py: _check_optimize"""
    import fgr_ref as F
    ref, spread = F.permutation_spread(i["src"], i["tgt"], i["corr"], 4, iteration_number=16)
    T, (par, its, failed, scale) = res
    assert np.all(np.isfinite(T)) and F.transform_difference(T, ref["transformation"], ref["scale"]) <= max(10.0 * spread, 1e-12)
    assert (its, failed) == (ref["iterations"], ref["failed_solves"])
    assert (par <= 0.025) == (ref["par"] <= 0.025) and abs(par - ref["par"]) <= 1e-15 * ref["par"]
    assert scale == ref["scale"] and np.array_equal(T[3], [0, 0, 0, 1])


add("fgr_optimize", functools.partial(_corres_make, large=1025), _fgr_run, _fgr_check)


@functools.lru_cache(maxsize=None)
def _coloured(n):
    return synth.coloured_pair(n)


def _coloured_make(size):
    n = _n(size, large=3001, small=200)
    src, sc, tgt, tc, T = _coloured(n)
    radius = 70.0 if n > 1000 else 400.0
    tn = O.estimate_normals(tgt, radius, 30)[0].astype(np.float32)
    return dict(src=src, sc=sc, tgt=tgt, tc=tc, T=T, tn=tn, radius=2 * radius + 20.0)


def _gradient_check(res, i):
    """test_colour_gradient_and_coloured_icp_match_oracle"""
    assert np.allclose(res[0], O.color_gradient(i["tgt"], i["tn"], i["tc"], i["radius"], 30), rtol=1e-7, atol=1e-10)


add("color_gradient", _coloured_make, lambda i: (npy(_ops().color_gradient(i["tgt"], i["tn"], i["tc"], i["radius"], 30)),), _gradient_check)


def _cicp_check(res, i):
    rT, rf, rr, rit = O.registration_colored_icp(i["src"], i["sc"], i["tgt"], i["tc"], i["tn"], 80.0, None, 0.968, 6)
    assert res[1][2] == rit and res[1][0] == rf and abs(res[1][1] - rr) < 1e-8
    assert np.abs(res[0] - rT).max() < TOL_T


add("colored_icp", _coloured_make, lambda i: _reg_tuple(_ops().colored_icp(i["src"], i["sc"], i["tgt"], i["tc"], i["tn"], 80.0, None, 0.968, 6)),
    _cicp_check)


def _cov_make(size):
    n = _n(size, large=3001, small=SMALL)
    return dict(p=subset(n, 7), radius=60.0 if n > 1000 else 1e150, nn=30)


def _cov_check(res, i):
    """tests/test_gicp_gpu.py: test_estimate_covariances_matches_restatement"""
    import gicp_ref as G
    p, g = i["p"], res[0]
    ref = G.estimate_covariances(O, p, i["radius"], i["nn"])
    nbr, cnt = O.hybrid_knn(p, i["radius"], i["nn"])
    p64 = p.astype(np.float64)
    mu = np.stack([p64[nbr[r, :cnt[r]]].mean(0) if cnt[r] else np.zeros(3) for r in range(len(p))])
    tol = 1e-9 * np.linalg.norm(ref, axis=(1, 2)) + 1e-12 * (mu * mu).sum(1)
    assert g.shape == (len(p), 3, 3) and (np.abs(g - ref).max(axis=(1, 2)) <= tol).all()
    assert np.array_equal(g, np.transpose(g, (0, 2, 1)))
    assert np.array_equal(g[cnt < 3], np.broadcast_to(np.eye(3), g[cnt < 3].shape))


add("estimate_covariances", _cov_make, lambda i: (npy(_ops().estimate_covariances(i["p"], i["radius"], i["nn"])),), _cov_check)


def _gicp_make(size):
    import gicp_ref as G
    i = _pair_make(size)
    i["cs"], i["ct"] = G.estimate_covariances(O, i["src"], 1e150, 30), G.estimate_covariances(O, i["tgt"], 1e150, 30)
    return i


def _gicp_check(res, i):
    """tests/test_gicp_gpu.py: test_generalized_icp_matches_restatement"""
    import gicp_ref as G
    rT, rf, rr, rit, (ri, rd) = G.registration_generalized_icp(O, i["src"], i["tgt"], 100.0, i["cs"], i["ct"], None, 6)
    assert res[1][2] == rit and res[1][0] == rf and abs(res[1][1] - rr) < 1e-8
    assert np.abs(res[0] - rT).max() < TOL_T
    ok = rd < 100.0 ** 2
    assert np.array_equal(res[3] < 100.0 ** 2, ok) and np.array_equal(res[2][ok], ri[ok])


add("generalized_icp", _gicp_make,
    lambda i: _reg_tuple(_ops().generalized_icp(i["src"], i["cs"], i["tgt"], i["ct"], 100.0, None, 6, want_corr=True), True), _gicp_check)


# ============================================================================================ the frame (tests/test_parity_gpu.py)
def _frame_make(size):
    """two sensors, one frame: the smallest ring of the parity suite, at synth.small_xy(2) (92160 pixels a sensor, the parity suite's)
    and at synth.small_xy() (23040 pixels, 2333 output points).  Not smaller: at small_xy(6) and small_xy(8) the registration clouds
    hold a few hundred points and the 6 x 6 solve is conditioned so badly that the library -- the native frame and the Python pipeline
    alike, over poisoned scratch or not, the same bits -- and the oracle agree on the transforms to 8e-8 and 1e-7 only, beyond the
    parity suite's 1e-8, and three output coordinates move by a float32 ulp (measured on MI355X; 2e-13 at small_xy())"""
    from kinectpy_amd.pipeline import PipelineParams
    xy, depth, rgb, inits, _ = synth.sensor_ring(2, 1, synth.small_xy({"large": 2, "small": 4}[size]))
    return dict(xy=xy, depth=depth[0], rgb=rgb[0], inits=inits, params=PipelineParams())


def _frame_run(i):
    from kinectpy_amd.pipeline import NativeFramePipeline
    gp, gc, gT = NativeFramePipeline(i["xy"], 2, i["inits"], i["params"]).step(cuda(i["depth"]), cuda(i["rgb"]))
    return npy(gp), npy(gc), gT


def _frame_check(res, i):
    """test_native_frame_step_equals_python_pipeline_and_oracle"""
    rp, rc, rT, _ = O.pipeline_step(i["xy"], i["depth"], i["rgb"], i["inits"], i["params"])
    eq(res[0], rp), eq(res[1], rc)
    assert np.abs(res[2] - np.stack(rT)).max() < TOL_T


add("frame_step", _frame_make, _frame_run, _frame_check)


# ============================================================== meshes (tests/test_mesh_ops_gpu.py, test_tsdf_mesh_gpu.py, test_mesh_checks_gpu.py)
def bit_eq(got, want, what=""):
    """the mesh suites' same(): shape, dtype and bits"""
    if want is None:
        assert got is None or len(got) == 0, what
        return
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got.reshape(-1) != want.reshape(-1))[:5].tolist())


MESH_LARGE, MESH_SMALL = "res-24", "cut-8-40"          # 13918 vertices, 16548 triangles (eight 2048-item tiles and a tail); 40 triangles


def _mesh_make(size, large=MESH_LARGE, small=MESH_SMALL):
    import test_mesh_ops_gpu as T
    import tsdf_mesh_ref as M
    v, c, t = T.case({"large": large, "small": small}[size])
    rng = np.random.default_rng(len(t))
    return dict(v=v, c=c, t=t, vn=M.vertex_normals(v, t), tn=M.triangle_normals(v, t), tkeep=rng.random(len(t)) >= 0.4, vkeep=rng.random(len(v)) >= 0.2)


def _mesh_normals_check(res, i):
    import tsdf_mesh_ref as M
    for k, normalized in enumerate((True, False)):
        bit_eq(res[2 * k], M.triangle_normals(i["v"], i["t"], normalized)), bit_eq(res[2 * k + 1], M.vertex_normals(i["v"], i["t"], normalized))


add("mesh_normals", _mesh_make, lambda i: tuple(npy(a) for nz in (True, False) for a in _ops().mesh_normals(i["v"], i["t"], nz)), _mesh_normals_check)


def _mesh_ref(fn):
    def check(res, i):
        import mesh_ops_ref as R
        want = fn(R, i)
        assert len(res) == len(want)
        for k, (g, w) in enumerate(zip(res, want)):
            bit_eq(g, w, k)
    return check


add("_mesh_adjacency", _mesh_make, lambda i: tuple(npy(a) for a in _ops().mesh_adjacency(i["v"], i["t"])),
    _mesh_ref(lambda R, i: R.adjacency(i["t"], len(i["v"]))))
add("mesh_non_manifold_edges", _mesh_make, lambda i: tuple(npy(_ops().mesh_non_manifold_edges(i["v"], i["t"], a)) for a in (True, False)),
    lambda res, i: [eq(res[k], __import__("mesh_ops_ref").non_manifold_edges(i["t"], a).reshape(-1, 2)) for k, a in enumerate((True, False))])
add("mesh_cluster_triangles", _mesh_make, lambda i: tuple(npy(a) for a in _ops().mesh_cluster_triangles(i["v"], i["t"])),
    _mesh_ref(lambda R, i: R.cluster_connected_triangles(i["v"], i["t"])))
add("mesh_select_triangles", _mesh_make, lambda i: tuple(npy(a) for a in _ops().mesh_select_triangles(i["t"], i["tkeep"], False, i["tn"])),
    _mesh_ref(lambda R, i: R.remove_triangles(i["t"], ~i["tkeep"], i["tn"])))
add("mesh_select_vertices", _mesh_make,
    lambda i: tuple(npy(a) for a in _ops().mesh_select_vertices(i["v"], i["t"], i["vkeep"], False, i["c"], i["vn"], i["tn"])),
    _mesh_ref(lambda R, i: R.remove_vertices(i["v"], i["t"], ~i["vkeep"], i["c"], i["vn"], i["tn"])))
add("mesh_smooth", _mesh_make, lambda i: tuple(npy(a) for a in _ops().mesh_smooth(i["v"], i["t"], "taubin", 2, normals=i["vn"], colors=i["c"])),
    _mesh_ref(lambda R, i: R.smooth(i["v"], i["t"], "taubin", 2, normals=i["vn"], colors=i["c"])))


def _mesh_sample_run(i):
    n = 2 * TILE + 3 if len(i["t"]) > 1000 else 65
    return tuple(npy(a) for a in _ops().mesh_sample_points(i["v"], i["t"], n, 5, colors=i["c"], vertex_normals=i["vn"]))


add("mesh_sample_points", _mesh_make, _mesh_sample_run,
    _mesh_ref(lambda R, i: R.sample_points_uniformly(i["v"], i["t"], 2 * TILE + 3 if len(i["t"]) > 1000 else 65, 5, colors=i["c"],
                                                     vertex_normals=i["vn"])[:3]))


def _checks_make(size, large="res-24", small="cut-40"):
    import test_mesh_checks_gpu as T
    v, t = T.mesh({"large": large, "small": small}[size])
    return dict(v=v, t=t, tn=np.random.default_rng(len(t)).normal(size=(len(t), 3)).astype(np.float32))


def _checks_ref(fn):
    def check(res, i):
        import mesh_checks_ref as R
        want = fn(R, i)
        assert len(res) == len(want)
        for k, (g, w) in enumerate(zip(res, want)):
            bit_eq(g, np.asarray(w), k)
    return check


add("mesh_non_manifold_vertices", _checks_make, lambda i: (npy(_ops().mesh_non_manifold_vertices(i["v"], i["t"])),),
    _checks_ref(lambda R, i: (R.non_manifold_vertices(i["t"], len(i["v"])),)))


def _orientation_run(i):
    """the query, then the flips applied in place to device copies"""
    ops = _ops()
    ok, flip, _, _ = ops.mesh_orientation(i["v"], i["t"])
    ok2, _, tri, tn = ops.mesh_orientation(i["v"], cuda(i["t"]), True, cuda(i["tn"]))
    return np.array([ok, ok2]), npy(flip).astype(bool), npy(tri), npy(tn)


def _orientation_want(R, i):
    ok, flip = R.orientation(i["t"])
    rok, rt, rtn = R.orient_triangles(i["t"], i["tn"])
    return np.array([ok, rok]), flip, rt, rtn


add("mesh_orientation", functools.partial(_checks_make, large="fan"), _orientation_run, _checks_ref(_orientation_want))
add("mesh_volume", _checks_make, lambda i: (np.float64(_ops().mesh_volume(i["v"], i["t"])),), _checks_ref(lambda R, i: (np.float64(R.volume(i["v"], i["t"])),)))
add("mesh_edge_count", _checks_make, lambda i: (np.int64(_ops().mesh_edge_count(i["v"], i["t"])),),
    lambda res, i: eq(res[0], __import__("mesh_checks_ref").edge_count(i["t"])))


# ============================================================================= ray casting scenes (tests/test_raycast_gpu.py, test_mesh_checks_gpu.py)
_RAY_KEYS = ("t", "t_hit", "primitive_uvs", "primitive_normals", "geometry_ids", "primitive_ids")
_CLOSEST_KEYS = ("d2", "points", "distance", "geometry_ids", "primitive_ids")


def _scene_make(size):
    import test_raycast_gpu as T
    v, t = T.mesh({"large": "res-24", "small": "cut-3"}[size])
    return dict(v=v, t=t, rays=T.make_rays(v, t, 130), q=T.make_queries(v, t, 70))


def _scene_run(i):
    """the build, then one query of each kind on the built buffer"""
    ops = _ops()
    s = ops.rayscene_build(i["v"], i["t"])
    cast, closest = ops.rayscene_cast(s, i["rays"]), ops.rayscene_closest(s, i["q"])
    return (tuple(npy(cast[k]) for k in _RAY_KEYS) + tuple(npy(closest[k]) for k in _CLOSEST_KEYS)
            + (npy(ops.rayscene_count(s, i["rays"])), npy(ops.rayscene_occluded(s, i["rays"]))))


def _scene_check(res, i):
    """tests/test_raycast_gpu.py: assert_rays, assert_closest"""
    import raycast_ref as R
    ref = R.Scene([(i["v"], i["t"])])
    cast, closest = R.cast_rays(ref, i["rays"]), R.closest_points(ref, i["q"])
    for k, name in enumerate(_RAY_KEYS):
        bit_eq(res[k], cast[name], name)
    for k, name in enumerate(_CLOSEST_KEYS):
        bit_eq(res[6 + k], closest[name], name)
    eq(res[11], R.count_intersections(ref, i["rays"])), eq(res[12] != 0, R.test_occlusions(ref, i["rays"]))


add("rayscene_build", _scene_make, _scene_run, _scene_check)


def _pairs_run(i):
    ops = _ops()
    return (npy(ops.rayscene_triangle_pairs(ops.rayscene_build(i["v"], i["t"]), i["v"], i["t"], True)),)


# ================================================================ clusters, keypoints, samples, searches (the suites named in the checks)
def _permuted_subset(size, seed=5):
    """tests/test_cluster_gpu.py: a sorted subset of the frame cloud (integer millimetres), permuted; the median spacing"""
    from scipy.spatial import cKDTree
    n = _n(size)
    rng = np.random.default_rng(seed)
    b = base_cloud()
    pts = b[np.sort(rng.choice(len(b), n, replace=False))][rng.permutation(n)]
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=2)
    return dict(p=np.ascontiguousarray(pts), eps=float(np.round(1.5 * float(np.median(d[:, 1])), 1)) or 0.5)


def _dbscan_run(i):
    labels, cnt = _ops().cluster_dbscan(i["p"], i["eps"], 5)
    return npy(labels), npy(cnt)


def _dbscan_check(res, i):
    """tests/test_cluster_gpu.py: _check"""
    import dbscan_ref as R
    ref = R.dbscan_loop(*R.integer_neighbours(i["p"], i["eps"]), 5)
    eq(res[0], ref)
    assert res[1][0] == ref.max(initial=-1) + 1


add("cluster_dbscan", _permuted_subset, _dbscan_run, _dbscan_check)


def _radius_outlier_check(res, i):
    """tests/test_cluster_gpu.py: test_radius_outlier_matches_counts"""
    import dbscan_ref as R
    eq(res[0], np.flatnonzero(R.counts(R.integer_neighbours(i["p"], i["eps"])[0]) > 3))


add("remove_radius_outlier", _permuted_subset, lambda i: (npy(_ops().remove_radius_outlier(i["p"], 3, i["eps"])),), _radius_outlier_check)


def _slab_cloud_make(size):
    """tests/iss_ref.py: bumpy_slab, the cloud of the end-to-end ISS tests (7200 points; 36)"""
    import iss_ref as R
    p = R.bumpy_slab(*{"large": (60, 40, 3), "small": (6, 6, 1)}[size], seed=6)
    return dict(p=p, rs=3.3, rn=2.1, sal=np.random.default_rng(3).uniform(0.1, 1.0, len(p)))


def _saliency_check(res, i):
    """tests/test_iss_gpu.py: test_saliency_parity_and_suppression_of_it"""
    import iss_ref as R
    p, got = i["p"], res[0]
    ref = R.saliency(p, R.radius_pairs(p, i["rs"]))
    dec = ref["decided"]
    assert dec.any() and np.isfinite(got).all()
    zero_ref = ref["s"] == 0
    eq((got == 0)[dec], zero_ref[dec])
    nz = dec & ~zero_ref
    assert np.all(np.abs(got - ref["s"])[nz] <= R.tolerance(ref["e"][nz, 2], p[nz].astype(np.float64)))


add("iss_saliency", _slab_cloud_make, lambda i: (npy(_ops().iss_saliency(i["p"], i["rs"])),), _saliency_check)


def _nonmax_check(res, i):
    """tests/test_iss_gpu.py: _nonmax_both"""
    import iss_ref as R
    keep, _ = R.nonmax(i["sal"], len(i["p"]), R.radius_pairs(i["p"], i["rn"]), 5)
    eq(res[0], np.flatnonzero(keep))


add("iss_nonmax", _slab_cloud_make, lambda i: (npy(_ops().iss_nonmax(i["p"], i["sal"], i["rn"], 5)),), _nonmax_check)


def _resolution_check(res, i):
    """tests/test_iss_gpu.py: test_keypoints_default_radii_and_resolution"""
    import iss_ref as R
    want = R.resolution(i["p"])
    assert abs(float(res[0][0]) - want) <= 1e-12 * want


add("model_resolution", _slab_cloud_make, lambda i: (npy(_ops().model_resolution(i["p"])),), _resolution_check)


def _keypoints_run(i):
    idx, sal = _ops().iss_keypoints(i["p"], i["rs"], i["rn"], want_saliency=True)
    return npy(idx), npy(sal)


def _keypoints_check(res, i):
    """tests/test_iss_gpu.py: _end_to_end -- the keypoint flags on the points no rounding can move"""
    import iss_ref as R
    ref = R.iss_keypoints(i["p"], i["rs"], i["rn"])
    got, n = res[0], len(i["p"])
    assert got.dtype == np.int32 and np.all(np.diff(got) > 0) and (len(got) == 0 or (got[0] >= 0 and got[-1] < n))
    safe = R.safe_points(ref, i["p"], 5)
    is_kp = np.zeros(n, bool)
    is_kp[got] = True
    assert safe.any() and np.array_equal(is_kp[safe], ref["keep"][safe])
    assert np.isfinite(res[1]).all()


add("iss_keypoints", _slab_cloud_make, _keypoints_run, _keypoints_check)

FPS_BLOCK_MAX_N = _define("KPX_FPS_BLOCK_MAX_N")          # the one-block form up to here, the chain of blocks (candidate slots in scratch) beyond


def _fps_make(size):
    """tests/test_fps_gpu.py: integer millimetres, where the library's distance equals the restated loop's sum"""
    n = _n(size, large=FPS_BLOCK_MAX_N + 857)
    return dict(p=subset(n, 9), k=min(40, n), start=n // 2,
                clouds=[subset(n, 1), subset(max(n // 9, 2), 2), subset(max(n // 3, 3), 3)])          # ("one": 1, 2 and 3 points, k = 1)


def _fps_run(i):
    sel, cover = _ops().farthest_point_sample(i["p"], i["k"], i["start"], want_cover=True)
    return npy(sel), npy(cover)


def _fps_check(res, i):
    import fps_ref as R
    R.assert_squares_exact(i["p"])
    rs, rc = R.fps(i["p"], i["k"], i["start"])
    eq(res[0], rs), bit_eq(res[1], rc)


add("farthest_point_sample", _fps_make, _fps_run, _fps_check, ("large", "small", "one"))


def _fps_batch_check(res, i):
    import fps_ref as R
    k = min(20, min(len(c) for c in i["clouds"]))
    for c, cloud in enumerate(i["clouds"]):
        rs, rc = R.fps(cloud, k, 0)
        eq(res[0][c], rs), bit_eq(res[1][c], rc)


add("farthest_point_sample_batch", _fps_make,
    lambda i: tuple(npy(t) for t in _ops().farthest_point_sample_batch(i["clouds"], min(20, min(len(c) for c in i["clouds"])), 0)), _fps_batch_check, ("large", "small", "one"))


def _search_make(size):
    """tests/test_search_gpu.py: quantised coordinates, where the reference's sum and the library's fma chain are both exact; a third of
    the queries outside the cloud's box"""
    import search_ref as R
    n = _n(size)
    rng = np.random.default_rng(11 + n)
    pts = R.quantised(rng, n, [-40, -25, -10], [40, 25, 10])
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    c, e = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1.0)
    return dict(p=pts, q=R.quantised(rng, 3 * 64 + 9, c - 1.25 * e, c + 1.25 * e), r=6.0 if n > 100 else 20.0)


def _index_run(i):
    """the build, then one query of each kind on the built buffer"""
    ops = _ops()
    index = ops.search_index(i["p"])
    return (tuple(npy(t) for t in ops.search_knn(index, i["q"], 8)) + tuple(npy(t) for t in ops.search_hybrid(index, i["q"], i["r"], 10))
            + tuple(npy(t) for t in ops.search_radius(index, i["q"], i["r"])))


def _index_check(res, i):
    """tests/test_search_gpu.py: _same_knn, _same_csr"""
    import search_ref as R
    want = R.knn(i["p"], i["q"], 8) + R.knn(i["p"], i["q"], 10, i["r"]) + R.radius(i["p"], i["q"], i["r"])
    for k, (g, w) in enumerate(zip(res, want)):
        bit_eq(g, w, k)


add("search_index", _search_make, _index_run, _index_check, ("large", "small", "one"))


def _knn_run(i):
    ops = _ops()
    index = ops.search_index(i["p"])
    return tuple(npy(t) for t in ops.search_knn(index, i["q"], 33)) + tuple(npy(t) for t in ops.search_hybrid(index, i["q"], i["r"], 200))


def _knn_check(res, i):
    import search_ref as R
    for k, (g, w) in enumerate(zip(res, R.knn(i["p"], i["q"], 33) + R.knn(i["p"], i["q"], 200, i["r"]))):
        bit_eq(g, w, k)


add("_search_knn", _search_make, _knn_run, _knn_check, ("large", "small", "one"))


def _radius_run(i):
    ops = _ops()
    return tuple(npy(t) for t in ops.search_radius(ops.search_index(i["p"]), i["q"], 2 * i["r"]))


def _radius_check(res, i):
    import search_ref as R
    for k, (g, w) in enumerate(zip(res, R.radius(i["p"], i["q"], 2 * i["r"]))):
        bit_eq(g, w, k)


add("search_radius", _search_make, _radius_run, _radius_check, ("large", "small", "one"))


def _obb_make(size):
    """test_hull_vertices_bit_exact_and_obb: three clouds of one size; points on a sphere -- every one a hull vertex, so that at 3000
    points the hull's edge set (5996 facets) leaves LDS for the table in scratch"""
    n = _n(size, large=3000, small=9)
    rng = np.random.default_rng(11 + n)
    s = rng.normal(size=(3, n, 3))
    x = (s / np.linalg.norm(s, axis=2)[:, :, None]).astype(np.float32)
    x[1] = (rng.normal(size=(n, 3)) * [300, 900, 200]).astype(np.float32)
    return dict(x=x)


def _obb_run(i):
    obb, flags = _ops().obb_batch(torch.as_tensor(i["x"]), want_vertices=True)
    return npy(obb), npy(flags)


def _obb_check(res, i):
    for c, p in enumerate(i["x"]):
        ref = O.hull_vertices(p)
        eq(np.flatnonzero(res[1][c]), ref, c)
        row = res[0][c]
        assert row[15] == len(ref)
        if c == 1:                                               # (the spheres' covariances have no eigenvalue gap: their axes are not compared)
            R_, ctr, ext = O.obb_from_vertices(p[ref])
            assert np.allclose(row[:9].reshape(3, 3), R_, atol=1e-7)
            assert np.allclose(row[9:12], ctr, atol=1e-7 * np.abs(p).max()) and np.allclose(row[12:15], ext, rtol=1e-7)
        else:
            assert np.isfinite(row).all()


add("obb_batch", _obb_make, _obb_run, _obb_check)


# ================================================================================================ occupancy grids (tests/test_voxelgrid_gpu.py)
def _grid_cloud_make(size):
    import test_voxelgrid_gpu as T
    pts, col, v = T.cases()[{"large": "ring", "small": "normal63", "one": "normal1"}[size]]
    return dict(p=pts, col=col, v=50.0 if size == "large" else v)


def _grid_cloud_run(i):
    """the build, then the one query there is on its keys"""
    ops = _ops()
    keys, col, origin = ops.voxelgrid_from_cloud(i["p"], i["v"], i["col"])
    return npy(keys), npy(col), origin, npy(ops.voxelgrid_included(keys, origin, i["v"], i["p"][::3]))


def _grid_cloud_check(res, i):
    import voxelgrid_ref as R
    idx, rc, origin = R.create_from_point_cloud(i["p"], i["v"], i["col"])
    eq(res[0], R.keys_of(idx)), bit_eq(res[1], rc), eq(res[2], origin)
    eq(res[3] != 0, R.included(idx, origin, i["v"], i["p"][::3]))


add("voxelgrid_from_cloud", _grid_cloud_make, _grid_cloud_run, _grid_cloud_check, ("large", "small", "one"))


def _carve_make(size):
    """a dense grid of the suite (33 x 17 x 65 = 36465 voxels; 27) and the ring's four uint16 depth frames"""
    import test_voxelgrid_gpu as T
    import voxelgrid_ref as R
    idx, col, origin, v = T.grid_def({"large": "dense33x17x65", "small": "dense3"}[size])
    depth, _, extr, _ = T.ring()
    return dict(idx=idx, col=col, origin=np.asarray(origin, dtype=np.float64), v=v, keys=R.keys_of(idx), depth=[depth[0, s] for s in range(4)], extr=extr)


def _carve_run(i):
    import test_voxelgrid_gpu as T
    keys, col = cuda(i["keys"]), cuda(i["col"])
    out = ()
    for outside, unmeasured in ((False, False), (True, True)):
        k, c = _ops().voxelgrid_carve(keys, col, i["origin"], i["v"], "depth", [torch.as_tensor(d) for d in i["depth"]], T.W, T.H, T.K4, i["extr"],
                                      outside, unmeasured, T.SCALE, T.TRUNC)
        out += (npy(k), npy(c))
    return out


def _carve_check(res, i):
    import test_voxelgrid_gpu as T
    import voxelgrid_ref as R
    ims = [R.depth_from_u16(d, T.SCALE, T.TRUNC).reshape(T.H, T.W) for d in i["depth"]]
    for k, (outside, unmeasured) in enumerate(((False, False), (True, True))):
        alive = R.carve_all(i["idx"], i["origin"], i["v"], ims, T.K4, i["extr"], "depth", outside, unmeasured)
        eq(res[2 * k], i["keys"][alive]), bit_eq(res[2 * k + 1], i["col"][alive])


add("voxelgrid_carve", _carve_make, _carve_run, _carve_check)


# ================================================================================ images and RGB-D odometry (tests/test_odometry_gpu.py)
ODO_LARGE, ODO_SMALL = "79x71", "65x65"          # 5609 pixels: 22 blocks of 256 and a tail, levels of odd sizes; 65 x 65: levels of four blocks and one


def _odo_fixture(size):
    import odometry_scenes as S
    return S.fixture({"large": ODO_LARGE, "small": ODO_SMALL}[size]), {"large": ODO_LARGE, "small": ODO_SMALL}[size]


def _image_make(size):
    f, _ = _odo_fixture("large" if size == "large" else "small")
    st = {"large": lambda: np.stack([f["Is"], f["It"], f["Ds"]]),                                    # three different images
          "small": lambda: np.stack([f["Is"][:5, :7], f["It"][:5, :7], f["Ds"][:5, :7]]),           # narrower than the seven taps
          "one": lambda: np.ascontiguousarray(f["Is"][:1, :1])[None]}[size]()                        # one pixel
    return dict(st=st)


def _image_check(res, i):
    """test_stack_of_different_images_through_every_operator"""
    import odometry_ref as R
    for k, code in enumerate(sorted(_ops().IMAGE_FILTERS.values())):
        for s in range(len(i["st"])):
            assert np.array_equal(res[k][s], R.image_filter(i["st"][s], code), equal_nan=True), (code, s)


add("image_filter", _image_make, lambda i: tuple(npy(_ops().image_filter(i["st"], code)) for code in sorted(_ops().IMAGE_FILTERS.values())), _image_check, ("large", "small", "one"))


def _levels_make(size):
    import odometry_ref as R
    import odometry_scenes as S
    f, name = _odo_fixture(size)
    return dict(name=name, lv=S.fixture_levels(name)[0], K=R.level_camera(f["K4"], 0), T=f["init"], dmax=f["opt"]["depth_diff_max"])


def _corr_check(res, i):
    """test_odometry_gpu.py: the correspondences of a level equal the restatement's"""
    import odometry_ref as R
    want = R.correspondence(i["K"], i["T"], i["lv"][1], i["lv"][3], i["dmax"])
    assert len(want) > 20
    bit_eq(res[0], want)


add("odometry_correspondence", _levels_make, lambda i: (npy(_ops().odometry_correspondence(i["lv"][1], i["lv"][3], i["K"], i["T"], i["dmax"])),), _corr_check)


def _iteration_run(i):
    g = _ops().odometry_iteration(*i["lv"], i["K"], i["T"], "hybrid", i["dmax"])
    return g["sums"], np.array([float(g["count"]), float(g["solved"])]), g["transformation"]


def _iteration_check(res, i):
    """test_one_iteration_equals_restatement"""
    import odometry_ref as R
    import odometry_scenes as S
    from test_odometry_gpu import tol as _odo_tol
    ref = S.fixture_iteration_reference(i["name"], R.HYBRID, 0, "init")
    sums, (count, solved), T = res
    assert count == ref["count"] and solved and ref["solved"]
    assert R.sums_difference(sums[:21], ref["sums"][:21]) <= _odo_tol(ref["spread_JTJ"])
    assert R.sums_difference(sums[21:27], ref["sums"][21:27]) <= _odo_tol(ref["spread_JTr"])
    assert float(np.abs(T - ref["T"]).max()) <= _odo_tol(ref["spread_T"])


add("odometry_iteration", _levels_make, _iteration_run, _iteration_check)


def _chain_make(size):
    """a batch of three pairs of one fixture, each from its own pose: source -> target, target -> source, and a pair whose source has
    no depth at all (it fails: the identities, as in test_batch_with_its_own_poses_masks_and_a_failing_pair)"""
    f, name = _odo_fixture(size)
    Is, Ds, It, Dt = f["Is"], f["Ds"], f["It"], f["Dt"]
    return dict(f=f, name=name, inits=np.stack([f["init"], np.linalg.inv(f["init"]), f["init"]]),
                Ds=np.stack([Ds, Dt, np.zeros_like(Ds)]), Is=np.stack([Is, It, Is]), Dt=np.stack([Dt, Ds, Dt]), It=np.stack([It, Is, It]))


def _chain_run(i):
    f = i["f"]
    n_px = f["W"] * f["H"]
    ok, T, G, n = _ops().rgbd_odometry(i["Ds"].reshape(3, n_px), i["Is"].reshape(3, n_px), i["Dt"].reshape(3, n_px), i["It"].reshape(3, n_px), f["W"], f["H"],
                                       f["K4"], i["inits"], "hybrid", (4, 3, 2), **f["opt"])
    return np.asarray(ok, dtype=bool), T, G, n


def _chain_check(res, i):
    """test_odometry_gpu.py: _compare_chain, every pair against the restatement of its own chain"""
    import odometry_ref as R
    import odometry_scenes as S
    from test_odometry_gpu import tol
    ok, T, G, n = res
    opt = S.fixture_option(i["name"], (4, 3, 2))
    success = []
    for p in range(3):
        ref = S._chain_reference(i["Is"][p], i["Ds"][p], i["It"][p], i["Dt"][p], i["f"]["K4"], i["inits"][p], R.HYBRID, opt, 3)
        success.append(ref["success"])
        assert bool(ok[p]) is ref["success"], p
        if not ref["success"]:
            assert np.array_equal(T[p], np.eye(4)) and np.array_equal(G[p], np.eye(6)) and n[p] == 0, p
            continue
        assert float(np.abs(T[p] - ref["T"]).max()) <= tol(ref["spread_T"]) and R.sums_difference(G[p], ref["info"]) <= tol(ref["spread_info"]), p
        Rm = T[p][:3, :3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and np.array_equal(T[p][3], [0, 0, 0, 1]) and np.array_equal(G[p], G[p].T) and n[p] > 500, p
    assert success == [True, True, False]


add("rgbd_odometry", _chain_make, _chain_run, _chain_check)


# ====================================================================================== normal orientation (tests/test_orient_gpu.py)
def _orient_make(size):
    import search_ref
    import test_orient_gpu as T
    n = _n(size, large=700)
    p = search_ref.quantised(np.random.default_rng(20 + n), n, -2, 2)
    nrm = T.quantised_normals(np.random.default_rng(n), n)
    nrm[3] = 0.0
    return dict(p=p, nrm=nrm, k=8)


def _emst_check(res, i):
    import orient_ref as R
    eq(res[0], R.emst(i["p"]))


add("emst", _orient_make, lambda i: (npy(_ops().emst(i["p"], i["k"])),), _emst_check)


def _tangent_run(i):
    got, flips, tree = _ops().orient_normals_tangent(cuda(i["p"]), cuda(i["nrm"]), i["k"], want_flips=True, want_tree=True)
    return npy(got), npy(flips), npy(tree)


def _tangent_check(res, i):
    """test_orient_gpu.py: the tree, the flips and the normals of the reference's walk over its own EMST and rows"""
    import orient_ref as R
    p = i["p"]
    want, want_flips, want_tree = R.tangent_from_graph(p, i["nrm"], R.emst(p), R.knn_rows(p, i["k"])[:, :min(i["k"], len(p))])
    eq(res[2], want_tree), eq(res[1], want_flips), bit_eq(res[0], want)


add("orient_normals_tangent", _orient_make, _tangent_run, _tangent_check)


# ============================================================================ PointNet (tests/test_pointnet_gpu.py, test_pointnet_train_gpu.py)
def _pn_make(size):
    import pointnet_ref as R
    B, N, J = {"large": (5, 3 * 64 + 8, 3), "small": (2, 5, 3)}[size]          # the 64-point tile: three and a tail; less than one
    x, y64, tau = R.case(B, N, J, R.UNIT)
    return dict(x=np.array(x), y64=y64, tau=tau, folded=list(R.model(J)[1]))


def _pn_run(i):
    import pointnet_ref as R
    ops = _ops()
    y, st = ops.pointnet_forward(ops.pointnet_pack(i["folded"]), cuda(i["x"]), want_stages=True)
    got = dict({k: npy(v) for k, v in st.items()}, joints=npy(y))
    return tuple(got[k] for k in R.STAGES)


def _pn_check(res, i):
    """test_pointnet_gpu.py: check"""
    import pointnet_ref as R
    for g, k in zip(res, R.STAGES):
        assert g.dtype == np.float32 and g.shape == i["y64"][k].shape, k
        assert np.isfinite(g).all() and R.rel_dev(g, i["y64"][k]) <= i["tau"][k], k


add("pointnet_forward", _pn_make, _pn_run, _pn_check)
PN_TRAIN = {"large": (32, 200), "small": (16, 1)}          # cases of tests/pointnet_train_ref.py that meet its input condition


def _pt_make(size):
    import pointnet_train_ref as T
    B, N = PN_TRAIN[size]
    w, x, y = T.case(B, N, 3)
    return dict(B=B, N=N, w=w, x=np.array(x), y=np.array(y), seed=T.seed_of(B, N))


def _pt_grad_run(i):
    ops = _ops()
    params = ops.pointnet_train_pack(i["w"])
    loss, grad, st = ops.pointnet_grad(params, cuda(i["x"]), cuda(i["y"]), seed=i["seed"], step=0, training_dropout=True, want_stages=True)
    return (npy(loss), npy(grad), npy(params)) + tuple(npy(st[k]) for k in ("i1", "i2", "i3", "T3", "T32", "g1", "g2", "g3", "out"))


def _pt_grad_rule(loss, grad, pool, i):
    """test_pointnet_train_gpu.py: check_gradients"""
    import pointnet_train_ref as T
    import test_pointnet_train_gpu as G
    r64, tau, tau_loss = T.reference(i["w"], i["x"], i["y"], T.masks_of(i["B"], i["N"]), list(pool))
    assert np.isfinite(grad).all() and np.isfinite(loss).all()
    dev = T.layer_dev(G.layers_of(grad, 3), r64["grads"])
    for l in range(20):
        assert dev[l] <= tau[l], (l, dev[l], tau[l])
    assert abs(float(loss[0]) - r64["loss"]) / abs(r64["loss"]) <= tau_loss
    assert abs(float(loss[1]) + float(loss[2]) - float(loss[0])) <= 2e-7 * abs(float(loss[0]))
    assert abs(float(loss[2]) - r64["reg"]) <= max(tau_loss * abs(r64["loss"]), 1e-6 * abs(r64["reg"]))


def _pt_grad_check(res, i):
    _pt_grad_rule(res[0], res[1], res[3:6], i)
    assert all(np.isfinite(a).all() for a in res[2:3] + res[6:])
    assert all(a.min() >= 0 and a.max() < i["N"] for a in res[3:6])


add("pointnet_grad", _pt_make, _pt_grad_run, _pt_grad_check)


def _pt_step_run(i):
    """the step; the pooled points its gradient is judged at come from a pointnet_grad of the same inputs"""
    ops = _ops()
    n = ops.pointnet_train_layout(3)[1]
    x, y = cuda(i["x"]), cuda(i["y"])
    p = ops.pointnet_train_pack(i["w"])
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    loss, grad = ops.pointnet_train_step(p, x, y, m, v, learning_rate=0.005, t=1, seed=i["seed"], step=0)
    st = ops.pointnet_grad(ops.pointnet_train_pack(i["w"]), x, y, seed=i["seed"], step=0, want_stages=True)[2]
    return (npy(loss), npy(grad), npy(p), npy(m), npy(v)) + tuple(npy(st[k]) for k in ("i1", "i2", "i3"))


def _pt_step_check(res, i):
    """the gradient by check_gradients' rule; w, m, v by test_adam_step_within_two_ulp_of_the_float64_formula"""
    import pointnet_train_ref as T
    import test_pointnet_train_gpu as G
    loss, grad, p, m, v = res[:5]
    _pt_grad_rule(loss, grad, res[5:8], i)
    n = len(grad)
    w0 = _ops().pointnet_train_pack_host(i["w"])[:n]
    for name, a, r in zip("wmv", (p[:n], m, v), T.adam(w0, grad, np.zeros(n, np.float32), np.zeros(n, np.float32), lr=0.005, t=1)):
        assert G._ulps(a, r).max() <= 2.0, name
    assert np.isfinite(p).all()


add("pointnet_train_step", _pt_make, _pt_step_run, _pt_step_check)

# "coincident": 200 copies of one triangle, 19900 pairs (nine 2048-pair tiles and a tail); "tetrahedra": 3 pairs
add("rayscene_triangle_pairs", functools.partial(_checks_make, large="coincident", small="tetrahedra"), _pairs_run,
    _checks_ref(lambda R, i: (R.triangle_pairs(i["v"], i["t"]),)))

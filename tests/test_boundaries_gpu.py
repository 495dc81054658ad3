"""GPU suite (-m gpu): the size and k thresholds at which the kernels switch form, crossed on purpose, against the C oracle and -- where
the oracle is too slow (clouds above 4M points) -- against the float64 sampled-row references of oracle/lineage2.py.

The functions below restate the library's switch conditions (kpx_knn.hip's SOR / normals cascades, kpx_voxel.hip's sort choice); each
case asserts, from its own inputs, which side of each threshold it sits on.  The limits the public header defines are read from
include/kinectpx.h; the others are restated here and must be moved with the library's."""
import os
import re

import numpy as np
import pytest
import torch

from kinectpy_amd.utils import synth
from oracle import lineage2 as L2

pytestmark = pytest.mark.gpu

TOL_STATS = L2.TOL_STATS
_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kinectpx.h")).read()
_define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, _HEADER).group(1))
RADIX_MAX_PAIRS = 2048 * 32 * 64          # kpx_radix.h kRadixMaxPairs: the library's own radix sort serves up to 4M pairs
GRID_OWN_SORT_MIN = 65536                 # kpx_knn.hip grid build: its own radix sort above 65536 points (counting build below)
VOXEL_READBACK_MIN = 128 * 1024           # kpx_voxel.hip voxel_batch_impl: the key width is read back above 131072 points
VOXEL_BATCH_MAX = 8                       # kpx_voxel.hip kVoxelBatchMax: clouds per concatenated pass
SOR_LDS_K, NORMALS_LDS_NN = _define("KPX_SOR_LDS_K"), _define("KPX_NORMALS_LDS_NN")    # the fall-back heaps: LDS up to here, workspace beyond
SOR_MAX_K, NORMALS_MAX_NN = _define("KPX_SOR_MAX_K"), _define("KPX_NORMALS_MAX_NN")
WORKERS = 16


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


def npy(t):
    return t.cpu().numpy()


def _heap_blocks(k, lds_k):
    b = 256
    while k > lds_k and b > 8 and b * 64 * k * 8 > (256 << 20):
        b >>= 1
    return b


def sor_form(k):
    """kpx_sor's cascade at k (KPX_SOR_* unset): pass 0 = the block-per-64-queries kernel (33 <= k <= 1024; staged S per query
    block), pass 1 = the wave-per-query kernel (k <= 512; 512- or 1024-candidate buffer), pass 2 (always), pass 3's heaps"""
    S = None if not 33 <= k <= 1024 else (8 if k <= 64 else 16 if k <= 128 else 32)
    return dict(block=S, pass1=(512 if k <= 32 else 1024) if k <= 512 else None,
                heap="lds" if k <= SOR_LDS_K else "workspace", heap_blocks=_heap_blocks(k, SOR_LDS_K))


def normals_form(nn):
    """estimate_normals' / the neighbour lists' form at max_nn: the wave pass (max_nn <= 512; 512- or 1024-candidate buffer) and
    the heap walk's heaps"""
    return dict(wave=(512 if nn <= 48 else 1024) if nn <= 512 else None,
                heap="lds" if nn <= NORMALS_LDS_NN else "workspace", heap_blocks=_heap_blocks(nn, NORMALS_LDS_NN))


def voxel_key_bits(clouds, voxel):
    """voxel_batch_key_bits for the row-major key (morton = 0: kpx_voxel_downsample and _batch): the bit length of
    count x DX x DY x DZ, DX.. the largest grid extents over the clouds"""
    d = np.ones(3)
    for c in clouds:
        if len(c) == 0:
            continue
        lo, hi = c.min(0).astype(np.float64), c.max(0).astype(np.float64)
        d = np.maximum(d, np.floor((hi - (lo - voxel * 0.5)) / voxel) + 1.0)
    rng = len(clouds) * int(d[0]) * int(d[1]) * int(d[2])
    return max(1, rng.bit_length())


def voxel_sort_form(clouds, voxel):
    """which sort voxel_batch_impl takes for one concatenated pass (no normals)"""
    total = sum(len(c) for c in clouds)
    if total <= VOXEL_READBACK_MIN:
        return "vendor-64"                                             # no read-back: 64-bit keys, all 64 bits sorted
    bits = voxel_key_bits(clouds, voxel)
    if bits > 32:
        return "vendor-64"
    return "own-32" if total <= RADIX_MAX_PAIRS else "vendor-32"


def _cov_matrix(cov):
    A = np.zeros((len(cov), 3, 3))
    A[:, 0, 0], A[:, 1, 1], A[:, 2, 2] = cov[:, 0], cov[:, 3], cov[:, 5]
    A[:, 0, 1] = A[:, 1, 0] = cov[:, 1]
    A[:, 0, 2] = A[:, 2, 0] = cov[:, 2]
    A[:, 1, 2] = A[:, 2, 1] = cov[:, 4]
    return A


def _normals_vs_oracle(gn, rn, cov, cnt, well_min):
    """the rule of test_large_neighbourhoods_beyond_the_lds_forms: same neighbour sets -> same normal up to sign where the eigengap
    is well conditioned"""
    w = np.linalg.eigvalsh(_cov_matrix(cov))
    well = (cnt >= 3) & ((w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-30))
    assert well.mean() > well_min
    assert (np.abs((gn * rn).sum(1))[well] > 1 - 1e-6).all()
    assert np.allclose(gn[cnt < 3], [0, 0, 1])


def _rows(n, m, seed):
    return np.sort(np.random.default_rng(seed).choice(n, min(n, m), replace=False))


@pytest.fixture(scope="module")
def halo_cloud():
    """frame density (a 30k sample of the rendered frame: the block kernel's dense cells) plus a sparse halo around it (queries
    whose k-th neighbour lies many cells away: the fall-back passes)"""
    rng = np.random.default_rng(41)
    base = synth.frame_cloud()
    p = base[rng.choice(len(base), 30000, replace=False)]
    lo, hi = p.min(0), p.max(0)
    halo = rng.uniform(lo - 500, hi + 500, size=(400, 3)).astype(np.float32)
    q = np.concatenate([p, halo])
    return np.ascontiguousarray(q[rng.permutation(len(q))])


# ---------------------------------------------------------------------------------------------- B: SOR k boundaries
SOR_CASES = [(32, None, 512, "lds"), (33, 8, 1024, "lds"), (64, 8, 1024, "lds"), (65, 16, 1024, "lds"), (128, 16, 1024, "lds"),
             (288, 32, 1024, "lds"), (289, 32, 1024, "workspace"), (512, 32, 1024, "workspace"), (513, 32, None, "workspace"),
             (1024, 32, None, "workspace"), (1025, None, None, "workspace"), (2049, None, None, "workspace"),
             (SOR_MAX_K, None, None, "workspace")]


@pytest.mark.parametrize("k,block,cap1,heap", SOR_CASES)
def test_sor_k_boundaries(ops, oracle, halo_cloud, k, block, cap1, heap):
    f = sor_form(k)
    assert (f["block"], f["pass1"], f["heap"]) == (block, cap1, heap)
    assert f["heap_blocks"] == (128 if k > 2048 else 256)              # 2048 | 2049: the workspace heaps halve their blocks
    p = halo_cloud
    ratio = 1.0 if k % 2 else 2.0
    gi, gs, ga = ops.sor(p, k, ratio, want_avg=True)
    ri, rs, ra = oracle.sor(p, k, ratio)
    assert np.array_equal(npy(gi), ri)
    assert np.allclose(npy(ga), ra, rtol=1e-14, atol=0)
    assert np.allclose(npy(gs), rs, rtol=TOL_STATS, atol=0)
    L2.check_sor_f64(p, k, ratio, npy(gi), npy(gs), npy(ga), _rows(len(p), 2000, k), workers=WORKERS)


# ---------------------------------------------------------------------------------------------- B: normals / neighbour lists
NORMALS_CASES = [(48, 300.0, 512, "lds"), (49, 300.0, 1024, "lds"), (128, 300.0, 1024, "lds"), (129, 300.0, 1024, "workspace"),
                 (512, 600.0, 1024, "workspace"), (513, 600.0, None, "workspace"), (2049, 1500.0, None, "workspace"),
                 (NORMALS_MAX_NN, 1500.0, None, "workspace")]


@pytest.mark.parametrize("nn,radius,wave,heap", NORMALS_CASES)
def test_normals_max_nn_boundaries(ops, oracle, halo_cloud, nn, radius, wave, heap):
    f = normals_form(nn)
    assert (f["wave"], f["heap"]) == (wave, heap) and f["heap_blocks"] == (128 if nn > 2048 else 256)
    p = halo_cloud
    gn = npy(ops.estimate_normals(p, radius, nn)).astype(np.float64)
    rn, cov, cnt = oracle.estimate_normals(p, radius, nn)
    assert cnt.max() == nn and cnt.min() < nn                          # the cap binds, and the radius cuts some neighbourhoods
    _normals_vs_oracle(gn, rn, cov, cnt, 0.6)
    assert L2.check_normals_f64(p, radius, nn, gn, _rows(len(p), 2000, nn), workers=WORKERS) > 0.5


@pytest.mark.parametrize("nn,radius", [(129, 600.0), (513, 1200.0)])
def test_fpfh_neighbour_lists_beyond_the_wave_pass(ops, oracle, halo_cloud, nn, radius):
    f = normals_form(nn)
    assert f["heap"] == "workspace" and (f["wave"] is None) == (nn > 512)
    q = halo_cloud[:3000]
    _, cnt = oracle.hybrid_knn(q, radius, nn)
    assert cnt.max() == nn
    nrm = npy(ops.estimate_normals(q, 150.0, 40))
    got = npy(ops.fpfh(q, nrm, radius, nn))
    want, _ = oracle.fpfh(q, nrm, radius, nn)
    bad = np.abs(got - want).max(1) > 1e-6                              # (a libm atan2 ulp can move one pair across a bin edge)
    assert bad.mean() < 2e-3 and np.allclose(got[~bad], want[~bad], rtol=1e-9, atol=1e-9)


def test_colour_gradient_beyond_the_wave_pass(ops, oracle):
    assert normals_form(513)["wave"] is None
    _, _, tgt, tc, _ = synth.coloured_pair(3000)
    _, cnt = oracle.hybrid_knn(tgt, 400.0, 513)
    assert cnt.max() == 513
    tn = oracle.estimate_normals(tgt, 70.0, 30)[0].astype(np.float32)
    g = npy(ops.color_gradient(tgt, tn, tc, 400.0, 513))
    rg = oracle.color_gradient(tgt, tn, tc, 400.0, 513)
    assert np.allclose(g, rg, rtol=1e-7, atol=1e-10)


# ---------------------------------------------------------------------------------------------- B: 65536 | 65537 (grid build)
@pytest.mark.parametrize("n", [GRID_OWN_SORT_MIN, GRID_OWN_SORT_MIN + 1])
def test_grid_build_sort_boundary_with_lattice_duplicates(ops, oracle, n):
    """the grid behind SOR and normals bins by counting up to 65536 points and sorts (own radix) above; integer-lattice points with
    exact duplicates among frame-density points, so the k-th distance is shared and cells hold blocks of coincident points"""
    rng = np.random.default_rng(n)
    base = synth.frame_cloud()
    g = np.arange(0, 30, dtype=np.float32) * 5.0
    lat = np.stack(np.meshgrid(g, g, g[:8], indexing="ij"), -1).reshape(-1, 3) + np.float32([-200, -300, 2500])
    lat = np.concatenate([lat, lat[rng.choice(len(lat), 3000)]])      # 3000 exact duplicates
    p = np.concatenate([base[rng.choice(len(base), n - len(lat), replace=False)], lat]).astype(np.float32)
    p = np.ascontiguousarray(p[rng.permutation(len(p))])
    assert len(p) == n and (len(p) > GRID_OWN_SORT_MIN) == (n == GRID_OWN_SORT_MIN + 1)
    for k, ratio in ((20, 2.0), (200, 1.0)):
        gi, gs, ga = ops.sor(p, k, ratio, want_avg=True)
        ri, rs, ra = oracle.sor(p, k, ratio)
        assert np.array_equal(npy(gi), ri) and np.allclose(npy(ga), ra, rtol=1e-14, atol=0), k
        assert np.allclose(npy(gs), rs, rtol=TOL_STATS, atol=0), k
    gn = npy(ops.estimate_normals(p, 40.0, 40)).astype(np.float64)
    rn, cov, cnt = oracle.estimate_normals(p, 40.0, 40)
    _normals_vs_oracle(gn, rn, cov, cnt, 0.5)


# ---------------------------------------------------------------------------------------------- B: 131072 | 131073 (voxel read-back)
@pytest.mark.parametrize("n", [VOXEL_READBACK_MIN, VOXEL_READBACK_MIN + 1])
def test_voxel_readback_boundary(ops, oracle, n):
    """up to 131072 points in all the one-pass form sorts 64-bit keys with the vendor sort; above, it reads the key width back and
    sorts <= 32-bit keys with its own radix sort.  One cloud, and a batch of two whose total sits at the same boundary."""
    c = synth.filter_cloud(n, seed=7)
    rng = np.random.default_rng(n)
    col = rng.random(c.shape).astype(np.float32)
    assert voxel_key_bits([c], 10.0) <= 32
    assert voxel_sort_form([c], 10.0) == ("vendor-64" if n == VOXEL_READBACK_MIN else "own-32")
    gp, _, _ = ops.voxel_downsample(c, 10.0)
    assert np.array_equal(npy(gp), oracle.voxel_downsample(c, 10.0)[0])
    a, b = c[: n // 3], np.ascontiguousarray(c[n // 3:] + np.float32(11.0))
    assert len(a) + len(b) == n and voxel_sort_form([a, b], 10.0) == voxel_sort_form([c], 10.0)
    got = ops.voxel_downsample_batch([a, b], 10.0, [col[: n // 3], col[n // 3:]])
    for (gp, gc), x, xc in zip(got, (a, b), (col[: n // 3], col[n // 3:])):
        rp, rc, _ = oracle.voxel_downsample(x, 10.0, xc)
        assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc)


# ---------------------------------------------------------------------------------------------- C: above kRadixMaxPairs
@pytest.fixture(scope="module")
def tiled_room():
    """five copies of a 1M-point config-3 room side by side in x (5,242,880 points)"""
    c = synth.filter_cloud(1 << 20, seed=5)
    return np.ascontiguousarray(np.concatenate([c + np.float32([5000.0 * i, 0, 0]) for i in range(5)]))


@pytest.mark.parametrize("n", [RADIX_MAX_PAIRS, RADIX_MAX_PAIRS + 1, 5_000_000])
def test_voxel_one_pass_above_the_own_sort(ops, oracle, tiled_room, n):
    """no normals: the one-pass form.  At 10 mm the keys fit 32 bits -- the own radix sort up to 4M points, the vendor sort of 32-bit
    keys above; at 1 mm they do not -- the vendor sort of 64-bit keys.  Bit-exact against the oracle."""
    p = tiled_room[:n]
    for voxel, form in ((10.0, "own-32" if n <= RADIX_MAX_PAIRS else "vendor-32"), (1.0, "vendor-64")):
        assert voxel_sort_form([p], voxel) == form, (n, voxel, voxel_key_bits([p], voxel))
        gp, _, _ = ops.voxel_downsample(p, voxel)
        rp, _, _ = oracle.voxel_downsample(p, voxel)
        assert np.array_equal(npy(gp), rp), (n, voxel)


def test_voxel_batch_in_the_a7_shape(ops, oracle):
    """bench.py --full's a7 leg scaled down: 17 coloured clouds of ~600k points -> two 8-cloud groups above 4M pairs (vendor sort of
    32-bit keys) and a one-cloud straggler group (own radix sort).  Every cloud bit-exact against the oracle."""
    base = synth.filter_cloud(600_000, seed=9)
    rng = np.random.default_rng(9)
    clouds = [np.ascontiguousarray(base[: 600_000 - 1000 * i] + np.float32([13.0 * i, -7.0 * i, 3.0 * i])) for i in range(17)]
    cols = [rng.random(c.shape).astype(np.float32) for c in clouds]
    groups = [clouds[g:g + VOXEL_BATCH_MAX] for g in range(0, len(clouds), VOXEL_BATCH_MAX)]
    assert [len(g) for g in groups] == [8, 8, 1]
    assert [voxel_sort_form(g, 10.0) for g in groups] == ["vendor-32", "vendor-32", "own-32"]
    got = ops.voxel_downsample_batch(clouds, 10.0, cols)
    for i, ((gp, gc), c, col) in enumerate(zip(got, clouds, cols)):
        rp, rc, _ = oracle.voxel_downsample(c, 10.0, col)
        assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc), i


@pytest.fixture(scope="module")
def big_room():
    """4.5M points of config 3 (dense floor, person and wall, 1 % outliers): the grid's cell table is capped at 4M cells, so cells
    overfill, and the grid build's point sort is the vendor's"""
    p = synth.filter_cloud(4_500_000, seed=13)
    from scipy.spatial import cKDTree
    return p, cKDTree(p.astype(np.float64))


@pytest.mark.parametrize("k,ratio", [(20, 2.0), (200, 1.0)])
def test_sor_above_four_million_points_f64(ops, big_room, k, ratio):
    p, tree = big_room
    assert len(p) > RADIX_MAX_PAIRS and len(p) >= 256 * 1024            # grid: vendor sort of the points, cell table at its 4M cap
    gi, gs, ga = ops.sor(p, k, ratio, want_avg=True)
    L2.check_sor_f64(p, k, ratio, npy(gi), npy(gs), npy(ga), _rows(len(p), 2000, k), workers=WORKERS, tree=tree)


def test_normals_above_four_million_points_f64(ops, big_room):
    p, tree = big_room
    assert len(p) > RADIX_MAX_PAIRS and normals_form(40)["wave"] == 512
    gn = npy(ops.estimate_normals(p, 70.0, 40))
    assert L2.check_normals_f64(p, 70.0, 40, gn, _rows(len(p), 2000, 40), workers=WORKERS, tree=tree) > 0.5


# ---------------------------------------------------------------------------------------------- D: stale bounds
def test_bounds_follow_normalise_and_scale():
    """PointCloud caches its bounds on the device; every replacement of its points must drop them"""
    from kinectpy_amd import o3d
    from kinectpy_amd.floor_removal import remove_floor
    from kinectpy_amd.utils import processing as P
    c = synth.filter_cloud(60_000, seed=21)
    pc = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(c))
    pc.get_min_bound(), pc.get_max_bound()                             # populate the cache
    P.normalize_pointcloud(pc)
    host = np.asarray(pc.points)
    assert np.array_equal(pc.get_min_bound(), host.min(0)) and np.array_equal(pc.get_max_bound(), host.max(0))
    src = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(c))
    src.get_max_bound()                                                # cached before the deep copy
    sc = P.scale_point_cloud(src, 0.5, 2.0, 0.25)
    host = np.asarray(sc.points)
    assert np.array_equal(sc.get_min_bound(), host.min(0)) and np.array_equal(sc.get_max_bound(), host.max(0))
    assert np.array_equal(src.get_max_bound(), c.max(0).astype(np.float64))
    # remove_floor reads max(y) from the cached bounds: on the normalised cloud it must equal remove_floor on a fresh cloud of the same points
    pts = np.asarray(pc.points).astype(np.float32)
    fresh = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(pts))
    a = remove_floor(pc, slab=0.05, distance_threshold=0.01, seed=3)
    b = remove_floor(fresh, slab=0.05, distance_threshold=0.01, seed=3)
    assert len(a.points) > 0 and np.array_equal(np.asarray(a.points), np.asarray(b.points))


# ---------------------------------------------------------------------------------------------- D: the frame loop's key-width speculation
def fused_key_bits(masked, Ts, voxel):
    """kpx_voxel.hip fuse_key_bits: the bit length of DX x DY x DZ over the box of the masked clouds moved in float64"""
    q = np.vstack([np.asarray(m, np.float64) @ np.asarray(T)[:3, :3].T + np.asarray(T)[:3, 3] for m, T in zip(masked, Ts)])
    lo, hi = q.min(0), q.max(0)
    d = np.floor((hi - (lo - voxel * 0.5)) / voxel) + 1.0
    return (int(d[0]) * int(d[1]) * int(d[2])).bit_length()


def test_frame_loop_fuse_width_speculation_across_frames(oracle):
    """kpx_frame_step speculates the fused cloud's sort-key width from the previous frame of the same host thread (whole 8-bit passes,
    <= 32 bits; wider keys are not speculated).  One thread steps a sequence of filter voxel sizes whose width rises within 32 bits (the
    speculation is too narrow: the frame is fused again), goes above 32 (too narrow again, then no speculation), and falls (a wider
    speculation than needed).  Every frame equals SensorShardPipeline bit for bit and the oracle step."""
    from kinectpy_amd.pipeline import NativeFramePipeline, PipelineParams, SensorShardPipeline
    xy, depth, rgb, inits, _ = synth.sensor_ring(4, 1)
    d, c = torch.as_tensor(depth[0]).cuda(), torch.as_tensor(rgb[0]).cuda()
    voxels, widths = (20.0, 5.0, 1.0, 0.25, 10.0, 20.0), []
    for voxel in voxels:
        prm = PipelineParams(filt_voxel=voxel)
        rp, rc, rT, mid = oracle.pipeline_step(xy, depth[0], rgb[0], inits, prm)
        widths.append(fused_key_bits([m[0] for m in mid["masked"]], rT, voxel))
        gp, gc, gT = NativeFramePipeline(xy, 4, inits, prm).step(d, c)
        pp, pc, pT = SensorShardPipeline(xy, 4, inits, prm).step(d, c)
        assert torch.equal(gp, pp) and torch.equal(gc, pc) and np.abs(gT - pT).max() < 1e-11, voxel
        assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc) and np.abs(gT - np.stack(rT)).max() < 1e-8, voxel
    spec = [(w + 7) // 8 * 8 if w <= 32 else 0 for w in widths]        # what each frame leaves for the next one to speculate
    assert all(w <= 32 for w in widths[:3]) and widths[3] > 32 and widths[4] <= 32 and widths[5] < widths[4], widths
    assert widths[1] > spec[0] and widths[2] > spec[1] and widths[3] > spec[2], (widths, spec)      # rises: too narrow each time
    assert spec[3] == 0 and widths[5] < spec[4], (widths, spec)                                     # wide: not speculated; falls


def test_frame_stream_fuse_width_speculation_with_frames_in_flight(oracle):
    """The same speculation under NativeFrameStream: its worker threads take whichever frame comes next, so each speculates from the
    last frame IT handled.  The filter voxel is fixed (0.3 mm) and the fused width changes with the frame: A keeps a small window of
    sensor 0's person mask only (<= 24 bits), B a larger window (25 .. 32 bits: too narrow after A), C every sensor's whole mask (> 32
    bits: never speculated).  The depth images -- and so the registrations -- are the same in every frame; only the colour mask
    changes.  One thread steps A B C A, then a stream four frames deep runs a mixed sequence; every frame equals SensorShardPipeline
    bit for bit and the oracle step."""
    from kinectpy_amd.pipeline import NativeFramePipeline, NativeFrameStream, PipelineParams, SensorShardPipeline
    xy, depth, rgb, inits, _ = synth.sensor_ring(4, 1)
    prm = PipelineParams(filt_voxel=0.3)
    rows, cols = np.divmod(np.arange(synth.H * synth.W), synth.W)

    def sensor0_window(r0, r1, c0, c1):
        r = rgb[0].copy()
        r[1:] = 0
        r[0][~((rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1))] = 0
        return r

    variants = {"A": sensor0_window(280, 290, 310, 320), "B": sensor0_window(250, 330, 280, 360), "C": rgb[0]}
    d = torch.as_tensor(depth[0]).cuda()
    dev, ref, shard, width = {}, {}, {}, {}
    for v, col in variants.items():
        dev[v] = torch.as_tensor(col).cuda()
        rp, rc, rT, mid = oracle.pipeline_step(xy, depth[0], col, inits, prm)
        ref[v] = (rp, rc, np.stack(rT))
        width[v] = fused_key_bits([m[0] for m in mid["masked"]], rT, prm.filt_voxel)
        pp, pc, pT = SensorShardPipeline(xy, 4, inits, prm).step(d, dev[v])
        shard[v] = (npy(pp), npy(pc), pT)
    assert width["A"] <= 24 < width["B"] <= 32 < width["C"], width

    def same(v, gp, gc, gT, tag):
        assert np.array_equal(gp, shard[v][0]) and np.array_equal(gc, shard[v][1]) and np.abs(gT - shard[v][2]).max() < 1e-11, tag
        assert np.array_equal(gp, ref[v][0]) and np.array_equal(gc, ref[v][1]) and np.abs(gT - ref[v][2]).max() < 1e-8, tag

    nat = NativeFramePipeline(xy, 4, inits, prm)
    for v in "ABCA":                                                   # rises past the speculation, goes above 32, falls
        gp, gc, gT = nat.step(d, dev[v])
        same(v, npy(gp), npy(gc), gT, ("serial", v))
    seq = "ABCAACBACCBAB"
    fs = NativeFrameStream(nat, 4)
    got = []
    for v in seq:
        if fs.full():
            got.append([npy(t) if isinstance(t, torch.Tensor) else t.copy() for t in fs.pop()])
        fs.submit(d, dev[v])
    while fs.pending:
        got.append([npy(t) if isinstance(t, torch.Tensor) else t.copy() for t in fs.pop()])
    fs.close()
    assert len(got) == len(seq)
    for i, (v, (gp, gc, gT)) in enumerate(zip(seq, got)):
        same(v, gp, gc, gT, ("stream", i, v))

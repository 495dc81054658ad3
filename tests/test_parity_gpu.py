"""GPU suite (-m gpu): the HIP path through the C ABI against the CPU oracle on the same seeded inputs.
Bar: bit-exact for integer / index outputs and for floats produced in a defined operation order
(compaction, voxel means, transforms, NN distances); stated tolerances where a parallel reduction
reorders a floating-point sum (SOR statistics, plane re-fit, ICP transform)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from kinectpy_amd.utils import synth
from odometry_scenes import write_device as _write_device          # shared with the drift check's directory

pytestmark = pytest.mark.gpu
KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_kat.json")))
NORM_KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_norm_kat.json")))

TOL_STATS = 1e-11      # relative, SOR mean/std/threshold (reduction order)
TOL_PLANE = 1e-10      # absolute, re-fitted plane coefficients (unit normal; d in mm)
TOL_T = 1e-8           # absolute, ICP 4x4 (rotation entries / mm)


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as o
    return o


def npy(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- extract
def test_unproject_bit_exact(ops, oracle):
    xy = synth.xy_table()
    dep = synth.render_depth(xy=xy)
    assert np.array_equal(npy(ops.unproject_u16(dep, xy))[0], oracle.unproject_u16(dep, xy))
    # scalar path (size not a multiple of 8), extreme depths, NaN table entries
    rng = np.random.default_rng(0)
    n = 1003
    d = rng.integers(0, 65535, n).astype(np.uint16)
    d[:5] = [0, 1, 65535, 32767, 32768]
    t = rng.normal(scale=0.6, size=(n, 2)).astype(np.float32)
    t[7] = np.nan
    assert np.array_equal(npy(ops.unproject_u16(d, t))[0], oracle.unproject_u16(d, t))
    # batched frames share the table
    deps = np.stack([synth.render_depth(seed=s, xy=xy) for s in (3, 4)])
    got = npy(ops.unproject_u16(deps, xy, 2))
    for f in range(2):
        assert np.array_equal(got[f], oracle.unproject_u16(deps[f], xy))


def test_median_exact(ops):
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 1000, 1001, 368640):
        v = rng.integers(-32768, 32767, size=(3, n, 3)).astype(np.int16)
        if n > 10:
            v[1, :, 2] = 1234                 # constant column
            v[2, : n // 2, 2] = -5            # two clusters -> even-n mean of different values
            v[2, n // 2:, 2] = 6
        t = torch.as_tensor(v).cuda()
        got = npy(ops.median_i16(t.reshape(-1)[2:], n, 3, 3))
        assert got.tolist() == [float(np.median(v[f, :, 2])) for f in range(3)]
        os.environ["KPX_MEDIAN_FRAME"] = "1"          # the one-block-per-frame form (a batch's default), forced for three frames
        try:
            got = npy(ops.median_i16(t.reshape(-1)[2:], n, 3, 3))
        finally:
            del os.environ["KPX_MEDIAN_FRAME"]
        assert got.tolist() == [float(np.median(v[f, :, 2])) for f in range(3)]
    # a batch (>= 64 frames: one block per frame, the frame's whole histogram in LDS): Kinect-like depths, frames that are mostly
    # negative (the second read), constant frames, odd and even sizes, contiguous values (stride 1) and the z channel of XYZ images
    for n, stride in ((36864, 1), (36865, 1), (40000, 3), (32769, 3)):
        F = 66
        v = rng.integers(0, 6000, size=(F, n, stride)).astype(np.int16)
        v[1] = rng.integers(-32768, 32767, size=(n, stride))
        v[2] = rng.integers(-32768, -1, size=(n, stride))
        v[3, : n // 2 + 1] = -7
        v[4] = 0
        v[5, ::2] = 32767
        v[6, : n // 2] = -32768
        t = torch.as_tensor(v).cuda()
        got = npy(ops.median_i16(t.reshape(-1)[stride - 1:], n, stride, F))
        assert got.tolist() == [float(np.median(v[f, :, stride - 1])) for f in range(F)], (n, stride)


@pytest.mark.parametrize("cm,dg", [(False, False), (True, False), (False, True), (True, True)])
def test_compact_bit_exact(ops, oracle, cm, dg):
    xy = synth.xy_table()
    dep = synth.render_depth(xy=xy)
    rgb = synth.person_mask_rgb(dep)
    xyz = oracle.unproject_u16(dep, xy)
    (p, c, i), = ops.rgbd_compact(xyz, rgb, 1, cm, dg)
    rp, rc, ri = oracle.rgbd_compact(xyz, rgb, cm, dg, oracle.median_z(xyz) + 750.0)
    assert np.array_equal(npy(p), rp) and np.array_equal(npy(c), rc) and np.array_equal(npy(i), ri)


def test_compact_reference_kat(ops):
    """the reference's own NumPy masks (captured by tests/golden/make_ref_kat.py)"""
    from kinectpy_amd.preprocessing.data import transform_filtered_image_to_pointcloud
    for c in KAT["mask_gate_compact"]:
        pcd = transform_filtered_image_to_pointcloud(np.array(c["color"], np.uint8), np.array(c["depth"], np.int16))
        assert np.array_equal(np.asarray(pcd.points), np.array(c["final_points"]).reshape(-1, 3))
        assert np.allclose(np.asarray(pcd.colors), np.array(c["final_colors"]).reshape(-1, 3), atol=6e-8)


def test_extract_random_frames_match_oracle(ops, oracle):
    """thirty seeded random frame batches (pixel counts that do / do not take the 8-pixel vector path, 1 .. 5 frames, random
    validity holes, NaN table entries, sparse colour masks, every flag combination, with / without index output): fused
    depth->cloud and the int16-XYZ compaction against the oracle, bit for bit"""
    rng = np.random.default_rng(123)
    for case in range(30):
        n = int(rng.choice([8, 64, 512, 1000, 4096, 5003, 20000, 36864]))
        F = int(rng.integers(1, 6))
        t = rng.normal(scale=0.5, size=(n, 2)).astype(np.float32)
        t[rng.random(n) < 0.01] = np.nan
        d = rng.integers(300, 6000, size=(F, n)).astype(np.uint16)
        d[rng.random((F, n)) < rng.uniform(0.0, 0.6)] = 0
        rgb = rng.integers(0, 255, size=(F, n, 3)).astype(np.uint8)
        rgb[rng.random((F, n)) < rng.uniform(0.0, 0.9)] = 0
        cm, dg, wi = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        use_rgb = bool(rng.integers(0, 2)) or cm
        res = ops.depth_to_cloud(d, t, rgb if use_rgb else None, F, cm, dg, want_idx=wi)
        xyz = np.stack([oracle.unproject_u16(d[f], t) for f in range(F)])
        res2 = ops.rgbd_compact(xyz, rgb if use_rgb else None, F, cm, dg, want_idx=wi)
        for f in range(F):
            rp, rc, ri = oracle.rgbd_compact(xyz[f], rgb[f] if use_rgb else None, cm, dg, oracle.median_z(xyz[f]) + 750.0)
            for (gp, gc, gi) in (res[f], res2[f]):
                assert np.array_equal(npy(gp), rp), (case, n, F, cm, dg)
                if use_rgb:
                    assert np.array_equal(npy(gc), rc), (case, "colour")
                if wi:
                    assert np.array_equal(npy(gi), ri), (case, "idx")


def test_fused_depth_to_cloud_batched_and_edge_cases(ops, oracle):
    xy = synth.xy_table()
    deps = np.stack([synth.render_depth(seed=s, xy=xy) for s in (1, 2, 3)] + [np.zeros(576 * 640, np.uint16)])
    rgbs = np.stack([synth.person_mask_rgb(d) for d in deps])
    res = ops.depth_to_cloud(deps, xy, rgbs, 4, True, True, want_idx=True)
    for f in range(4):
        r = oracle.unproject_u16(deps[f], xy)
        rp, rc, ri = oracle.rgbd_compact(r, rgbs[f], True, True, oracle.median_z(r) + 750.0)
        p, c, i = res[f]
        assert np.array_equal(npy(p), rp) and np.array_equal(npy(c), rc) and np.array_equal(npy(i), ri)
    assert res[3][0].shape[0] == 0           # empty frame -> empty cloud
    # a batch of 64 frames (the median takes its one-block-per-frame form): every frame equals its single-frame result
    big = ops.depth_to_cloud(np.tile(deps, (16, 1)), xy, np.tile(rgbs, (16, 1, 1)), 64, True, True, want_idx=True)
    for f in range(64):
        for a, b in zip(big[f], res[f % 4]):
            assert np.array_equal(npy(a), npy(b)), f
    xyz = np.stack([oracle.unproject_u16(deps[f], xy) for f in range(4)])
    one = ops.rgbd_compact(xyz, rgbs, 4, True, True)
    many = ops.rgbd_compact(np.tile(xyz, (16, 1, 1)), np.tile(rgbs, (16, 1, 1)), 64, True, True)
    for f in range(64):
        for a, b in zip(many[f], one[f % 4]):
            assert np.array_equal(npy(a), npy(b)), f
    # no colours, no gate, ragged size
    d = deps[0][:5001]
    (p, c, i), = ops.depth_to_cloud(d, xy[:5001], None, 1, False, False, want_idx=True)
    rp, _, ri = oracle.rgbd_compact(oracle.unproject_u16(d, xy[:5001]))
    assert c is None and np.array_equal(npy(p), rp) and np.array_equal(npy(i), ri)


# ------------------------------------------------------------------------------------------- container
def test_transform_rotate_bit_exact(ops, oracle, base_cloud):
    T = synth.t_star()
    for n in (0, 1, 5, 4096, len(base_cloud)):
        assert np.array_equal(npy(ops.transform(base_cloud[:n], T)), oracle.transform(base_cloud[:n], T))
    nrm = np.random.default_rng(0).normal(size=(1001, 3)).astype(np.float32)
    assert np.array_equal(npy(ops.rotate(nrm, T)), oracle.rotate(nrm, T))
    t = torch.as_tensor(base_cloud[:1000].copy()).cuda()       # in place
    ops.transform(t, T, out=t)
    assert np.array_equal(npy(t), oracle.transform(base_cloud[:1000], T))


def test_transform_rotate_every_form(ops, oracle):
    """Each form of kpx_transform / kpx_rotate at the smallest sizes that reach it, bit for bit against the oracle: the scalar loop alone
    (n < 4, or a view that starts 12 bytes in and so is not 16-byte aligned), the vector loop with every n % 4 tail, transform's LDS
    kernel alone (65536 aligned points) and with its one-block tail launch; out of place and in place."""
    T = synth.t_star()
    sizes = (1, 3, 4, 5, 255, 256, 257, 65535, 65536, 65536 + 3, 65536 + 255, 65536 + 256 + 1)
    host = (np.random.default_rng(11).standard_normal((max(sizes) + 1, 3)) * 700.0).astype(np.float32)
    dev = torch.as_tensor(host).cuda()
    assert dev.data_ptr() % 16 == 0
    for name in ("transform", "rotate"):
        op, ref = getattr(ops, name), getattr(oracle, name)
        for first in (0, 1):
            for n in sizes:
                want = ref(host[first:first + n], T)
                view = dev[first:first + n]
                assert view.data_ptr() == dev.data_ptr() + 12 * first
                assert np.array_equal(npy(op(view, T)), want), (name, first, n, "out of place")
                work = dev.clone()
                view = work[first:first + n]
                assert work.data_ptr() % 16 == 0 and op(view, T, out=view) is view
                assert np.array_equal(npy(view), want), (name, first, n, "in place")
                assert np.array_equal(npy(work[first + n:]), host[first + n:]) and np.array_equal(npy(work[:first]), host[:first]), (name, first, n, "wrote outside the view")


def test_joints_affine_reference_kat():
    from kinectpy_amd.preprocessing.extractor import transform_joint_rows
    for c in KAT["transform_joints"]:
        got = transform_joint_rows(np.array(c["x"]), np.array(c["T"]))
        assert np.allclose(got, np.array(c["y"]), rtol=1e-15, atol=1e-12)


def test_select_halfspace_slab(ops, oracle, base_cloud):
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.floor_removal import pcd_above_plane
    rng = np.random.default_rng(1)
    idx = rng.choice(len(base_cloud), 1000, replace=False)
    pc = PointCloud(base_cloud)
    pc.colors = rng.random(base_cloud.shape)
    col32 = npy(pc._col)
    # [O3D] SelectByIndex has mask semantics: ascending original order, duplicates collapse, whatever the list's order
    sel = pc.select_by_index(idx.reshape(-1, 1))                     # (K,1) argwhere-style, here unsorted
    srt = np.sort(idx)
    assert np.array_equal(npy(sel._pts), base_cloud[srt]) and np.array_equal(npy(sel._col), col32[srt])
    dup = pc.select_by_index(np.concatenate([idx, idx[:100], idx[::-1]]))
    assert np.array_equal(npy(dup._pts), base_cloud[srt]) and np.array_equal(npy(dup._col), col32[srt])
    assert np.array_equal(npy(ops.select_by_index([pc._pts], srt, trusted=True)[0]), base_cloud[srt])   # the one-gather path
    inv = pc.select_by_index(idx, invert=True)
    m = np.ones(len(base_cloud), bool)
    m[idx] = False
    assert np.array_equal(npy(inv._pts), base_cloud[m]) and np.array_equal(npy(inv._col), col32[m])
    assert pc.select_by_index([]).points.__len__() == 0
    assert len(pc.select_by_index([], invert=True).points) == len(base_cloud)
    lo, up = ops.slab_split(base_cloud, 200.0)
    y = base_cloud[:, 1].astype(np.float64)
    assert np.array_equal(npy(lo), np.flatnonzero(y >= y.max() - 200)) and np.array_equal(npy(up), np.flatnonzero(y < y.max() - 200))
    pl = [0.1, -0.9, 0.2, 300.0]
    assert np.array_equal(npy(ops.halfspace_select(base_cloud, pl)), oracle.halfspace_keep_idx(*pl, base_cloud))
    for c in KAT["pcd_above_plane"]:                                    # reference KAT2
        kept = pcd_above_plane(*c["abcd"], PointCloud(np.array(c["pts"])))
        want = np.array(c["pts"], dtype=np.float64)[np.array(c["idx"]).reshape(-1)]
        assert np.array_equal(np.asarray(kept.points), want.astype(np.float32).astype(np.float64))   # float32 storage


def test_selections_random_sizes_and_unaligned_views(ops, oracle):
    """half-space / slab selections, index selection and transforms on random sizes (tails that are not a multiple of the
    8-point vector width) and on device views whose first element is not 16-byte aligned (scalar fallback)"""
    rng = np.random.default_rng(19)
    for case in range(24):
        n = int(rng.choice([1, 7, 8, 9, 63, 2047, 2048, 2049, 10007, 65536 + 5]))
        off = int(rng.integers(0, 4))                                # rows skipped: 12-byte steps break the alignment
        host = rng.normal(scale=500, size=(n + off, 3)).astype(np.float32)
        dev = torch.as_tensor(host).cuda()[off:]                     # contiguous view, possibly unaligned
        p = host[off:]
        pl = [float(x) for x in rng.normal(size=3)] + [float(rng.normal(scale=200))]
        assert np.array_equal(npy(ops.halfspace_select(dev, pl)), oracle.halfspace_keep_idx(*pl, p)), (case, n, off)
        slab = float(rng.uniform(1, 800))
        lo, up = ops.slab_split(dev, slab)
        y = p[:, 1].astype(np.float64)
        assert np.array_equal(npy(lo), np.flatnonzero(y >= y.max() - slab)) and np.array_equal(npy(up), np.flatnonzero(y < y.max() - slab))
        T = synth.t_star()
        assert np.array_equal(npy(ops.transform(dev, T)), oracle.transform(p, T))
        k = int(rng.integers(0, n + 1))
        idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
        g = ops.select_by_index([dev], idx)[0]
        assert np.array_equal(npy(g), p[idx])
        gi = ops.select_by_index([dev], idx, invert=True)[0]
        m = np.ones(n, bool); m[idx] = False
        assert np.array_equal(npy(gi), p[m])


def test_bounds_and_the_split_that_reads_them(ops):
    """kpx_bounds (lane-contiguous 16-byte loads above 65536 points, one block below, scalar loads for unaligned views), the gather that
    leaves the bounds of what it wrote, and kpx_slab_split_bounded: numpy's min / max, and the lists of the two-pass split"""
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.floor_removal import remove_floor
    rng = np.random.default_rng(23)
    for n in [1, 2, 255, 256, 257, 65536, 65537, 65536 + 255, 65536 + 256, 300_001, 1_048_576, 2_000_003]:
        for off in ([0, 1] if n < 400_000 else [0]):
            host = rng.normal(scale=700, size=(n + off, 3)).astype(np.float32)
            if n > 3:                                                  # the extremes at the ends and inside a chunk
                host[off, 0] = -9e4; host[off + n - 1, 1] = 8e4; host[off + n // 2, 2] = -7e4
            dev = torch.as_tensor(host).cuda()[off:]
            p = host[off:]
            bb = ops.bounds(dev)
            want = np.concatenate([p.min(0), p.max(0)]).astype(np.float64)
            assert np.array_equal(npy(bb), want), (n, off)
            slab = float(rng.uniform(1, 900))
            lo, up = ops.slab_split(dev, slab)
            lo2, up2 = ops.slab_split(dev, slab, bounds=bb)
            y = p[:, 1].astype(np.float64)
            assert np.array_equal(npy(lo), np.flatnonzero(y >= y.max() - slab)) and np.array_equal(npy(up), np.flatnonzero(y < y.max() - slab)), (n, off)
            assert np.array_equal(npy(lo2), npy(lo)) and np.array_equal(npy(up2), npy(up)), (n, off)
            k = int(rng.integers(1, n + 1))
            idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
            col = torch.as_tensor(rng.random((n, 3)).astype(np.float32)).cuda()
            (g, gc, gn), gb = ops.select_by_index([dev, col, None], idx, trusted=True, want_bounds=True)
            assert gn is None and np.array_equal(npy(g), p[idx]) and np.array_equal(npy(gc), npy(col)[idx])
            assert np.array_equal(npy(gb), np.concatenate([p[idx].min(0), p[idx].max(0)]).astype(np.float64)), (n, off, k)
    # the cloud object: bounds left by the producing gather, dropped when the points move
    host = rng.normal(scale=700, size=(90_000, 3)).astype(np.float32)
    pc = PointCloud(host)
    assert pc._bounds is None
    assert np.array_equal(pc.get_max_bound(), host.max(0).astype(np.float64)) and np.array_equal(pc.get_min_bound(), host.min(0).astype(np.float64))
    assert pc._bounds is not None
    sel = pc._select(torch.arange(0, 90_000, 3, dtype=torch.int32).cuda())
    assert sel._bounds is not None and np.array_equal(sel.get_max_bound(), host[::3].max(0).astype(np.float64))
    filt, keep = pc.remove_statistical_outlier(8, 1.5)
    assert filt._bounds is not None and np.array_equal(npy(filt._bounds), np.concatenate([host[keep].min(0), host[keep].max(0)]).astype(np.float64))
    T = np.eye(4); T[1, 3] = 1234.0
    filt.transform(T)
    assert filt._bounds is None
    a = remove_floor(filt.clone(), seed=5)                             # bounds recomputed after the move ...
    b_in = filt.clone(); b_in._device_bounds()
    b = remove_floor(b_in, seed=5)                                     # ... or already there: the same cloud
    assert np.array_equal(npy(a._pts), npy(b._pts)) and len(a.points) > 0


# ---------------------------------------------------------------------------------------------- filters
@pytest.mark.parametrize("voxel", [0.02, 10.0, 35.0, 500.0])
def test_voxel_bit_exact(ops, oracle, base_cloud, voxel):
    rng = np.random.default_rng(0)
    col = rng.random(base_cloud.shape).astype(np.float32)
    nrm = rng.normal(size=base_cloud.shape).astype(np.float32)
    gp, gc, gn = ops.voxel_downsample(base_cloud, voxel, col, nrm)
    rp, rc, rn = oracle.voxel_downsample(base_cloud, voxel, col, nrm)
    assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc) and np.array_equal(npy(gn), rn)


def test_voxel_batch_equals_single_calls(ops, oracle, base_cloud):
    """several clouds side by side (ragged sizes, one empty, seven > number of lanes): bit-identical to one call each"""
    rng = np.random.default_rng(5)
    clouds = [base_cloud, base_cloud[:5001] + 7.0, np.zeros((0, 3), np.float32), base_cloud[::3].copy(), base_cloud[:17],
              (base_cloud[:30000] * 0.5).astype(np.float32), base_cloud[1000:1001]]
    cols = [rng.random(c.shape).astype(np.float32) for c in clouds]
    got = ops.voxel_downsample_batch(clouds, 35.0, cols)
    assert len(got) == len(clouds)
    for c, col, (gp, gc) in zip(clouds, cols, got):
        if len(c) == 0:
            assert gp.shape[0] == 0
            continue
        rp, rc, _ = oracle.voxel_downsample(c, 35.0, col)
        assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc)
    nocol = ops.voxel_downsample_batch(clouds[:2], 10.0)
    assert nocol[0][1] is None and np.array_equal(npy(nocol[0][0]), oracle.voxel_downsample(clouds[0], 10.0)[0])
    # up to 8 clouds go through ONE concatenated pass (cloud number = top digit of the key), more through the lanes
    for k in (1, 2, 4, 8, 9):
        sub = [clouds[i % len(clouds)] + np.float32(13.0 * i) for i in range(k)]
        for (gp, _), c in zip(ops.voxel_downsample_batch(sub, 20.0), sub):
            if len(c):
                assert np.array_equal(npy(gp), oracle.voxel_downsample(c, 20.0)[0]), k
            else:
                assert gp.shape[0] == 0
    # more than a million points together: the sort is an Onesweep over the key bits the batch really uses (read back)
    rngb = np.random.default_rng(8)
    big = [(rngb.random((n_, 3)) * [4000, 2500, 3800] + [-2000, -1200, 300]).astype(np.float32) for n_ in (300_000, 280_000, 310_000, 290_000)]
    for (gp, _), c in zip(ops.voxel_downsample_batch(big, 35.0), big):
        assert np.array_equal(npy(gp), oracle.voxel_downsample(c, 35.0)[0])
    # a cloud whose grid would overflow fails alone, with the same error as a single call
    from kinectpy_amd._lib import KinectPxError
    far = np.array([[0, 0, 0], [1e7, 0, 0]], np.float32)
    with pytest.raises(KinectPxError, match="too small"):
        ops.voxel_downsample_batch([clouds[0], far], 1.0)


def test_voxel_edge_cases(ops, oracle):
    from kinectpy_amd._lib import KinectPxError
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    assert np.array_equal(npy(ops.voxel_downsample(one, 5.0)[0]), one)
    dup = np.repeat(one, 17, 0)
    assert np.array_equal(npy(ops.voxel_downsample(dup, 5.0)[0]), one)
    assert ops.voxel_downsample(np.zeros((0, 3), np.float32), 5.0)[0].shape[0] == 0
    with pytest.raises(KinectPxError, match="voxel_size"):
        ops.voxel_downsample(one, 0.0)
    far = np.array([[0, 0, 0], [1e7, 0, 0]], np.float32)
    with pytest.raises(KinectPxError, match="too small"):
        ops.voxel_downsample(far, 0.001)
    with pytest.raises(RuntimeError):
        oracle.voxel_downsample(far, 0.001)


@pytest.mark.parametrize("n,k,ratio", [(5000, 20, 2.0), (60000, 20, 2.0), (20000, 50, 0.3), (20000, 200, 3.0),
                                       (17, 20, 1.0), (2, 5, 1.0), (300, 288, 1.5), (12000, 500, 2.0), (3000, 1500, 1.0)])
def test_sor_indices_bit_exact(ops, oracle, base_cloud, n, k, ratio):
    rng = np.random.default_rng(n + k)
    p = base_cloud[rng.choice(len(base_cloud), n, replace=False)]
    gi, gs, ga = ops.sor(p, k, ratio, want_avg=True)
    ri, rs, ra = oracle.sor(p, k, ratio)
    assert np.array_equal(npy(gi), ri)
    assert np.allclose(npy(ga), ra, rtol=1e-14, atol=0)
    if n > 2:
        assert np.allclose(npy(gs), rs, rtol=TOL_STATS, atol=0)


@pytest.mark.parametrize("n,k,ratio", [(0, 200, 3.0), (100000, 129, 1.0), (150000, 400, 2.0), (200000, 1000, 2.5)])
def test_sor_large_k_at_frame_density(ops, oracle, base_cloud, n, k, ratio):
    """the block-per-64-queries kernel (k > 128) where it works hardest: dense clouds, whose 27-cell blocks hold up to 2048 candidates and
    whose k-th neighbour lies near the distance the block covers (the selection window ends at the cover's high word); n = 0: the whole
    283k-point frame cloud at filter_outliers' defaults.  Keep list equal, per-point means to 1e-14 -- a selection that takes one candidate
    too many moves a mean by ~1e-3 of itself.  Then the float64 sampled-row check of oracle/lineage2.py on 2000 rows: a second lineage
    (cKDTree) for the means, the statistics and the keep list"""
    from oracle import lineage2 as L2
    rng = np.random.default_rng(n + k)
    p = base_cloud if n == 0 else base_cloud[rng.choice(len(base_cloud), n, replace=False)]
    gi, gs, ga = ops.sor(p, k, ratio, want_avg=True)
    ri, rs, ra = oracle.sor(p, k, ratio)
    assert np.array_equal(npy(gi), ri)
    assert np.allclose(npy(ga), ra, rtol=1e-14, atol=0)
    assert np.allclose(npy(gs), rs, rtol=TOL_STATS, atol=0)
    rows = np.sort(rng.choice(len(p), 2000, replace=False))
    L2.check_sor_f64(p, k, ratio, npy(gi), npy(gs), npy(ga), rows, workers=16)


def test_sor_block_kernel_fuzz_ties_duplicates_clusters(ops, oracle):
    """random (cloud, k) pairs for the block-per-64-queries kernel (k > 32) and the counting selection behind every form: integer
    lattices (many candidates AT the k-th distance: the low-word phase, ties beyond the selection buffer's room), clouds with blocks of
    coincident points (zero distances: the window starts above them, or the k-th is one of them), tight clusters in empty space (the
    second block radius, the leftovers' list), tiny clouds (k >= n).  Keep list equal, means to 1e-13."""
    rng = np.random.default_rng(77)
    for case in range(40):
        kind = case % 4
        if kind == 0:                                   # lattice, integer coordinates, permuted
            a, b, c = (int(v) for v in rng.integers(6, 22, size=3))
            step = float(rng.choice([1.0, 3.0, 10.0]))
            gx, gy, gz = np.arange(a, dtype=np.float32), np.arange(b, dtype=np.float32), np.arange(c, dtype=np.float32)
            p = np.stack(np.meshgrid(gx, gy, gz, indexing="ij"), -1).reshape(-1, 3) * step
        elif kind == 1:                                 # smooth sheet with blocks of coincident points
            n = int(rng.integers(3000, 30000))
            p = np.stack([rng.uniform(0, 2000, n), rng.uniform(0, 1500, n), np.zeros(n)], 1).astype(np.float32)
            p[:, 2] = 1500 + 40 * np.sin(p[:, 0] / 300) + rng.normal(scale=2.0, size=n)
            for _ in range(int(rng.integers(1, 6))):
                i0, m = int(rng.integers(0, n - 400)), int(rng.integers(2, 400))
                p[i0:i0 + m] = p[i0]
        elif kind == 2:                                 # tight clusters far apart + a few isolated points
            cl = [rng.normal(loc=rng.uniform(-3000, 3000, 3), scale=rng.uniform(3, 60), size=(int(rng.integers(50, 4000)), 3)) for _ in range(6)]
            p = np.concatenate(cl + [rng.uniform(-5000, 5000, size=(20, 3))]).astype(np.float32)
        else:                                           # tiny
            p = rng.normal(scale=100, size=(int(rng.integers(2, 200)), 3)).astype(np.float32)
        p = np.ascontiguousarray(p[rng.permutation(len(p))], dtype=np.float32)
        k = int(rng.choice([33, 40, 64, 65, 100, 128, 129, 200, 288, 400, 700])) if kind != 3 else int(rng.integers(1, 300))
        ratio = float(rng.choice([0.3, 1.0, 2.0, 3.0]))
        gi, gs, ga = ops.sor(p, k, ratio, want_avg=True)
        ri, rs, ra = oracle.sor(p, k, ratio)
        assert np.array_equal(npy(gi), ri), (case, kind, len(p), k, ratio)
        assert np.allclose(npy(ga), ra, rtol=1e-13, atol=0), (case, kind, len(p), k, ratio)


def test_sor_duplicates_and_errors(ops, oracle):
    from kinectpy_amd._lib import KinectPxError
    rng = np.random.default_rng(3)
    p = rng.normal(scale=100, size=(2000, 3)).astype(np.float32)
    p[:40] = p[0]                 # 40 coincident points: avg distance 0 for k <= 40 -> dropped (avg > 0 test)
    gi, _, ga = ops.sor(p, 20, 2.0, want_avg=True)
    ri, _, ra = oracle.sor(p, 20, 2.0)
    assert np.array_equal(npy(gi), ri) and (npy(ga)[:40] == 0).all() and not np.isin(np.arange(40), ri).any()
    for bad in [(0, 1.0), (5, 0.0), (5, -1.0), (4097, 1.0)]:
        with pytest.raises(KinectPxError):
            ops.sor(p, *bad)


def _random_cloud(rng, n):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        p = rng.normal(scale=rng.uniform(1, 800), size=(n, 3))
    elif kind == 1:                                              # sheet with noise
        p = np.stack([rng.uniform(-2000, 2000, n), rng.uniform(-1500, 1500, n), rng.normal(scale=2.0, size=n)], -1)
    elif kind == 2:                                              # a few tight blobs far apart + stragglers
        c = rng.uniform(-5000, 5000, size=(rng.integers(1, 6), 3))
        p = c[rng.integers(0, len(c), n)] + rng.normal(scale=3.0, size=(n, 3))
        p[: max(1, n // 50)] = rng.uniform(-6000, 6000, size=(max(1, n // 50), 3))
    elif kind == 3:                                              # integer lattice with repeats
        p = rng.integers(-20, 20, size=(n, 3)).astype(np.float64) * rng.integers(1, 9)
    else:                                                        # line
        t = rng.uniform(-3000, 3000, n)
        p = np.stack([t, 0.5 * t + 10, np.full(n, 700.0)], -1)
    return (p + rng.uniform(-3000, 3000, size=3)).astype(np.float32)


def test_filters_random_shapes_match_oracle(ops, oracle):
    """forty seeded random clouds (blobs, sheets, lines, lattices with duplicates; 1 .. 8000 points) through voxel, SOR and
    normals with random parameters: kept indices / voxel means bit-exact, statistics within tolerance"""
    rng = np.random.default_rng(77)
    for case in range(40):
        n = int(rng.integers(1, 8000))
        p = _random_cloud(rng, n)
        voxel = float(rng.choice([3.0, 10.0, 35.0, 120.0]))
        gp = npy(ops.voxel_downsample(p, voxel)[0])
        rp = oracle.voxel_downsample(p, voxel)[0]
        assert np.array_equal(gp, rp), ("voxel", case, n, voxel)
        k, ratio = int(rng.choice([1, 5, 20, 50, 200])), float(rng.choice([0.3, 1.0, 2.0, 3.0]))
        gi, gs, ga = ops.sor(p, k, ratio, want_avg=True)
        ri, rs, ra = oracle.sor(p, k, ratio)
        assert np.allclose(npy(ga), ra, rtol=1e-12, atol=0), ("sor avg", case, n, k)
        near = np.abs(ra - rs[2]) <= 1e-9 * max(abs(rs[2]), 1.0)      # means exactly at the threshold may fall either way
        assert np.array_equal(np.setdiff1d(npy(gi), np.flatnonzero(near)), np.setdiff1d(ri, np.flatnonzero(near))), ("sor idx", case, n, k)
        radius, nn = float(rng.choice([5.0, 40.0, 150.0])), int(rng.choice([3, 10, 40, 100]))
        gn = npy(ops.estimate_normals(p, radius, nn)).astype(np.float64)
        rn, cov, cnt = oracle.estimate_normals(p, radius, nn)
        assert np.allclose(gn[cnt < 3], [0, 0, 1]), ("normals degenerate", case)
        A = np.zeros((len(p), 3, 3))
        A[:, 0, 0], A[:, 1, 1], A[:, 2, 2] = cov[:, 0], cov[:, 3], cov[:, 5]
        A[:, 0, 1] = A[:, 1, 0] = cov[:, 1]
        A[:, 0, 2] = A[:, 2, 0] = cov[:, 2]
        A[:, 1, 2] = A[:, 2, 1] = cov[:, 4]
        w = np.linalg.eigvalsh(A)
        well = (cnt >= 3) & ((w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-30)) & (w[:, 2] > 1e-9)
        assert (np.abs((gn * rn).sum(1))[well] > 1 - 1e-5).all(), ("normals", case, n, radius, nn)


def test_sor_and_normals_on_lattice_ties(ops, oracle):
    """integer lattice (raw Kinect XYZ is int16): many neighbours at exactly the k-th distance.  SOR counts ties at the
    k-th value k - (#smaller) times; normals keep the lowest original indices among them -- both as the oracle does.
    Sparse outliers next to the dense block exercise the truncated / radius-filtered gather passes."""
    g = np.arange(0, 24, dtype=np.float32)
    lat = np.stack(np.meshgrid(g, g, g[:6], indexing="ij"), -1).reshape(-1, 3) * 5.0
    rng = np.random.default_rng(9)
    far = rng.integers(-400, 600, size=(60, 3)).astype(np.float32)
    p = np.concatenate([lat, far])[rng.permutation(len(lat) + 60)]
    for k, ratio in ((6, 1.0), (20, 2.0), (27, 0.5), (200, 3.0)):
        gi, gs, ga = ops.sor(p, k, ratio, want_avg=True)
        ri, rs, ra = oracle.sor(p, k, ratio)
        assert np.array_equal(npy(gi), ri)
        assert np.allclose(npy(ga), ra, rtol=1e-13, atol=0)
    for radius, nn in ((12.0, 10), (8.0, 30), (26.0, 40)):
        gn = npy(ops.estimate_normals(p, radius, nn)).astype(np.float64)
        rn, cov, cnt = oracle.estimate_normals(p, radius, nn)
        A = np.zeros((len(p), 3, 3))
        A[:, 0, 0], A[:, 1, 1], A[:, 2, 2] = cov[:, 0], cov[:, 3], cov[:, 5]
        A[:, 0, 1] = A[:, 1, 0] = cov[:, 1]
        A[:, 0, 2] = A[:, 2, 0] = cov[:, 2]
        A[:, 1, 2] = A[:, 2, 1] = cov[:, 4]
        w = np.linalg.eigvalsh(A)
        well = (cnt >= 3) & ((w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-30))
        assert (np.abs((gn * rn).sum(1))[well] > 1 - 1e-6).all()      # same neighbour sets -> same normal (up to sign)
        assert np.allclose(gn[cnt < 3], [0, 0, 1])


def test_normals_up_to_sign(ops, oracle, base_cloud):
    rng = np.random.default_rng(2)
    p = base_cloud[rng.choice(len(base_cloud), 30000, replace=False)]
    gn = npy(ops.estimate_normals(p, 70.0, 40)).astype(np.float64)
    rn, cov, cnt = oracle.estimate_normals(p, 70.0, 40)
    A = np.zeros((len(p), 3, 3))
    A[:, 0, 0], A[:, 1, 1], A[:, 2, 2] = cov[:, 0], cov[:, 3], cov[:, 5]
    A[:, 0, 1] = A[:, 1, 0] = cov[:, 1]
    A[:, 0, 2] = A[:, 2, 0] = cov[:, 2]
    A[:, 1, 2] = A[:, 2, 1] = cov[:, 4]
    w = np.linalg.eigvalsh(A)
    well = (cnt >= 3) & ((w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-30))
    assert well.mean() > 0.95
    assert (np.abs((gn * rn).sum(1))[well] > 1 - 1e-6).all()          # float32 storage of a unit vector
    assert np.allclose(gn[cnt < 3], [0, 0, 1])


def test_large_neighbourhoods_beyond_the_lds_forms(ops, oracle, base_cloud):
    """The reference takes any nb_neighbors / max_nn (preprocessing/filtering.py:12-17, registration.py:7-21).  Up to 288 / 128 the
    neighbour heaps of the fall-back passes live in LDS; beyond, in the workspace (round 5): remove_statistical_outlier(500, 2.0),
    estimate_normals(Hybrid(r, 300)) and compute_fpfh_feature(Hybrid(r, 200)) against the oracle."""
    rng = np.random.default_rng(5)
    p = base_cloud[rng.choice(len(base_cloud), 8000, replace=False)]
    gi, gs, ga = ops.sor(p, 500, 2.0, want_avg=True)
    ri, rs, ra = oracle.sor(p, 500, 2.0)
    assert np.array_equal(npy(gi), ri) and np.allclose(npy(ga), ra, rtol=1e-14, atol=0)
    gn = npy(ops.estimate_normals(p, 400.0, 300)).astype(np.float64)
    rn, cov, cnt = oracle.estimate_normals(p, 400.0, 300)
    assert cnt.max() == 300                                            # the cap binds: neighbourhoods are cut at max_nn
    A = np.zeros((len(p), 3, 3))
    A[:, 0, 0], A[:, 1, 1], A[:, 2, 2] = cov[:, 0], cov[:, 3], cov[:, 5]
    A[:, 0, 1] = A[:, 1, 0] = cov[:, 1]
    A[:, 0, 2] = A[:, 2, 0] = cov[:, 2]
    A[:, 1, 2] = A[:, 2, 1] = cov[:, 4]
    w = np.linalg.eigvalsh(A)
    well = (cnt >= 3) & ((w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-30))
    assert well.mean() > 0.9 and (np.abs((gn * rn).sum(1))[well] > 1 - 1e-6).all()
    q = p[:3000]
    nrm = npy(ops.estimate_normals(q, 150.0, 40))
    got = npy(ops.fpfh(q, nrm, 600.0, 200))
    want, _ = oracle.fpfh(q, nrm, 600.0, 200)
    bad = np.abs(got - want).max(1) > 1e-6                              # (a libm atan2 ulp can move one pair across a bin edge)
    assert bad.mean() < 2e-3 and np.allclose(got[~bad], want[~bad], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("n,rn,iters,prob,seed", [(50000, 30, 2000, 0.99999999, 7), (50000, 3, 500, 0.99999999, 1),
                                                  (400000, 30, 2000, 0.99999999, 7), (20000, 30, 200, 1.0, 11),
                                                  (100, 30, 50, 0.9, 2)])
def test_segment_plane_inliers_bit_exact(ops, oracle, n, rn, iters, prob, seed):
    c3 = synth.filter_cloud(1_000_000 if n > 100000 else 200_000)
    fl = c3[c3[:, 1] >= c3[:, 1].max() - 200][:n]
    gpl, gidx = ops.segment_plane(fl, 30.0, rn, iters, prob, seed)
    rpl, ridx = oracle.segment_plane(fl, 30.0, rn, iters, prob, seed)
    assert np.array_equal(npy(gidx), ridx)
    assert np.abs(gpl - rpl).max() < TOL_PLANE


def test_segment_plane_vanishing_exit_bound(ops, oracle):
    """a cloud where the best plane holds a few per cent of the points and ransac_n = 30: fitness^30 vanishes against 1, the early-exit
    bound log(1-p) / log(1 - fitness^n) is -inf -- Open3D assigns it to a size_t (2^63 on x86-64: the loop runs on), and so do the
    oracle and the kernels since the second lineage found them stopping at the first hypothesis there (tests/test_oracle_cpu.py)"""
    rng = np.random.default_rng(11)
    k = 3000
    floor = np.stack([rng.uniform(-1500, 1500, k), 900 + rng.normal(0, 3, k), rng.uniform(1200, 3200, k)], 1)
    blob = rng.normal(0, 1, (k, 3)) * [250, 600, 200] + [0, 100, 2200]
    pts = np.vstack([floor, blob]).astype(np.float32)
    for rn, iters, prob in ((30, 120, 0.99999999), (30, 120, 1.0), (12, 200, 0.99999999)):
        gpl, gidx = ops.segment_plane(pts, 30.0, rn, iters, prob, 1)
        rpl, ridx, hyp = oracle.segment_plane(pts, 30.0, rn, iters, prob, 1, return_hypotheses=True)
        assert np.array_equal(npy(gidx), ridx) and np.abs(gpl - rpl).max() < TOL_PLANE
        if rn == 30:
            assert len(ridx) == int(hyp[:, 4].max())             # the best of ALL hypotheses, not the first one


def test_segment_plane_ties_thresholds_and_sequential_path(ops, oracle):
    """the matrix-core scoring (counts by fp64 MFMA, rmse only for the hypotheses the replay can ask about) at its edges: an exactly
    planar cloud where EVERY hypothesis ties (more ties than the list holds: the full sequential scoring takes over), distances that
    share the threshold's high word (the low words decide), thresholds outside the float32-pattern range (sequential kernel), and
    the same answers with the matrix path switched off in a child process"""
    import subprocess
    import sys
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(120, dtype=np.float32), np.arange(100, dtype=np.float32))
    flat = np.stack([gx.ravel() * 7, np.full(gx.size, 900.0, np.float32), gy.ravel() * 5], -1).astype(np.float32)
    cases = [(flat, 30.0, 3, 600), (flat, 30.0, 30, 300)]
    # a slab whose distances to the winning plane land ON the threshold's high word: y = 900 +- exactly 30 and a hair inside / outside
    edge = flat.copy()
    edge[::3, 1] += np.float32(30.0)
    edge[1::3, 1] -= np.float32(29.999998)
    cases.append((edge, 30.0, 3, 400))
    noisy = (flat + rng.normal(scale=4.0, size=flat.shape)).astype(np.float32)
    cases += [(noisy, 1e-320, 3, 50), (noisy, 30.0, 5, 500), (noisy, 2.5, 3, 1000)]
    for pts, thr, rn, iters in cases:
        gpl, gidx = ops.segment_plane(pts, thr, rn, iters, 1.0, 11)
        rpl, ridx = oracle.segment_plane(pts, thr, rn, iters, 1.0, 11)
        assert np.array_equal(npy(gidx), ridx), (thr, rn, iters)
        assert np.abs(gpl - rpl).max() < TOL_PLANE
    code = ("import numpy as np, sys; sys.path.insert(0, %r); from kinectpy_amd import ops; from kinectpy_amd.utils import synth; "
            "c = synth.filter_cloud(200000); pl, idx = ops.segment_plane(c, 30.0, 30, 2000, 1.0, 7); "
            "print(repr(pl.tolist()), int(idx.sum().item()), int(idx.shape[0]))") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = [subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KPX_PLANE_MFMA=v), capture_output=True, text=True, timeout=300) for v in ("1", "0")]
    assert all(o.returncode == 0 for o in outs), outs[0].stderr[-2000:] + outs[1].stderr[-2000:]
    assert outs[0].stdout.strip().splitlines()[-1] == outs[1].stdout.strip().splitlines()[-1]


# ------------------------------------------------------------------------------------------- registration
@pytest.fixture(params=["culled", "dense", "dense_fp64"])
def engine(request, ops):
    """the correspondence-search implementations: the culled sweep (default), the all-pairs sweeps (fp64 MFMA + float32 screening),
    and the all-pairs engine with every search on the fp64 MFMA sweep (loose bounds from the seed sweep first, tight ones from the previous partners in later iterations)"""
    prev = ops.nn_engine(request.param)
    yield request.param
    ops.nn_engine(prev)


@pytest.mark.parametrize("n,m", [(20000, 20000), (1000, 777), (333, 5000), (5, 1), (64, 17), (4097, 16), (17, 4097)])
def test_nn_bit_exact(ops, oracle, base_cloud, engine, n, m):
    src, tgt, T = synth.icp_pair(max(n, m), base_cloud)
    src, tgt = src[:n], tgt[:m]
    for M in (np.eye(4), np.linalg.inv(T)):
        gi, gd = ops.nn_search(src, tgt, M)
        ri, rd, _ = oracle.nn(src, M, tgt, grid=(n * m > 1e6))
        assert np.array_equal(npy(gi), ri) and np.array_equal(npy(gd), rd)


def test_nn_bit_exact_one_million(ops, oracle):
    """BASELINE-scale clouds through the culled search (10^12 pairs, ~1 ms): still the oracle's argmin, bit for bit"""
    src, tgt, T = synth.icp_pair(1_000_000)
    gi, gd = ops.nn_search(src, tgt, np.linalg.inv(T))
    ri, rd, _ = oracle.nn(src, np.linalg.inv(T), tgt, grid=True)
    assert np.array_equal(npy(gi), ri) and np.array_equal(npy(gd), rd)


def test_nn_ties_go_to_the_lowest_index(ops, oracle, engine):
    """integer-grid data (raw Kinect XYZ is int16): exact ties, exact arithmetic in both forms"""
    rng = np.random.default_rng(4)
    tgt = rng.integers(-50, 50, size=(3000, 3)).astype(np.float32)
    tgt[1500:] = tgt[:1500]                    # every target point twice
    src = rng.integers(-50, 50, size=(2000, 3)).astype(np.float32)
    gi, gd = ops.nn_search(src, tgt, np.eye(4))
    ri, rd, _ = oracle.nn(src, np.eye(4), tgt)
    assert np.array_equal(npy(gi), ri) and np.array_equal(npy(gd), rd) and (ri < 1500).all()


def test_nn_ties_between_distinct_points(ops, oracle, engine):
    """sources half way between lattice targets: equidistant DISTINCT targets that the Morton order puts into
    different column tiles; the lowest caller index must win"""
    g = np.arange(-12, 12, dtype=np.float32)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * 4.0
    tgt = tgt[np.random.default_rng(2).permutation(len(tgt))]
    src = tgt[::3] + np.array([2.0, 0.0, 0.0], np.float32)          # exactly between two lattice points
    src = np.concatenate([src, tgt[1::5] + np.array([2.0, 2.0, 2.0], np.float32)])       # centre of a cell: 8 ties
    gi, gd = ops.nn_search(src, tgt, np.eye(4))
    ri, rd, _ = oracle.nn(src, np.eye(4), tgt)
    assert np.array_equal(npy(gi), ri) and np.array_equal(npy(gd), rd)


def test_nn_far_apart_and_clustered(ops, oracle, base_cloud, engine):
    """rows without any finite bound (clouds 20 m apart), dense clumps plus isolated points, collinear targets"""
    rng = np.random.default_rng(11)
    src, tgt, _ = synth.icp_pair(6000, base_cloud)
    far = (src + np.array([20000.0, -3000.0, 500.0])).astype(np.float32)
    clumps = np.concatenate([rng.normal(c, 2.0, size=(800, 3)) for c in ((0, 0, 0), (5000, 0, 0), (0, 7000, 100))]
                            + [rng.uniform(-9000, 9000, size=(50, 3))]).astype(np.float32)
    line = np.stack([np.linspace(-4000, 4000, 3000), np.zeros(3000), np.full(3000, 2000.0)], -1).astype(np.float32)
    for s_, t_ in ((far, tgt), (src, clumps), (clumps, tgt), (src[:500], line), (line, src)):
        gi, gd = ops.nn_search(s_, t_, np.eye(4))
        ri, rd, _ = oracle.nn(s_, np.eye(4), t_)
        assert np.array_equal(npy(gi), ri) and np.array_equal(npy(gd), rd)


def test_nn_random_shapes_engines_and_oracle_agree(ops, oracle):
    """sixty seeded random problems (sizes 1 .. 6000, blobs / sheets / lines / lattices / duplicates, random rigid motion):
    culled engine == all-pairs engine == oracle, bit for bit"""
    rng = np.random.default_rng(2025)

    def cloud(n):
        kind = rng.integers(0, 5)
        if kind == 0:
            p = rng.normal(scale=rng.uniform(1, 800), size=(n, 3))
        elif kind == 1:                                          # sheet with noise
            p = np.stack([rng.uniform(-2000, 2000, n), rng.uniform(-1500, 1500, n), rng.normal(scale=2.0, size=n)], -1)
        elif kind == 2:                                          # a few tight blobs far apart
            c = rng.uniform(-5000, 5000, size=(rng.integers(1, 6), 3))
            p = c[rng.integers(0, len(c), n)] + rng.normal(scale=3.0, size=(n, 3))
        elif kind == 3:                                          # integer lattice with repeats
            p = rng.integers(-20, 20, size=(n, 3)).astype(np.float64) * rng.integers(1, 9)
        else:                                                    # line
            t = rng.uniform(-3000, 3000, n)
            p = np.stack([t, 0.5 * t + 10, np.full(n, 700.0)], -1)
        return (p + rng.uniform(-3000, 3000, size=3)).astype(np.float32)

    for case in range(60):
        n, m = int(rng.integers(1, 6000)), int(rng.integers(1, 6000))
        src, tgt = cloud(n), cloud(m)
        ang = rng.uniform(-0.6, 0.6, 3)
        cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
        R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = rng.uniform(-500, 500, 3)
        ri, rd, _ = oracle.nn(src, T, tgt)
        for name in ("culled", "dense"):
            prev = ops.nn_engine(name)
            try:
                gi, gd = ops.nn_search(src, tgt, T)
            finally:
                ops.nn_engine(prev)
            assert np.array_equal(npy(gi), ri) and np.array_equal(npy(gd), rd), (case, name, n, m)


def test_icp_without_any_correspondence(ops, oracle, base_cloud, engine):
    """nothing within max_correspondence_distance: fitness 0, the transform stays the initial one"""
    src, tgt, _ = synth.icp_pair(3000, base_cloud)
    far = (src + np.array([20000.0, 0.0, 0.0])).astype(np.float32)
    g = ops.icp(far, tgt, 100.0, None, "p2p", None, 5, want_corr=True)
    rT, rf, rr, rit = oracle.registration_icp(far, tgt, 100.0, None, "p2p", None, 5)
    assert g["fitness"] == rf == 0.0 and g["iterations"] == rit
    assert np.array_equal(g["transformation"], rT)
    assert (npy(g["d2"]) >= 100.0 ** 2).all()


@pytest.mark.parametrize("mode", ["p2p", "p2plane"])
def test_icp_matches_oracle(ops, oracle, base_cloud, engine, mode):
    src, tgt, T = synth.icp_pair(20000, base_cloud)
    tn = oracle.estimate_normals(tgt, 70.0, 40)[0].astype(np.float32) if mode == "p2plane" else None
    g = ops.icp(src, tgt, 100.0, None, mode, tn, want_corr=True)
    trace = []
    rT, rf, rr, rit = oracle.registration_icp(src, tgt, 100.0, None, mode, tn, trace=trace)
    assert g["iterations"] == rit and g["fitness"] == rf
    assert abs(g["inlier_rmse"] - rr) < 1e-9 * max(rr, 1)
    assert np.abs(g["transformation"] - rT).max() < TOL_T
    # correspondence search is bit-exact at every iteration when both sides use the same transform
    for Tk, idx, d2 in trace[:: max(1, len(trace) // 6)]:
        gi, gd = ops.nn_search(src, tgt, Tk)
        assert np.array_equal(npy(gi), idx) and np.array_equal(npy(gd), d2)
    if mode == "p2plane":
        assert np.abs(g["transformation"][:3, 3] - T[:3, 3]).max() < 3.0       # recovers the ground truth


def test_icp_random_problems_match_oracle(ops, oracle, base_cloud):
    """twelve seeded registrations (sizes 300 .. 6000, partial overlap, random motion up to ~8 deg / 60 mm, both estimators,
    random max_correspondence_distance): iterations and fitness equal, transform within tolerance"""
    rng = np.random.default_rng(31)
    for case in range(12):
        n, m = int(rng.integers(300, 6000)), int(rng.integers(300, 6000))
        tgt = base_cloud[rng.choice(len(base_cloud), m, replace=False)]
        src0 = base_cloud[rng.choice(len(base_cloud), n, replace=False)].astype(np.float64)
        if case % 3 == 0:
            src0 = src0[src0[:, 0] > np.median(src0[:, 0]) - 200]          # partial overlap
        ang = rng.uniform(-0.14, 0.14, 3)
        cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
        R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        src = ((src0 - src0.mean(0)) @ R.T + src0.mean(0) + rng.uniform(-60, 60, 3)).astype(np.float32)
        mode = "p2plane" if case % 2 else "p2p"
        tn = oracle.estimate_normals(tgt, 70.0, 40)[0].astype(np.float32) if mode == "p2plane" else None
        md = float(rng.choice([40.0, 100.0, 300.0]))
        g = ops.icp(src, tgt, md, None, mode, tn, 20)
        rT, rf, rr, rit = oracle.registration_icp(src, tgt, md, None, mode, tn, 20)
        assert g["iterations"] == rit and g["fitness"] == rf, (case, mode, n, m, md)
        assert np.abs(g["transformation"] - rT).max() < TOL_T, (case, mode)


def test_icp_engines_agree(ops, base_cloud):
    """culled and all-pairs engines: same iterations, fitness and correspondences (within max_dist); transforms agree
    to the tolerance of the reordered sums"""
    src, tgt, _ = synth.icp_pair(15000, base_cloud)
    out = {}
    for name in ("culled", "dense"):
        prev = ops.nn_engine(name)
        try:
            out[name] = ops.icp(src, tgt, 100.0, None, "p2p", None, 10, want_corr=True)
        finally:
            ops.nn_engine(prev)
    a, b = out["culled"], out["dense"]
    assert a["iterations"] == b["iterations"] and a["fitness"] == b["fitness"]
    assert np.abs(a["transformation"] - b["transformation"]).max() < TOL_T
    near = npy(b["d2"]) < 100.0 ** 2
    assert np.array_equal(npy(a["idx"])[near], npy(b["idx"])[near])
    assert np.allclose(npy(a["d2"])[near], npy(b["d2"])[near], rtol=1e-9, atol=1e-9)
    assert (npy(a["idx"])[~near] == -1).all() or (npy(a["d2"])[~near] >= 100.0 ** 2).all()


def test_icp_batch_equals_single_problems(ops, oracle, base_cloud, engine):
    """several subs onto one master, software-pipelined: same answers as one registration at a time"""
    src, tgt, T = synth.icp_pair(12000, base_cloud)
    tn = oracle.estimate_normals(tgt, 70.0, 40)[0].astype(np.float32)
    srcs = [src, src[:7001], oracle.transform(src, synth.t_star())[:9000]]
    inits = [np.eye(4), np.eye(4), np.linalg.inv(synth.t_star())]
    for mode, nrm in (("p2p", None), ("p2plane", tn)):
        batch = ops.icp_batch(srcs, tgt, 100.0, inits, mode, nrm, 12)
        for s, i0, b in zip(srcs, inits, batch):
            one = ops.icp(s, tgt, 100.0, i0, mode, nrm, 12)
            rT, rf, _, rit = oracle.registration_icp(s, tgt, 100.0, i0, mode, nrm, 12)
            assert rit == b["iterations"] and rf == b["fitness"] and np.abs(rT - b["transformation"]).max() < TOL_T, (mode, "batch vs oracle")
            assert rit == one["iterations"] and rf == one["fitness"] and np.abs(rT - one["transformation"]).max() < TOL_T, (mode, "single vs oracle")
            assert np.array_equal(b["transformation"], one["transformation"]), mode       # same kernels, same order


def test_icp_batch_more_problems_than_lanes(ops, base_cloud):
    """seven registrations onto one target (the library runs them on four internal lanes, two per lane at times): each
    equals the single-problem call bit for bit, whatever the interleaving"""
    rng = np.random.default_rng(8)
    src, tgt, T = synth.icp_pair(9000, base_cloud)
    srcs, inits = [], []
    for i in range(7):
        k = int(rng.integers(500, 9000))
        srcs.append(src[rng.choice(len(src), k, replace=False)])
        P = np.eye(4); P[:3, 3] = rng.uniform(-20, 20, 3)
        inits.append(P)
    for _ in range(2):                                            # twice: the lanes and pinned slots are reused
        batch = ops.icp_batch(srcs, tgt, 100.0, inits, "p2p", None, 9)
        for s_, i0, b in zip(srcs, inits, batch):
            one = ops.icp(s_, tgt, 100.0, i0, "p2p", None, 9)
            assert b["iterations"] == one["iterations"] and b["fitness"] == one["fitness"]
            assert np.array_equal(b["transformation"], one["transformation"])


def test_icp_batch_of_eight_sources_equals_single_problems(ops, base_cloud):
    """eight registrations onto one target: with the target one cloud more than the batch sort takes, so the batch's workspace is carved
    without the sort's scratch and every problem runs its own chain of launches -- each equals the single-problem call bit for bit"""
    src, tgt, _ = synth.icp_pair(4000, base_cloud)
    tn = ops.estimate_normals(torch.as_tensor(tgt).cuda(), 70.0, 40)
    srcs = [src[450 * i:450 * i + 200 + 57 * i] for i in range(8)]      # 200 .. 599 rows
    assert len(srcs) == 8 and all(200 <= len(s) <= 600 for s in srcs)
    inits = [np.eye(4)] * 8
    for mode, nrm in (("p2p", None), ("p2plane", tn)):
        batch = ops.icp_batch(srcs, tgt, 100.0, inits, mode, nrm, 6)
        for s_, b in zip(srcs, batch):
            one = ops.icp(s_, tgt, 100.0, None, mode, nrm, 6)
            assert b["iterations"] == one["iterations"] and b["fitness"] == one["fitness"], mode
            assert np.array_equal(b["transformation"], one["transformation"]), mode


def test_kabsch_pairs(ops, oracle, base_cloud):
    src, tgt, T = synth.icp_pair(5000, base_cloud)
    rng = np.random.default_rng(0)
    corr = np.stack([rng.choice(5000, 300, replace=False), rng.choice(5000, 300, replace=False)], 1).astype(np.int32)
    assert np.abs(ops.kabsch(src, tgt, corr) - oracle.kabsch(src[corr[:, 0]], tgt[corr[:, 1]])).max() < 1e-9
    s = rng.normal(scale=300, size=(3, 3)).astype(np.float32)        # minimum of 3 picked pairs
    t = oracle.transform(s, T)
    got = ops.kabsch(s, t, np.stack([np.arange(3), np.arange(3)], 1))
    assert np.abs(got - T).max() < 1e-3


# ------------------------------------------------------------------------------------- module-level APIs
def test_filter_outliers_and_remove_floor_chain(oracle):
    from kinectpy_amd.floor_removal import remove_floor
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.filtering import filter_outliers
    c3 = synth.filter_cloud(200_000)
    pcd = PointCloud(c3)
    before = np.asarray(pcd.points).copy()
    out = filter_outliers(pcd, nb_neighbors=20, std_ratio=2.0, voxel_size=10)
    assert np.array_equal(np.asarray(pcd.points), before)                    # input not mutated (deepcopy)
    vp, _, _ = oracle.voxel_downsample(c3, 10.0)
    keep, _, _ = oracle.sor(vp, 20, 2.0)
    assert np.array_equal(npy(out._pts), vp[keep])
    fl = remove_floor(out, seed=7)
    want, info = oracle.floor_removal(vp[keep], seed=7)
    assert np.array_equal(npy(fl._pts), want)
    assert len(want) < 0.7 * len(keep)                                        # the floor is gone


def test_default_filter_outliers_on_mm_data(oracle):
    """reference defaults (voxel 0.02 on millimetre data, k=200, ratio 3): every point its own voxel"""
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.filtering import filter_outliers
    p = synth.filter_cloud(30_000)
    out = filter_outliers(PointCloud(p))
    vp, _, _ = oracle.voxel_downsample(p, 0.02)
    keep, _, _ = oracle.sor(vp, 200, 3.0)
    assert np.array_equal(npy(out._pts), vp[keep])


def test_point_to_plane_registration_api(oracle):
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.registration import execute_point_to_plane_registration
    E0, E1 = synth.camera_pose(0, 8), synth.camera_pose(1, 8)
    xy = synth.xy_table()
    clouds = []
    for E, seed in ((E0, 100), (E1, 101)):
        dep = synth.render_depth(E, seed=seed, xy=xy)
        pts, _, _ = oracle.rgbd_compact(oracle.unproject_u16(dep, xy))
        clouds.append(pts)
    T_true = np.linalg.inv(E0) @ E1                       # sub -> master
    a = np.deg2rad(2.0)
    pert = np.eye(4)
    pert[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    pert[:3, 3] = [30, -20, 25]
    init = pert @ T_true
    master, sub = PointCloud(clouds[0]), PointCloud(clouds[1])
    T = execute_point_to_plane_registration(master, sub, init)
    # oracle: same call sequence (voxel 35, normals r=70 nn=40 on the master, ICP threshold 100)
    sd, _, _ = oracle.voxel_downsample(clouds[1], 35.0)
    md, _, _ = oracle.voxel_downsample(clouds[0], 35.0)
    mn = oracle.estimate_normals(md, 70.0, 40)[0].astype(np.float32)
    from kinectpy_amd import o3d
    mn_gpu = np.asarray(PointCloud(md).estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(70.0, 40)).normals).astype(np.float32)
    oT, _, _, _ = oracle.registration_icp(sd, md, 100.0, init, "p2plane", mn_gpu)
    assert np.abs(T - oT).max() < 1e-6
    assert np.abs(T[:3, 3] - T_true[:3, 3]).max() < 15 and np.abs(T[:3, :3] - T_true[:3, :3]).max() < 5e-3
    assert (np.abs((mn * mn_gpu.astype(np.float64)).sum(1)) > 0.999).mean() > 0.95


# ----------------------------------------------------------------- global registration (rows a11-a13)
@pytest.fixture(scope="module")
def two_views(oracle):
    """two cluttered views 22.5 degrees apart, voxel 50 (keeps the oracle's brute-force feature matching short)"""
    xy = synth.xy_table()
    ex = synth.clutter()
    out = []
    for i, seed in ((0, 100), (1, 101)):
        E = synth.camera_pose(i, 16)
        dep = synth.render_depth(E, seed=seed, xy=xy, extra=ex)
        p, _, _ = oracle.rgbd_compact(oracle.unproject_u16(dep, xy))
        out.append((E, oracle.voxel_downsample(p, 50.0)[0]))
    return out


def test_fpfh_matches_oracle(ops, oracle, two_views):
    for _, d in two_views:
        nrm = npy(ops.estimate_normals(d, 100.0, 40))              # the oracle gets the same float32 normals
        got = npy(ops.fpfh(d, nrm, 250.0, 40))
        want, _ = oracle.fpfh(d, nrm, 250.0, 40)
        assert got.shape == want.shape == (len(d), 33)
        # histogram sums: 3 x 100 from SPFH (+ 3 x 100 weighted) for every point with neighbours
        assert np.allclose(got.sum(1)[want.sum(1) > 0], 600.0, atol=1e-6)
        bad = np.abs(got - want).max(1) > 1e-6                      # a libm atan2 ulp can move one pair across a bin edge
        assert bad.mean() < 1e-3
        assert np.allclose(got[~bad], want[~bad], rtol=1e-9, atol=1e-9)


def test_feature_matching_and_ransac_match_oracle(ops, oracle, two_views):
    (E0, tgt), (E1, src) = two_views
    feats = []
    for d in (src, tgt):
        nrm = npy(ops.estimate_normals(d, 100.0, 40))
        feats.append(oracle.fpfh(d, nrm, 250.0, 40)[0])            # identical features on both sides
    gi = npy(ops.feature_nn(feats[0], feats[1]))
    assert np.array_equal(gi, oracle.feature_nn(feats[0], feats[1]))          # bit-exact 33-D nearest neighbour
    corr = ops.feature_correspondences(feats[0], feats[1], True, 3)
    assert np.array_equal(corr, oracle.feature_correspondences(feats[0], feats[1], True, 3))
    for seed, iters in ((1, 60000), (2, 20000)):
        g = ops.ransac_corres(src, tgt, corr, 75.0, 3, 0.95, iters, 0.999, seed)
        oT, ost = oracle.ransac_corres(src, tgt, corr, 75.0, 3, 0.95, iters, 0.999, seed)
        assert g["iterations"] == ost["iterations"] and g["validations"] == ost["validations"]
        assert g["fitness"] == ost["fitness"] and abs(g["inlier_rmse"] - ost["rmse"]) < 1e-9
        assert np.abs(g["transformation"] - oT).max() < 1e-6


def test_execute_global_registration_recovers_pose(oracle, two_views):
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.preprocessing.registration import execute_global_registration, execute_point_to_plane_registration
    (E0, tgt), (E1, src) = two_views
    T_true = np.linalg.inv(E0) @ E1
    master, sub = PointCloud(tgt), PointCloud(src)
    T0 = execute_global_registration(master, sub, voxel_size=50, ransac_n_trials=3, seed=5)
    assert T0 is not None
    ang = np.degrees(np.arccos(np.clip((np.trace(T0[:3, :3].T @ T_true[:3, :3]) - 1) / 2, -1, 1)))
    assert ang < 6.0 and np.abs(T0[:3, 3] - T_true[:3, 3]).max() < 250.0          # coarse: good enough to start ICP
    T1 = execute_point_to_plane_registration(master, sub, T0, voxel_size=50)       # the reference's next step (data.py:156-157)
    ang = np.degrees(np.arccos(np.clip((np.trace(T1[:3, :3].T @ T_true[:3, :3]) - 1) / 2, -1, 1)))
    assert ang < 0.5 and np.abs(T1[:3, 3] - T_true[:3, 3]).max() < 15.0


def test_data_processor_frame(oracle):
    from kinectpy_amd.preprocessing.data import DataProcessor
    xy = synth.xy_table()
    S = 2
    Es = [synth.camera_pose(i, 8) for i in range(S)]
    deps = [synth.render_depth(E, seed=200 + i, xy=xy) for i, E in enumerate(Es)]
    xyzs = [oracle.unproject_u16(d, xy) for d in deps]
    rgbs = [synth.person_mask_rgb(d, E) for d, E in zip(deps, Es)]
    Ts = [np.linalg.inv(Es[0]) @ Es[i] for i in range(1, S)]
    dp = DataProcessor.in_memory(S)
    dp.registration_transformations = Ts
    fused = dp.process_frame(rgbs, xyzs)
    parts, cols = [], []
    for i in range(S):
        p, c, _ = oracle.rgbd_compact(xyzs[i], rgbs[i], True, True, oracle.median_z(xyzs[i]) + 750.0)
        parts.append(p)
        cols.append(c)
    # transform + vstack + voxel_down_sample(0.02) on the fp64 values of the moved points (data.py:44-61, float64 in the reference)
    vp, vc = oracle.fuse_voxel_downsample(parts, cols, [np.eye(4)] + Ts, 0.02)
    keep, _, _ = oracle.sor(vp, 200, 3.0)
    assert np.array_equal(npy(fused._pts), vp[keep]) and np.array_equal(npy(fused._col), vc[keep])
    assert len(keep) > 1000


def test_pcd_io_round_trip(tmp_path):
    from kinectpy_amd import o3d
    rng = np.random.default_rng(0)
    pcd = o3d.geometry.PointCloud(rng.normal(scale=1000, size=(500, 3)))
    pcd.colors = rng.integers(0, 256, size=(500, 3)) / 255.0
    fp = str(tmp_path / "a.pcd")
    o3d.io.write_point_cloud(fp, pcd)
    back = o3d.io.read_point_cloud(fp)
    assert np.array_equal(np.asarray(back.points), np.asarray(pcd.points))
    assert np.allclose(np.asarray(back.colors), np.asarray(pcd.colors), atol=1e-6)
    both = pcd + back
    assert len(both.points) == 1000 and both.has_colors()
    c = copy.deepcopy(pcd)
    c.transform(synth.t_star())
    assert not np.array_equal(np.asarray(c.points), np.asarray(pcd.points))


def test_extract_writes_dat_files(tmp_path, oracle):
    from kinectpy_amd.preprocessing.extractor import MKVFilesProcessing
    from kinectpy_amd.utils.io import load_depth
    xy = synth.xy_table()
    # timestamps: ordinary, zero-padded ("0123": kept -- only the NAME "0_..." marks an empty frame, extractor.py:150-154), and 0
    frames = [(1000 + 33 * i, synth.render_depth(seed=i, xy=xy)) for i in range(3)]
    frames += [("0123", synth.render_depth(seed=7, xy=xy)), (0, synth.render_depth(seed=8, xy=xy))]
    m = MKVFilesProcessing(["a.mkv"], [str(tmp_path / "master_1")], frame_source=lambda fp: (xy, iter(frames)))
    m.extract(pointcloud=True, batch=2)
    for ts, d in frames[:4]:
        got = load_depth(str(tmp_path / "master_1" / "depths" / str(ts)))
        assert np.array_equal(got, oracle.unproject_u16(d, xy))
    assert not (tmp_path / "master_1" / "depths" / "0_depth.dat").exists()


# ----------------------------------------------------------------------------- BASELINE.json full sizes
def test_full_size_icp_pair_nn(ops, oracle, base_cloud):
    """config 2: 100k x 100k correspondence search, bit-exact against the (grid-accelerated) oracle"""
    src, tgt, T = synth.icp_pair(100_000, base_cloud)
    gi, gd = ops.nn_search(src, tgt, np.eye(4))
    ri, rd, _ = oracle.nn(src, np.eye(4), tgt, grid=True)
    assert np.array_equal(npy(gi), ri) and np.array_equal(npy(gd), rd)
    # size-independent properties: the reported distance is the distance of the reported pair, and no
    # sampled target is closer
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    assert np.allclose(((s64 - t64[npy(gi)]) ** 2).sum(1), npy(gd), rtol=1e-12)
    probe = np.random.default_rng(0).choice(len(tgt), 64, replace=False)
    assert (((s64[:, None, :] - t64[probe][None]) ** 2).sum(2).min(1) >= npy(gd) * (1 - 1e-12)).all()


def test_full_size_filter_chain(ops, oracle):
    """config 3: 1M points, voxel 10 mm -> SOR(20, 2.0) -> slab -> RANSAC plane(30,30,2000,seed 7)"""
    c3 = synth.filter_cloud(1_000_000)
    vp, _, _ = ops.voxel_downsample(c3, 10.0)
    rv, _, _, cnt = oracle.voxel_downsample(c3, 10.0, return_counts=True)
    assert np.array_equal(npy(vp), rv) and cnt.sum() == len(c3)
    gi, gs, _ = ops.sor(vp, 20, 2.0)
    ri, rs, _ = oracle.sor(rv, 20, 2.0)
    assert np.array_equal(npy(gi), ri) and np.allclose(npy(gs), rs, rtol=TOL_STATS)
    cloud = rv[ri]
    lo, up = ops.slab_split(cloud, 200.0)
    floor = cloud[npy(lo)]
    gpl, gidx = ops.segment_plane(floor, 30.0, 30, 2000, seed=7)
    rpl, ridx = oracle.segment_plane(floor, 30.0, 30, 2000, seed=7)
    assert np.array_equal(npy(gidx), ridx) and np.abs(gpl - rpl).max() < TOL_PLANE
    assert abs(abs(gpl[1]) - 1) < 1e-4 and abs(abs(gpl[3]) - 900) < 3.0       # it is the floor
    # the tail of floor_removal.py:71-73 at full size: select_by_index(inliers, invert=True), outlier_cloud + upper, SOR(50, 0.30)
    rest, = ops.select_by_index([torch.as_tensor(floor).cuda()], gidx, invert=True)[:1]
    upper = cloud[npy(up)]
    joined = np.concatenate([npy(rest), upper])
    r_rest = np.delete(floor, ridx, axis=0)
    assert np.array_equal(joined, np.concatenate([r_rest, upper])) and len(joined) > 100_000
    gi2, gs2, _ = ops.sor(joined, 50, 0.30)
    ri2, rs2, _ = oracle.sor(joined, 50, 0.30)
    assert np.array_equal(npy(gi2), ri2) and np.allclose(npy(gs2), rs2, rtol=TOL_STATS)
    assert 0.3 * len(joined) < len(ri2) < len(joined)


def test_configs_2_and_3_against_the_float64_storage_oracle(ops, oracle, base_cloud):
    """The reference keeps clouds in float64 between stages (utils/io.py:29-41), the product in float32 with fp64 decisions
    (DESIGN 3).  The HIP path against the oracle built with float64 storage (libkpx_oracle_f64), on float32-representable inputs
    (sensor data, .pcd files): index decisions equal, coordinates within the float32 rounding of the stored values.  Stated
    tolerances: voxel means 3e-4 mm (2^-24 relative at 5 m); SOR statistics 1e-5 relative (they are means of distances between
    rounded means); registrations: same fitness, iteration counts within one (the convergence test may sit on the edge),
    T within 1e-4 for point to plane and 2e-3 for point to point run to its 30-iteration cap."""
    # config 3
    c3 = synth.filter_cloud(1_000_000)
    assert c3.dtype == np.float32
    vp, _, _ = ops.voxel_downsample(c3, 10.0)
    gi, gs, _ = ops.sor(vp, 20, 2.0)
    with oracle.storage("f64"):
        rv, _, _, cnt = oracle.voxel_downsample(c3.astype(np.float64), 10.0, return_counts=True)
        ri, rs, _ = oracle.sor(rv, 20, 2.0)
    assert rv.dtype == np.float64 and len(vp) == len(rv)                         # voxel membership is the float64 path's
    assert np.abs(npy(vp).astype(np.float64) - rv).max() < 3e-4
    assert np.allclose(npy(gs), rs, rtol=1e-5)
    assert len(np.setxor1d(npy(gi), ri)) <= 2                                    # a point whose mean distance sits within 1e-6 of the threshold may flip
    # config 2
    src, tgt, _ = synth.icp_pair(100_000, base_cloud)
    for mode, tol in (("p2plane", 1e-4), ("p2p", 2e-3)):
        with oracle.storage("f64"):
            tn64 = oracle.estimate_normals(tgt.astype(np.float64), 70.0, 40)[0] if mode == "p2plane" else None
            rT, rf, rr, rit = oracle.registration_icp(src.astype(np.float64), tgt.astype(np.float64), 100.0, None, mode, tn64, 30, grid=True)
        tn = ops.estimate_normals(tgt, 70.0, 40) if mode == "p2plane" else None
        g = ops.icp(src, tgt, 100.0, None, mode, tn, 30)
        assert abs(g["iterations"] - rit) <= 1 and abs(g["fitness"] - rf) <= 2e-5, mode
        assert np.abs(g["transformation"] - rT).max() < tol and abs(g["inlier_rmse"] - rr) < 1e-4, mode


_RCCL_ONE_RANK = r"""
import os, sys, torch
os.environ.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
import torch.distributed as dist
from kinectpy_amd import parallel
torch.cuda.set_device(0)
dist.init_process_group(backend="nccl", rank=0, world_size=1)
g = torch.Generator().manual_seed(1)
buf = torch.rand((4096, 6), generator=g).cuda()
T = torch.rand((4, 4, 4), dtype=torch.float64, generator=g)
cloud, all_T, counts = parallel.allgather_clouds(buf, 3000, T, always_collective=True)
assert counts == [3000] and torch.equal(cloud, buf[:3000]) and torch.equal(all_T.cpu(), T)
cloud, all_T, counts = parallel.allgather_clouds(buf, 5000, T, always_collective=True)      # overflow: header says 5000
assert counts == [5000] and cloud.shape[0] == 4096
parallel.barrier()
assert parallel.allreduce_max(2.5, buf.device) == 2.5
# the north-star partition through RCCL on a one-rank group: broadcast, all_gather_into_tensor and the slab all-gather on device
# tensors, serially and with two frames in flight (one communicator per slot) -- same result as without any collective
import numpy as np
from kinectpy_amd.pipeline import FrameStream, PipelineParams, SensorShardPipeline
from kinectpy_amd.utils import synth
xy, depth, rgb, inits, _ = synth.sensor_ring(2, 2, synth.small_xy(2))
d, c = torch.as_tensor(depth).cuda(), torch.as_tensor(rgb).cuda()
plain = SensorShardPipeline(xy, 2, inits, PipelineParams())
want = [plain.step(d[f], c[f]) for f in range(2)]
parallel.FORCE_COLLECTIVES = True
for mode in ("sharded", "rank0"):
    pipe = SensorShardPipeline(xy, 2, inits, PipelineParams(), fused_filter=mode, cloud_capacity=4096)
    for rep in range(2):
        for f in range(2):
            p_, c_, T_ = pipe.step(d[f], c[f])
            assert torch.equal(p_, want[f][0]) and torch.equal(c_, want[f][1]) and np.array_equal(T_, want[f][2]), (mode, rep, f)
groups = [parallel.new_group() for _ in range(2)]
assert all(g is not None for g in groups)
for g in groups:
    parallel.warm(g, d.device)
fs = FrameStream([SensorShardPipeline(xy, 2, inits, PipelineParams(), group=g, cloud_capacity=4096) for g in groups])
got = []
for k in range(5):
    if fs.full():
        got.append(fs.pop())
    fs.submit(d[k % 2], c[k % 2])
while fs.pending:
    got.append(fs.pop())
fs.close()
for k, (p_, c_, T_) in enumerate(got):
    assert torch.equal(p_, want[k % 2][0]) and torch.equal(c_, want[k % 2][1])
parallel.FORCE_COLLECTIVES = False
dist.destroy_process_group()
print("rccl-ok")
"""


def test_rccl_exchange_on_one_rank():
    """the fuse exchange through RCCL itself (backend "nccl"), on the one GPU a test box has: a one-rank group runs
    the same all_gather_into_tensor / all_reduce / barrier calls the N-GPU bench makes (the multi-rank logic is
    covered on CPU with gloo, tests/test_dist_cpu.py)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _RCCL_ONE_RANK], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rccl-ok" in r.stdout, r.stderr[-2000:]


# ---- sampler / oriented bounding box / normalisers --------------------------------------
def _hull_clouds():
    rng = np.random.default_rng(11)
    c = {}
    for n in (4, 9, 100, 4096):
        c[f"gauss{n}"] = (rng.normal(size=(n, 3)) * [300, 900, 200]).astype(np.float32)
    s = rng.normal(size=(3000, 3))
    c["sphere"] = (s / np.linalg.norm(s, axis=1)[:, None]).astype(np.float32)      # 5996 facets: the edge set leaves LDS
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    c["lattice"] = g[rng.permutation(len(g))]
    p = rng.normal(size=(400, 3)).astype(np.float32)
    c["duplicates"] = np.concatenate([p, p, p[:50]])
    c3 = synth.filter_cloud(60000)
    c["scene"] = c3                                                                 # > 16384 points: 1024-thread block
    c["scene_int_mm"] = np.round(c3[:30000]).astype(np.float32)
    return c


def test_sample_points_equal_oracle(ops, oracle, base_cloud):
    for n, k, seed in [(1000, 100, 7), (len(base_cloud), 4096, 1234), (4096, 4096, 3), (5, 1, 0), (70000, 4096, 2 ** 63 + 5)]:
        p = base_cloud[:n] if n <= len(base_cloud) else np.tile(base_cloud, (2, 1))[:n]
        pts, idx = ops.sample_points(p, k, seed)
        ref = oracle.sample_indices(n, k, seed)
        assert np.array_equal(idx.cpu().numpy(), ref)
        assert np.array_equal(pts.cpu().numpy(), p[ref])
    _, idx = ops.sample_points(base_cloud[:100], 0, 1)
    assert idx.numel() == 0
    with pytest.raises(ValueError):
        ops.sample_points(base_cloud[:10], 11, 0)


def test_hull_vertices_bit_exact_and_obb(ops, oracle):
    for name, p in _hull_clouds().items():
        for dt in (np.float32, np.float64):
            obb, flags = ops.obb_batch(torch.as_tensor(p.astype(dt))[None], want_vertices=True)
            got = np.flatnonzero(flags[0].cpu().numpy())
            ref = oracle.hull_vertices(p)
            assert np.array_equal(got, ref), (name, dt)
            row = obb[0].cpu().numpy()
            assert row[15] == len(ref)
            if name == "lattice":
                continue
            R, c, ext = oracle.obb_from_vertices(p[ref])
            scale = np.abs(p).max()
            assert np.allclose(row[:9].reshape(3, 3), R, atol=1e-7), name           # eigenvectors: gap-dependent conditioning
            assert np.allclose(row[9:12], c, atol=1e-7 * scale) and np.allclose(row[12:15], ext, rtol=1e-7), name


def test_obb_batch_of_training_clouds(ops, oracle, base_cloud):
    rng = np.random.default_rng(4)
    B, N = 24, 4096
    x = np.stack([base_cloud[rng.choice(len(base_cloud), N, replace=False)] + rng.normal(size=3) * 100 for _ in range(B)]).astype(np.float64)
    x += rng.normal(size=x.shape) * 1e-3                                            # float64 payload, not f32-representable
    obb, flags = ops.obb_batch(x, want_vertices=True)
    fl = flags.cpu().numpy()
    for b in range(B):
        assert np.array_equal(np.flatnonzero(fl[b]), _hull_f64(oracle, x[b]))


def _hull_f64(oracle, p):
    """the oracle's hull on float64 points"""
    return oracle.hull_vertices_f64(p)


def test_obb_degenerate_clouds(ops):
    from kinectpy_amd._lib import KinectPxError
    line = np.stack([np.arange(10.0)] * 3, 1)
    for bad in (line, np.zeros((5, 3)), np.zeros((2, 3)), np.c_[np.random.default_rng(0).normal(size=(50, 2)), np.zeros(50)]):
        with pytest.raises(KinectPxError):
            ops.obb_batch(bad)
    good = np.random.default_rng(1).normal(size=(50, 3))
    obb, _ = ops.obb_batch(np.stack([good, good * 2]))
    assert (obb[:, 15] > 3).all()
    obb, _ = ops.obb_batch(np.stack([good, np.zeros((50, 3))]), check=False)     # per-cloud status, no exception
    st = obb[:, 15].cpu().numpy()
    assert st[0] > 3 and st[1] == -1


def test_normalisation_batches_match_oracle(oracle, base_cloud):
    from kinectpy_amd.utils import normalization as Nz
    rng = np.random.default_rng(9)
    B, N, K = 6, 2048, 13
    x = np.stack([base_cloud[rng.choice(len(base_cloud), N, replace=False)] for _ in range(B)]).astype(np.float64)
    y = rng.normal(size=(B, 3 * K)) * 500
    boxes = []
    for b in range(B):
        boxes.append(oracle.obb_from_vertices(x[b][oracle.hull_vertices_f64(x[b])]))
    for name in ("obb_normalization_batch", "obb_rotation_translation_batch", "translation_normalization_batch"):
        gx, gy = getattr(Nz, name)(x, y)
        rx, ry = getattr(oracle, name)(x, y, boxes)
        assert gx.shape == rx.shape and gy.shape == ry.shape and gx.dtype == np.float64
        assert np.allclose(gx, rx, rtol=0, atol=1e-6 if "translation_norm" not in name else 1e-7), name
        assert np.allclose(gy, ry, rtol=0, atol=1e-6), name
    gx, gy = Nz.scale_batch(x, y)
    assert np.array_equal(gx, x * (1 / 1000)) and np.array_equal(gy, y * (1 / 1000))
    gx, gy = Nz.rotate_batch(x, y, degs=37)
    a = np.deg2rad(37.0)
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    assert np.allclose(gx, x @ rot, atol=1e-9) and np.allclose(gy.reshape(B, K, 3), y.reshape(B, K, 3) @ rot, atol=1e-9)
    assert set(Nz.normalization_options) == {"obb_normalization", "obb_rotation_translation", "translation"}


def _box_tensor(boxes):
    """[(R, centre, extent)] -> the (B, 16) box tensor of kpx_obb_batch [R row-major | centre | extent | status]"""
    rows = [np.concatenate([np.asarray(b["R"], dtype=np.float64).reshape(-1), b["centre"], b["extent"], [8.0]]) for b in boxes]
    return torch.as_tensor(np.stack(rows)).cuda()


def test_normalisers_match_reference_kat(ops):
    """The HIP normalisers against the reference's OWN outputs (utils/processing.py:313-354, utils/normalization.py:16-159
    executed around a stub box: tests/golden/make_ref_norm_kat.py).  Tolerance: the kernels evaluate the affine maps in fp64
    in one fixed order, NumPy's matmul in another: 1e-9 absolute on millimetre-sized values."""
    from kinectpy_amd import o3d
    from kinectpy_amd.utils import normalization as Nz
    from kinectpy_amd.utils import processing as P
    for c in NORM_KAT["normalize_pointcloud"]:
        pcd = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(np.array(c["pts"])))
        got = np.asarray(P.normalize_pointcloud(pcd, c["min_range"], c["max_range"]).points)
        span = c["max_range"] - c["min_range"]
        assert np.allclose(got, np.array(c["out"]), rtol=0, atol=span * 2.0 ** -22)      # the cloud is stored as float32
    for c in NORM_KAT["obb_normalization"]:
        xo, jo = P.obb_normalization(np.array(c["pts"]), np.array(c["joints"]), c["number_of_joints"], _obb=_box_tensor([c]))
        assert np.allclose(xo, np.array(c["points_out"]), rtol=0, atol=1e-9) and np.allclose(jo, np.array(c["joints_out"]), rtol=0, atol=1e-9)
    b = NORM_KAT["batch"]
    x, y, obb = np.array(b["x"]), np.array(b["y"]), _box_tensor(b["boxes"])
    rz90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    for name, mode, M in (("obb_normalization_batch", ops.NORM_OBB, np.array(b["M"])), ("obb_rotation_translation_batch", ops.NORM_OBB_ROT_TRANS, rz90),
                          ("translation_normalization_batch", ops.NORM_TRANSLATE, None)):
        gx, gy = Nz._apply(x, y, mode, M, obb=obb)
        assert np.allclose(gx, np.array(b[name]["x"]), rtol=0, atol=1e-9), name
        assert np.allclose(gy, np.array(b[name]["y"]), rtol=0, atol=1e-9), name
    gx, gy = Nz.scale_batch(x, y)
    assert np.array_equal(gx, np.array(b["scale_batch"]["x"])) and np.array_equal(gy, np.array(b["scale_batch"]["y"]))
    gx, gy = Nz.scale_batch(x, y, 2.5)
    assert np.array_equal(gx, np.array(b["scale_batch_2p5"]["x"])) and np.array_equal(gy, np.array(b["scale_batch_2p5"]["y"]))
    gx, gy = Nz.rotate_batch(x, y, degs=b["rotate_batch"]["degs"])
    assert np.allclose(gx, np.array(b["rotate_batch"]["x"]), rtol=0, atol=1e-9) and np.allclose(gy, np.array(b["rotate_batch"]["y"]), rtol=0, atol=1e-9)


def test_processing_mirrors(oracle, base_cloud, tmp_path):
    from kinectpy_amd import o3d
    from kinectpy_amd.utils import processing as P
    pcd = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(base_cloud[:50000].astype(np.float64)))
    s = P.select_points_randomly(pcd, 4096, seed=5)
    assert s.shape == (4096, 3) and s.dtype == np.float64
    assert np.array_equal(s, base_cloud[:50000][oracle.sample_indices(50000, 4096, 5)].astype(np.float64))
    np.random.seed(3)
    a = P.select_points_randomly(pcd, 100)
    np.random.seed(3)
    assert np.array_equal(a, P.select_points_randomly(pcd, 100))                  # np.random.seed governs the default draw
    with pytest.raises(ValueError):
        P.select_points_randomly(pcd, 50001)
    box = pcd.get_oriented_bounding_box()
    R, c, ext = oracle.oriented_bounding_box(base_cloud[:50000])
    assert np.allclose(box.R, R, atol=1e-7) and np.allclose(box.get_center(), c, atol=1e-4) and np.allclose(box.extent, ext, rtol=1e-7)
    assert np.allclose(box.get_rotation_matrix_from_yxz([0, np.pi, 0]), oracle.rotation_matrix_from_yxz([0, np.pi, 0]), atol=0)
    xo, jo = P.obb_normalization(base_cloud[:3000], np.arange(12.0), 4)
    Rb, cb, _ = oracle.oriented_bounding_box(base_cloud[:3000])
    assert np.allclose(xo, (base_cloud[:3000].astype(np.float64) - cb) @ Rb, atol=1e-6) and jo.shape == (12,)
    n = P.normalize_pointcloud(pcd.clone())
    arr = np.asarray(n.points)
    assert np.allclose(arr, oracle.normalize_pointcloud(base_cloud[:50000]), atol=1e-6)
    sc = P.scale_point_cloud(pcd)
    assert np.allclose(np.asarray(sc.points), base_cloud[:50000] * 0.001, rtol=1e-6)
    P.save_points_npz(str(tmp_path / "1.npz"), pcd, 4096, seed=1)
    assert np.load(str(tmp_path / "1.npz"))["points"][:4096].shape == (4096, 3)


def test_frame_stream_equals_serial_steps():
    """pipeline.FrameStream (two frames in flight, each on its own host thread and stream) returns, in order, exactly what
    one step after the other returns"""
    import bench
    from kinectpy_amd.pipeline import FrameStream, PipelineParams, SensorGroupPipeline
    xy, depth_h, rgb_h, inits, truth, _ = bench.make_group(0, 1, 4, 3)
    depth = torch.as_tensor(depth_h).cuda()
    rgb = torch.as_tensor(rgb_h).cuda()
    pipe = SensorGroupPipeline(xy, inits, PipelineParams())
    serial = [pipe.step(depth[f % 3], rgb[f % 3]) for f in range(7)]
    fs = FrameStream(pipe, 2)
    got = []
    for f in range(7):
        if fs.full():
            got.append(fs.pop())
        fs.submit(depth[f % 3], rgb[f % 3])
    while fs.pending:
        got.append(fs.pop())
    fs.close()
    assert len(got) == 7
    for (p0, c0, T0), (p1, c1, T1) in zip(serial, got):
        assert torch.equal(p0, p1) and torch.equal(c0, c1) and np.array_equal(T0, T1)


def test_skeleton_fusion_matches_reference_outputs(ops, oracle):
    """kpx_fuse_skeletons against the reference's own results (golden vectors) and the oracle on a longer sequence"""
    from kinectpy_amd.utils.skeleton_fusion import fuse_skeletons_gradient
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_skeleton_fusion.json")))
    for c in kat["fuse_skeletons_gradient"]:
        got = fuse_skeletons_gradient(np.array(c["skeletons"]), c["alpha"], c["beta"])
        assert got.dtype == np.float64 and np.allclose(got, np.array(c["fused"]), rtol=1e-10, atol=1e-8)
    rng = np.random.default_rng(3)
    truth = np.cumsum(rng.normal(scale=4.0, size=(400, 32, 3)), axis=0)
    sk = np.stack([truth + rng.normal(scale=s, size=truth.shape) for s in (2.0, 6.0, 12.0, 50.0)])      # a fourth camera is ignored after frame 20
    got = ops.fuse_skeletons(sk, 1.4, 1.4).cpu().numpy()
    assert np.allclose(got, oracle.fuse_skeletons_gradient(sk, 1.4, 1.4), rtol=1e-9, atol=1e-7)
    from kinectpy_amd._lib import KinectPxError
    with pytest.raises(KinectPxError):
        ops.fuse_skeletons(sk[:2], 1.4, 1.4)


_coloured_pair = synth.coloured_pair


def test_colour_gradient_and_coloured_icp_match_oracle(ops, oracle, engine):
    src, sc, tgt, tc, T = _coloured_pair(6000)
    tn = oracle.estimate_normals(tgt, 70.0, 30)[0].astype(np.float32)
    g = ops.color_gradient(tgt, tn, tc, 160.0, 30).cpu().numpy()
    rg = oracle.color_gradient(tgt, tn, tc, 160.0, 30)
    assert np.allclose(g, rg, rtol=1e-7, atol=1e-10)
    for lam, iters, init in ((0.968, 25, None), (0.5, 8, np.linalg.inv(np.linalg.inv(T))), (1.0, 6, None)):
        r = ops.colored_icp(src, sc, tgt, tc, tn, 80.0, init, lam, iters)
        rT, rf, rr, rit = oracle.registration_colored_icp(src, sc, tgt, tc, tn, 80.0, init, lam, iters)
        assert r["iterations"] == rit and r["fitness"] == rf and abs(r["inlier_rmse"] - rr) < 1e-8
        assert np.abs(r["transformation"] - rT).max() < TOL_T
    r = ops.colored_icp(src, sc, tgt, tc, tn, 80.0, None, 0.968, 40)
    assert np.abs(r["transformation"][:3, :3] - T[:3, :3]).max() < 5e-3 and np.abs(r["transformation"][:3, 3] - T[:3, 3]).max() < 6.0
    # lambda = 1 drops the photometric row: the update is the point-to-plane one
    a = ops.colored_icp(src, sc, tgt, tc, tn, 80.0, None, 1.0, 5)
    b = ops.icp(src, tgt, 80.0, None, "p2plane", tn, 5)
    assert a["iterations"] == b["iterations"] and np.abs(a["transformation"] - b["transformation"]).max() < 1e-9


def test_coloured_icp_api_mirrors(oracle):
    from kinectpy_amd import o3d
    from kinectpy_amd.preprocessing.registration import execute_colored_ICP_registration
    src, sc, tgt, tc, T = _coloured_pair(20000)
    a = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(src.astype(np.float64)))
    b = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(tgt.astype(np.float64)))
    with pytest.raises(RuntimeError):
        o3d.pipelines.registration.registration_colored_icp(a, b, 80.0, np.eye(4))       # no normals
    b.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(radius=70.0, max_nn=30))
    with pytest.raises(RuntimeError):
        o3d.pipelines.registration.registration_colored_icp(a, b, 80.0, np.eye(4))       # no colours
    a.colors = o3d.utility.Vector3dVector(sc.astype(np.float64))
    b.colors = o3d.utility.Vector3dVector(tc.astype(np.float64))
    res = o3d.pipelines.registration.registration_colored_icp(
        a, b, 80.0, np.eye(4), o3d.pipelines.registration.TransformationEstimationForColoredICP(),
        o3d.pipelines.registration.ICPConvergenceCriteria(relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30))
    assert res.fitness > 0.9 and np.abs(res.transformation[:3, 3] - T[:3, 3]).max() < 8.0
    Tm = execute_colored_ICP_registration(a, b, np.eye(4))                                   # the reference's three-scale loop
    assert Tm.shape == (4, 4) and np.abs(Tm[:3, :3] - T[:3, :3]).max() < 2e-2


def test_two_ranks_share_one_gpu(tmp_path):
    """the N > 1 path on device tensors: two ranks (gloo, both on this GPU) run the frame pipeline with two frames in flight and
    exchange every frame; each rank must end up with rank 0's cloud followed by rank 1's, moved into the global frame"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KPX_DIST_BACKEND="gloo", OUT_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29591", os.path.join(root, "tests", "dist_gpu_worker.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = np.load(str(tmp_path / "rank0.npz")), np.load(str(tmp_path / "rank1.npz"))
    for i in range(3):
        assert np.array_equal(a[f"all_p{i}"], b[f"all_p{i}"]) and np.array_equal(a[f"all_c{i}"], b[f"all_c{i}"])
        assert np.array_equal(a[f"all_T{i}"], b[f"all_T{i}"]) and a[f"counts{i}"].tolist() == b[f"counts{i}"].tolist()
        n0, n1 = a[f"counts{i}"].tolist()
        assert n0 == len(a[f"own_p{i}"]) and n1 == len(b[f"own_p{i}"]) and len(a[f"all_p{i}"]) == n0 + n1
        for rank, own in ((0, a), (1, b)):
            G = own["to_global"]
            want = (own[f"own_p{i}"].astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
            part = a[f"all_p{i}"][:n0] if rank == 0 else a[f"all_p{i}"][n0:]
            assert np.abs(part - want).max() < 1e-2
            assert np.allclose(a[f"all_T{i}"][2 * rank:2 * rank + 2], np.stack([G @ T for T in own[f"own_T{i}"]]), atol=1e-12)


# ------------------------------------------------------------------ pipeline-level parity and the north-star partition
def _oracle_steps(oracle, S, frames):
    from kinectpy_amd.pipeline import PipelineParams
    xy, depth, rgb, inits, truth = synth.sensor_ring(S, frames)
    return xy, depth, rgb, inits, truth, [oracle.pipeline_step(xy, depth[f], rgb[f], inits, PipelineParams()) for f in range(frames)]


@pytest.fixture(scope="module")
def four_sensor_oracle(oracle):
    return _oracle_steps(oracle, 4, 2)


def test_pipeline_step_equals_oracle_full_size(ops, oracle, four_sensor_oracle):
    """BASELINE configs[3] on one GPU: one full-size 4-sensor step (extract -> pairwise point-to-plane ICP -> transform ->
    fuse -> voxel + SOR; preprocessing/data.py:35-61, 127-161) of BOTH pipelines against the oracle step: fused cloud and
    colours identical, transforms within TOL_T, iterations and fitness of every registration equal"""
    from kinectpy_amd.pipeline import PipelineParams, SensorGroupPipeline, SensorShardPipeline
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    d, c = torch.as_tensor(depth).cuda(), torch.as_tensor(rgb).cuda()
    for make in (lambda: SensorGroupPipeline(xy, inits, PipelineParams()), lambda: SensorShardPipeline(xy, 4, inits, PipelineParams())):
        pipe = make()
        for f in range(2):
            gp, gc, gT = pipe.step(d[f], c[f])
            rp, rc, rT, aux = ref[f]
            assert np.abs(gT - np.stack(rT)).max() < TOL_T
            assert [(it, fit) for it, fit, _ in pipe.last["icp"]] == [(it, fit) for it, fit, _ in aux["icp"]]
            assert pipe.last["n_down"] == [len(x) for x in aux["downs"]] and pipe.last["n_fused"] == len(aux["fused"])
            assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc)
            # (how close a registration gets to the true camera pose is a property of the scene and of the 3 deg / 50 mm
            # perturbed start -- ~100 mm here, in the oracle exactly as on the GPU -- and not a parity matter)
            for i in range(1, 4):
                assert np.abs(gT[i][:3, 3] - truth[i - 1][:3, 3]).max() < 200.0


@pytest.mark.parametrize("k,ratio,shards", [(20, 2.0, 4), (50, 0.3, 3), (200, 3.0, 8), (7, 1.0, 1)])
def test_sharded_sor_bit_identical_to_one_call(ops, oracle, base_cloud, k, ratio, shards):
    """kpx_sor_partial over `shards` slabs of the grid order + kpx_sor_finish == kpx_sor: keep list, statistics and mean
    distances bit-identical (same kernels, same reduction order), and equal to the oracle's keep list"""
    pts = torch.as_tensor(base_cloud[:: 3 if k < 100 else 8].copy()).cuda()
    n = pts.shape[0]
    keep, stats, avg = ops.sor(pts, k, ratio, want_avg=True)
    rows = -(-n // shards)
    parts, order = [], None
    for r in range(shards):
        part, order = ops.sor_partial(pts, k, min(n, r * rows), min(n, (r + 1) * rows))
        parts.append(part)
    keep2, stats2, avg2 = ops.sor_finish(torch.cat(parts), order, ratio, want_avg=True)
    assert torch.equal(keep, keep2) and torch.equal(stats, stats2) and torch.equal(avg, avg2)
    assert sorted(npy(order).tolist()) == list(range(n))
    ok, ostats, oavg = oracle.sor(npy(pts), k, ratio)
    assert np.array_equal(npy(keep2), ok) and np.allclose(npy(avg2), oavg, rtol=1e-12, atol=0)     # wave-order sums of sqrt: tolerance
    empty, _ = ops.sor_partial(pts, k, 5, 5)
    assert empty.numel() == 0


@pytest.mark.parametrize("world,mode,native", [(2, "sharded", 0), (4, "sharded", 0), (4, "rank0", 0), (2, "sharded", 1), (4, "sharded", 1), (4, "rank0", 1)])
def test_sensor_partition_equals_single_process_oracle(tmp_path, oracle, four_sensor_oracle, world, mode, native):
    """BASELINE configs[3] as the north star states it: sensor g on rank g (gloo ranks sharing the one GPU; world 2 = two
    sensors per rank), master-cloud broadcast, per-rank registration, all-gather, filter on the FUSED cloud -- every rank ends
    up with what the single-process oracle computes for the same four sensors: clouds identical, transforms within TOL_T;
    the same with two frames in flight (one communicator per slot).  native = 1: the host loop AND the collectives inside the library
    (kpx_frame_step_sharded through a host-staged gloo transport; collectives ordered by the library's kpx_order)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KPX_DIST_BACKEND="gloo", OUT_DIR=str(tmp_path), N_SENSORS="4", FUSED_FILTER=mode, NATIVE_LOOP=str(native))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                        "--master-port", str(29600 + world + (10 if mode == "rank0" else 0) + 20 * native), os.path.join(root, "tests", "dist_shard_worker.py")],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = four_sensor_oracle[5]
    for rank in range(world):
        z = np.load(str(tmp_path / f"rank{rank}.npz"))
        for key, f in [(f"{f}", f) for f in range(2)] + [(f"s{k}", k % 2) for k in range(4)]:
            pk, ck, tk = (f"p{key}", f"c{key}", f"T{key}") if not key.startswith("s") else (f"sp{key[1:]}", f"sc{key[1:]}", f"sT{key[1:]}")
            rp, rc, rT, _ = ref[f]
            assert np.abs(z[tk] - np.stack(rT)).max() < TOL_T
            if mode == "rank0" and rank != 0:
                assert pk not in z
                continue
            assert np.array_equal(z[pk], rp) and np.array_equal(z[ck], rc), (rank, key)


def _local_ranks(world, S, xy, depth, rgb, inits, mode, frames, slots=1, host=False, native_stream=False):
    """`world` in-process ranks (one thread each, all on this GPU) through the native sharded loop: -> per rank [(p, c, T, last)]"""
    import threading
    from kinectpy_amd import parallel
    from kinectpy_amd.pipeline import FrameStream, NativeFrameStream, NativeShardPipeline, PipelineParams
    hubs = [parallel.NativeComm.LocalHub(world) for _ in range(slots)]
    results, errors = [None] * world, []
    _local_ranks.retries = [0] * world

    def rank_main(r):
        try:
            torch.cuda.set_device(0)
            mine = parallel.shard_sensors(S, r, world)
            with torch.cuda.stream(torch.cuda.Stream()):
                pipes = [NativeShardPipeline(xy, S, inits, PipelineParams(), comm=parallel.NativeComm.local(h, r), fused_filter=mode) for h in hubs]
                feed = lambda f: ((torch.as_tensor(depth[f][mine]).pin_memory(), torch.as_tensor(rgb[f][mine]).pin_memory()) if host else
                                  (torch.as_tensor(depth[f][mine]).cuda(), torch.as_tensor(rgb[f][mine]).cuda()))
                out = []
                if slots == 1:
                    for f in frames:
                        p, c, Ts = pipes[0].step(*feed(f))
                        out.append((npy(p), npy(c), Ts, dict(pipes[0].last)))
                else:
                    fs = NativeFrameStream(pipes) if native_stream else FrameStream(pipes)
                    for f in frames:
                        if fs.full():
                            p, c, Ts = fs.pop()
                            out.append((npy(p), npy(c), Ts, {}))
                        fs.submit(*feed(f))
                    while fs.pending:
                        p, c, Ts = fs.pop()
                        out.append((npy(p), npy(c), Ts, {}))
                    fs.close()
                results[r] = out
                _local_ranks.retries[r] = sum(p_.retries for p_ in pipes)
        except BaseException as e:
            errors.append((r, e))
            for h in hubs:
                h.barrier.abort()

    ths = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    [t.start() for t in ths]
    [t.join(timeout=600) for t in ths]
    assert not errors, errors
    return results


@pytest.mark.parametrize("world,mode", [(1, "sharded"), (2, "sharded"), (3, "sharded"), (4, "sharded"), (4, "rank0")])
def test_native_sharded_loop_in_process_ranks(four_sensor_oracle, world, mode):
    """kpx_frame_step_sharded -- host loop and collectives in C++ -- with `world` in-process ranks on this GPU (device-to-device
    transport around a barrier): every rank ends with what the single-process oracle computes for the four sensors; the second
    frame runs with the message capacities learnt from the first, the third is handed over in pinned host memory"""
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    res = _local_ranks(world, 4, xy, depth, rgb, inits, mode, frames=(0, 1))
    res_h = _local_ranks(world, 4, xy, depth, rgb, inits, mode, frames=(1,), host=True)
    for r in range(world):
        for (p, c, Ts, last), f in list(zip(res[r], (0, 1))) + [(res_h[r][0], 1)]:
            rp, rc, rT, aux = ref[f]
            assert np.abs(Ts - np.stack(rT)).max() < TOL_T
            assert last["n_down"] == [len(x) for x in aux["downs"]] and last["n_fused"] == len(aux["fused"])
            assert [it for it, _, _ in last["icp"]] == [it for it, _, _ in aux["icp"]]
            if mode == "rank0" and r != 0:
                assert p.shape[0] == 0
                continue
            assert np.array_equal(p, rp) and np.array_equal(c, rc), (r, f)


def test_native_sharded_loop_through_the_native_stream(four_sensor_oracle):
    """kpx_stream with communicators (pipeline.NativeFrameStream over NativeShardPipelines): the rank's frames in flight scheduled by the
    library's worker threads, one communicator per slot, the collectives of the frames in flight in the order of the stream's own
    kpx_order (lookahead 2, round 5) -- 2 and 4 in-process ranks with three and four frames in flight: every frame on every rank equals
    the single-process oracle step."""
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    for world, slots in ((2, 3), (4, 4)):
        frames = (0, 1, 1, 0, 1, 0, 0)
        res = _local_ranks(world, 4, xy, depth, rgb, inits, "sharded", frames=frames, slots=slots, native_stream=True)
        for r in range(world):
            assert len(res[r]) == len(frames)
            for (p, c, Ts, _), f in zip(res[r], frames):
                rp, rc, rT, aux = ref[f]
                assert np.abs(Ts - np.stack(rT)).max() < TOL_T
                assert np.array_equal(p, rp) and np.array_equal(c, rc), (world, r, f)


def test_native_sharded_loop_round_robin_filter(four_sensor_oracle):
    """fused_filter 2 (round 5): frame f's fused transform + voxel + filter run on rank f mod world alone -- 4 in-process ranks, three
    frames in flight through the native stream: for every frame exactly one rank returns the oracle's frame, the others no rows, and
    every rank reports the same transforms."""
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    frames = (0, 1, 1, 0, 1, 0)
    res = _local_ranks(4, 4, xy, depth, rgb, inits, "round_robin", frames=frames, slots=3, native_stream=True)
    for j, f in enumerate(frames):
        rp, rc, rT, aux = ref[f]
        for r in range(4):
            p, c, Ts, _ = res[r][j]
            assert np.abs(Ts - np.stack(rT)).max() < TOL_T
            if r == j % 4:
                assert np.array_equal(p, rp) and np.array_equal(c, rc), (j, r)
            else:
                assert p.shape[0] == 0, (j, r)


def test_native_sharded_loop_eight_ranks_eight_sensors(oracle):
    """BASELINE configs[4]'s partition -- 8 sensors, one per rank, 8 ranks -- through the native loop (in-process ranks sharing this
    GPU): k_max = 1 headers, rank 0 owns only the master (no registration of its own), seven ranks register one sub each, the
    fused filter in eight slabs.  Every rank equals the oracle step over the eight sensors.  Then two frames in flight per rank
    (one communicator per slot, the library's kpx_order) on four ranks."""
    xy, depth, rgb, inits, truth, ref = _oracle_steps(oracle, 8, 1)
    rp, rc, rT, aux = ref[0]
    res = _local_ranks(8, 8, xy, depth, rgb, inits, "sharded", frames=(0, 0))
    for r in range(8):
        for p, c, Ts, last in res[r]:
            assert np.abs(Ts - np.stack(rT)).max() < TOL_T
            assert last["n_down"] == [len(x) for x in aux["downs"]] and last["n_fused"] == len(aux["fused"]) and last["n_voxel"] == len(aux["voxel"])
            assert np.array_equal(p, rp) and np.array_equal(c, rc), r
    res = _local_ranks(4, 8, xy, depth, rgb, inits, "sharded", frames=(0, 0, 0, 0, 0), slots=2)
    for r in range(4):
        assert len(res[r]) == 5
        for p, c, Ts, _ in res[r]:
            assert np.abs(Ts - np.stack(rT)).max() < TOL_T and np.array_equal(p, rp) and np.array_equal(c, rc), r


def test_native_sharded_loop_retries_a_frame_that_outgrows_its_messages(four_sensor_oracle):
    """message capacities follow the slot's previous frame (+25 %): a frame with an empty scene first (tiny capacities), then the
    real one -- every rank sees the overflow in the same header, returns KPX_RETRY and the frame runs again with room"""
    from kinectpy_amd import parallel
    from kinectpy_amd.pipeline import NativeShardPipeline, PipelineParams
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    comm = parallel.NativeComm.local(parallel.NativeComm.LocalHub(1), 0)
    pipe = NativeShardPipeline(xy, 4, inits, PipelineParams(), comm=comm)
    far = np.where(depth[0] > 0, np.uint16(60000), np.uint16(0)).astype(np.uint16)
    far[:, ::7] = 0                                    # a thin, far scene: few voxels in the registration grid, no person pixels kept
    try:
        pipe.step(torch.as_tensor(far).cuda(), torch.zeros_like(torch.as_tensor(rgb[0])).cuda())
    except Exception:
        pass                                           # (a degenerate registration may refuse; the capacities were learnt before)
    gp, gc, gT = pipe.step(torch.as_tensor(depth[0]).cuda(), torch.as_tensor(rgb[0]).cuda())
    assert pipe.retries >= 1
    assert np.array_equal(npy(gp), ref[0][0]) and np.array_equal(npy(gc), ref[0][1]) and np.abs(gT - np.stack(ref[0][2])).max() < TOL_T


def test_native_sharded_loop_retries_under_a_frame_stream(four_sensor_oracle):
    """the retry with frames in flight: two in-process ranks, two slots each; every slot first sees a thinned frame (one pixel in
    eight: small messages, small capacities), then the full one -- both ranks get KPX_RETRY for the same frames, FrameStream.pop()
    submits them again in program order (new frame numbers in the library's kpx_order) and every result equals the oracle step"""
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    thin = depth[0].copy()
    keep = (np.arange(thin.shape[1]) % 8) == 0
    thin[:, ~keep] = 0
    d2 = np.stack([thin, depth[0], depth[1]])
    c2 = np.stack([rgb[0], rgb[0], rgb[1]])
    res = _local_ranks(2, 4, xy, d2, c2, inits, "sharded", frames=(0, 0, 1, 2, 1, 2), slots=2)
    assert _local_ranks.retries[0] >= 2 and _local_ranks.retries[0] == _local_ranks.retries[1]       # both slots, the same frames on both ranks
    for r in range(2):
        assert len(res[r]) == 6
        for k, f in ((2, 0), (3, 1), (4, 0), (5, 1)):
            p, c, Ts, _ = res[r][k]
            assert np.array_equal(p, ref[f][0]) and np.array_equal(c, ref[f][1]) and np.abs(Ts - np.stack(ref[f][2])).max() < TOL_T, (r, k)


def test_native_sharded_loop_one_rank_failing_on_its_data_fails_every_rank(four_sensor_oracle):
    """an occluded camera on ONE rank (sensor 3: no valid pixel) -- a data-dependent error in front of the collectives: that rank keeps
    its place in them with a negative count in its header rows, so BOTH ranks return an error behind the same collective instead of
    one of them spinning in it; the communicators stay usable and the next (good) frame equals the oracle step.  Then the same for
    rank 0 (the master's camera occluded: the master header carries the failure)."""
    import threading
    from kinectpy_amd import parallel, _lib
    from kinectpy_amd.pipeline import NativeShardPipeline, PipelineParams
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    for bad_sensor, bad_rank in ((3, 1), (0, 0)):
        hub = parallel.NativeComm.LocalHub(2)
        got, errs = [None, None], [None, None]
        dbad = depth[0].copy()
        dbad[bad_sensor] = 0

        def rank_main(r):
            torch.cuda.set_device(0)
            mine = parallel.shard_sensors(4, r, 2)
            with torch.cuda.stream(torch.cuda.Stream()):
                pipe = NativeShardPipeline(xy, 4, inits, PipelineParams(), comm=parallel.NativeComm.local(hub, r))
                try:
                    pipe.step(torch.as_tensor(dbad[mine]).cuda(), torch.as_tensor(rgb[0][mine]).cuda())
                except _lib.KinectPxError as e:
                    errs[r] = str(e)
                p, c, Ts = pipe.step(torch.as_tensor(depth[0][mine]).cuda(), torch.as_tensor(rgb[0][mine]).cuda())
                got[r] = (npy(p), npy(c), Ts)

        ths = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
        [t.start() for t in ths]
        [t.join(timeout=120) for t in ths]
        stuck = any(t.is_alive() for t in ths)
        if stuck:
            hub.barrier.abort()
        assert not stuck, "a rank is still waiting inside a collective"
        assert errs[0] is not None and errs[1] is not None, errs
        assert "no valid pixel" in errs[bad_rank] and ("rank %d" % bad_rank in errs[1 - bad_rank] or "master" in errs[1 - bad_rank]), errs
        for r in range(2):
            assert np.array_equal(got[r][0], ref[0][0]) and np.array_equal(got[r][1], ref[0][1]) and np.abs(got[r][2] - np.stack(ref[0][2])).max() < TOL_T


def test_native_sharded_loop_through_rccl_one_rank(four_sensor_oracle):
    """the RCCL transport itself, as far as one GPU allows: a one-rank communicator built by kpx_comm_create_rccl (librccl dlopen'ed by
    the library, id from kpx_rccl_unique_id); broadcast, both all-gathers on the frame's stream from C++; two frames in flight on
    two communicators"""
    from kinectpy_amd import parallel
    from kinectpy_amd.pipeline import FrameStream, NativeShardPipeline, PipelineParams
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    d, c = torch.as_tensor(depth).cuda(), torch.as_tensor(rgb).cuda()
    comms = [parallel.NativeComm.rccl() for _ in range(2)]
    pipes = [NativeShardPipeline(xy, 4, inits, PipelineParams(), comm=cm) for cm in comms]
    for f in range(2):
        gp, gc, gT = pipes[0].step(d[f], c[f])
        assert np.array_equal(npy(gp), ref[f][0]) and np.array_equal(npy(gc), ref[f][1]) and np.abs(gT - np.stack(ref[f][2])).max() < TOL_T
    fs = FrameStream(pipes)
    got = []
    for k in range(5):
        if fs.full():
            got.append(fs.pop())
        fs.submit(d[k % 2], c[k % 2])
    while fs.pending:
        got.append(fs.pop())
    fs.close()
    for k, (gp, gc, gT) in enumerate(got):
        assert np.array_equal(npy(gp), ref[k % 2][0]) and np.array_equal(npy(gc), ref[k % 2][1])
    for cm in comms:
        cm.close()


@pytest.mark.parametrize("mode", ["p2p", "p2plane"])
def test_full_size_registration_config2(ops, oracle, base_cloud, engine, mode):
    """BASELINE configs[2]: 100k x 100k registration_icp, 30 iterations max (manual_pointcloud_registration.py:96-98 point to
    point; preprocessing/registration.py:78-84 point to plane) on both engines against the grid-accelerated oracle:
    iterations and fitness equal, T within TOL_T, and the correspondences of sampled iterations bit-exact"""
    src, tgt, T = synth.icp_pair(100_000, base_cloud)
    tn = oracle.estimate_normals(tgt, 70.0, 40)[0].astype(np.float32) if mode == "p2plane" else None
    g = ops.icp(src, tgt, 100.0, None, mode, tn, 30, want_corr=True)
    trace = []
    rT, rf, rr, rit = oracle.registration_icp(src, tgt, 100.0, None, mode, tn, 30, grid=True, trace=trace)
    assert g["iterations"] == rit and g["fitness"] == rf
    assert abs(g["inlier_rmse"] - rr) < 1e-9 * max(rr, 1)
    assert np.abs(g["transformation"] - rT).max() < TOL_T
    for Tk, idx, d2 in trace[:: max(1, len(trace) // 4)]:
        gi, gd = ops.nn_search(src, tgt, Tk)
        assert np.array_equal(npy(gi), idx) and np.array_equal(npy(gd), d2)
    # the last correspondence set the registration reports is the oracle's; a row whose nearest target lies beyond max_dist is
    # not a correspondence: the culled engine reports -1 there, the all-pairs engine the (unused) nearest index
    Tl, il, dl = trace[-1]
    gi = npy(g["idx"])
    within = dl < 100.0 * 100.0
    assert np.array_equal(gi[within], il[within]) and ((gi[~within] == -1) | (gi[~within] == il[~within])).all()


# ------------------------------------------------------------------ fused transform + stack + voxel grid (data.py:44-61)
def test_fuse_voxel_downsample_bit_exact(ops, oracle):
    """kpx_fuse_voxel_downsample against the oracle: 1 .. 5 clouds of ragged sizes (an empty one included), random rigid
    motions, voxel sizes from "every point alone" (the reference's 0.02 on mm data) to coarse; with identity transforms it
    equals voxel_down_sample of the stacked cloud; colours on all or none"""
    rng = np.random.default_rng(5)
    base = synth.frame_cloud()
    for case in range(10):
        cnt = int(rng.integers(1, 6))
        sizes = [int(rng.choice([0, 1, 7, 300, 5000, 40000])) for _ in range(cnt)]
        if sum(sizes) == 0:
            sizes[0] = 11
        clouds = [base[rng.choice(len(base), n, replace=False)] for n in sizes]
        cols = [rng.random((n, 3)).astype(np.float32) for n in sizes] if case % 3 else None
        Ts = []
        for c in range(cnt):
            T = synth.perturb(np.eye(4), deg=float(rng.uniform(0, 40)), mm=float(rng.uniform(0, 900)), seed=int(rng.integers(1 << 30)))
            Ts.append(np.eye(4) if c == 0 else T)
        voxel = float(rng.choice([0.02, 10.0, 35.0, 400.0]))
        gp, gc = ops.fuse_voxel_downsample(clouds, cols, Ts, voxel)
        rp, rc = oracle.fuse_voxel_downsample(clouds, cols, Ts, voxel)
        assert np.array_equal(npy(gp), rp), (case, sizes, voxel)
        assert (gc is None and rc is None) or np.array_equal(npy(gc), rc)
    clouds = [base[:30000], base[30000:50000]]
    gp, _ = ops.fuse_voxel_downsample(clouds, None, [np.eye(4)] * 2, 10.0)
    assert np.array_equal(npy(gp), npy(ops.voxel_downsample(base[:50000], 10.0)[0]))
    with pytest.raises(Exception):
        ops.fuse_voxel_downsample(clouds, None, [np.eye(4)] * 2, 0.0)


def test_fuse_voxel_downsample_upper_cloud_slots(ops, oracle):
    """9 and 16 clouds: slots 8 .. 15 of the 16-wide cloud set (the other fuse tests stop at 5 clouds).  Ragged sizes from
    {0, 1, 7, 300}, an empty cloud at a middle slot and one at slot 8, a random rigid motion per cloud, colours on all or
    none, a fine and a coarse voxel; a 17th cloud is refused"""
    rng = np.random.default_rng(16)
    base = synth.frame_cloud()
    for cnt in (9, 16):
        sizes = [int(rng.choice([0, 1, 7, 300])) for _ in range(cnt)]
        sizes[0], sizes[cnt // 2], sizes[8] = 300, 0, 0
        if cnt > 9:
            sizes[9], sizes[cnt - 1] = 7, 300                            # points behind the empty slot 8 and in the last slot
        clouds = [base[rng.choice(len(base), n, replace=False)] for n in sizes]
        Ts = [synth.perturb(np.eye(4), deg=float(rng.uniform(0, 40)), mm=float(rng.uniform(0, 900)), seed=int(rng.integers(1 << 30)))
              for _ in range(cnt)]
        for cols in (None, [rng.random((n, 3)).astype(np.float32) for n in sizes]):
            for voxel in (10.0, 400.0):
                gp, gc = ops.fuse_voxel_downsample(clouds, cols, Ts, voxel)
                rp, rc = oracle.fuse_voxel_downsample(clouds, cols, Ts, voxel)
                assert 0 < len(rp) <= sum(sizes)
                assert np.array_equal(npy(gp), rp), (cnt, sizes, voxel)
                assert (cols is None and gc is None and rc is None) or np.array_equal(npy(gc), rc), (cnt, sizes, voxel)
    with pytest.raises(Exception, match="1 .. 16 clouds"):
        ops.fuse_voxel_downsample([base[:7]] * 17, None, [np.eye(4)] * 17, 10.0)


def test_fused_voxel_membership_is_the_float64_path(ops, oracle):
    """what the fused pass is for: with float32 storage of the MOVED points a few points per 10^5 change voxel; the fused
    pass decides on the fp64 values, so its voxel count equals the oracle's float64-storage run (the reference's precision)"""
    base = synth.frame_cloud()
    clouds = [base[0::2][:90000], base[1::2][:90000]]
    T = synth.perturb(np.eye(4), deg=17.0, mm=400.0, seed=3)
    gp, _ = ops.fuse_voxel_downsample(clouds, None, [np.eye(4), T], 10.0)
    with oracle.storage("f64"):
        moved = np.concatenate([clouds[0].astype(np.float64), oracle.transform(clouds[1], T)])
        rp64, _, _, cnt64 = oracle.voxel_downsample(moved, 10.0, return_counts=True)
    assert len(gp) == len(rp64)
    assert np.abs(npy(gp).astype(np.float64) - rp64).max() < 3e-4          # the means differ by their float32 rounding only


# ------------------------------------------------------------------ the reference-shaped drivers (files in, files out)
def test_data_processor_reference_constructor(tmp_path, oracle):
    """DataProcessor(output_dirs, pb, pbtxt) as the reference runs it (preprocessing/data.py:15-69): directory walk in
    timestamp order, registration on frame 0 saved as transformation_master_sub_1.npy, per frame mask + gate + transform +
    fuse + filter_outliers, one .pcd per master timestamp -- against the oracle"""
    from kinectpy_amd.pcd_io import decode_pcd
    from kinectpy_amd.preprocessing.data import DataProcessor
    xy = synth.xy_table()
    Es = [synth.camera_pose(i, 8) for i in range(2)]
    stamps = [[900, 1000], [905, 1004]]                               # "900" sorts before "1000": numeric order, not text order
    frames = {}
    for d, E in enumerate(Es):
        deps = [synth.render_depth(E, seed=300 + 10 * d + f, xy=xy, return_person=True) for f in range(2)]
        xyzs = [oracle.unproject_u16(dep, xy) for dep, _ in deps]
        rgbs = [np.random.default_rng(40 + 10 * d + f).integers(1, 256, size=(len(xy), 3), dtype=np.uint8) for f in range(2)]
        frames[d] = (xyzs, rgbs, [p for _, p in deps])
        _write_device(str(tmp_path / ("master_1" if d == 0 else "sub_1")), stamps[d], xyzs, rgbs)
    dirs = [str(tmp_path / "master_1"), str(tmp_path / "sub_1")]
    init = synth.perturb(np.linalg.inv(Es[0]) @ Es[1], seed=1)
    masks = {}
    for d in range(2):
        for f in range(2):
            masks[frames[d][1][f].tobytes()[:64]] = frames[d][2][f]

    def mask_fn(img):                                                  # stand-in for Mask R-CNN: the renderer's person mask
        return masks[img.reshape(-1, 3).tobytes()[:64]].reshape(img.shape[:2])

    dp = DataProcessor(dirs, None, None, mask_fn=mask_fn, initial_transformations=[init])
    T = np.load(str(tmp_path / "master_1" / "transformation_master_sub_1.npy"))
    assert T.shape == (4, 4) and T.dtype == np.float64 and np.array_equal(T, dp.registration_transformations[0])
    full = [oracle.rgbd_compact(frames[d][0][0], frames[d][1][0])[0] for d in range(2)]
    downs = [oracle.voxel_downsample(c, 35.0)[0] for c in full]
    tn = oracle.estimate_normals(downs[0], 70.0, 40)[0].astype(np.float32)
    rT, _, _, _ = oracle.registration_icp(downs[1], downs[0], 100.0, init, "p2plane", tn, 30, grid=True)
    assert np.abs(T - rT).max() < TOL_T
    for f, ts in enumerate(stamps[0]):
        parts, cols = [], []
        for d in range(2):
            rgb = frames[d][1][f].copy()
            rgb[~frames[d][2][f]] = 0
            xyz = frames[d][0][f]
            p, c, _ = oracle.rgbd_compact(xyz, rgb, True, True, oracle.median_z(xyz) + 750.0)
            parts.append(p); cols.append(c)
        vp, vc = oracle.fuse_voxel_downsample(parts, cols, [np.eye(4), T], 0.02)
        keep, _, _ = oracle.sor(vp, 200, 3.0)
        with open(str(tmp_path / "master_1" / "filtered_and_registered_pointclouds" / f"{ts}.pcd"), "rb") as fh:
            pts, nrm, col = decode_pcd(fh.read())
        assert nrm is None and np.array_equal(pts, vp[keep].astype(np.float64))
        assert np.array_equal(col, np.round(vc[keep].astype(np.float64) * 255.0) / 255.0)


def test_manual_registration_from_picked_points(ops, oracle, base_cloud):
    """manual_pointcloud_registration.py:84-98: Umeyama from picked pairs, then point-to-point ICP (the reference's literal
    threshold 0.03 is metre-thinking on mm data: the test passes the mm equivalent as well)"""
    from kinectpy_amd.geometry import PointCloud
    from kinectpy_amd.manual_pointcloud_registration import manual_registration
    src, tgt, T = synth.icp_pair(20000, base_cloud)
    rng = np.random.default_rng(9)
    ps = rng.choice(len(src), 6, replace=False)
    s64 = src[ps].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    pt = np.array([int(np.argmin(((tgt.astype(np.float64) - q) ** 2).sum(1))) for q in s64])
    for thr in (0.03, 30.0):
        got = manual_registration(PointCloud(tgt), PointCloud(src), ps, pt, threshold=thr)
        init = oracle.kabsch(src[ps], tgt[pt])
        want, _, _, _ = oracle.registration_icp(src, tgt, thr, init, "p2p", None, 30, grid=True)
        assert np.abs(got - want).max() < 1e-7
    assert np.abs(got[:3, 3] - T[:3, 3]).max() < 5.0
    with pytest.raises(NotImplementedError):
        manual_registration(PointCloud(tgt), PointCloud(src))


def test_native_frame_step_equals_python_pipeline_and_oracle(four_sensor_oracle):
    """kpx_frame_step (the frame loop in C++ inside the library) against the Python pipeline (bit-identical: same entry points
    in the same order) and against the oracle step, serially and with three frames in flight"""
    from kinectpy_amd.pipeline import FrameStream, NativeFramePipeline, PipelineParams, SensorShardPipeline
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    d, c = torch.as_tensor(depth).cuda(), torch.as_tensor(rgb).cuda()
    nat, py = NativeFramePipeline(xy, 4, inits, PipelineParams()), SensorShardPipeline(xy, 4, inits, PipelineParams())
    for f in range(2):
        gp, gc, gT = nat.step(d[f], c[f])
        pp, pc, pT = py.step(d[f], c[f])
        # same clouds; the transforms agree to the last bits only: the native loop hands the registration clouds over in Z-curve
        # order (no Morton sort inside the ICP), so a block's 64 rows -- whose fp64 partial sums feed the exact accumulators -- are
        # other rows than in the Python pipeline
        assert torch.equal(gp, pp) and torch.equal(gc, pc) and np.abs(gT - pT).max() < 1e-11
        assert nat.last["n_down"] == py.last["n_down"] and nat.last["n_voxel"] == py.last["n_voxel"]
        assert [s[0] for s in nat.last["icp"]] == [s[0] for s in py.last["icp"]]
        rp, rc, rT, _ = ref[f]
        assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc) and np.abs(gT - np.stack(rT)).max() < TOL_T
    fs = FrameStream(nat, 3)
    got = []
    for k in range(7):
        if fs.full():
            got.append(fs.pop())
        fs.submit(d[k % 2], c[k % 2])
    while fs.pending:
        got.append(fs.pop())
    fs.close()
    for k, (gp, gc, gT) in enumerate(got):
        assert np.array_equal(npy(gp), ref[k % 2][0]) and np.array_equal(npy(gc), ref[k % 2][1])
    one = NativeFramePipeline(xy, 1, [], PipelineParams())
    gp, gc, gT = one.step(d[0][:1], c[0][:1])
    assert gT.shape == (1, 4, 4) and np.array_equal(gT[0], np.eye(4)) and gp.shape[0] > 1000
    # the frame loop speculates the voxel sort's key width from the thread's previous frame: a frame that suddenly needs MORE bits
    # (a 7x finer registration grid here: 24 -> 33 bits) must be caught and redone, one that needs fewer just sorts zero bits
    for voxel in (5.0, 35.0, 70.0, 35.0):
        prm = PipelineParams(reg_voxel=voxel)
        gp, gc, gT = NativeFramePipeline(xy, 4, inits, prm).step(d[0], c[0])
        pp, pc, pT = SensorShardPipeline(xy, 4, inits, prm).step(d[0], c[0])
        assert torch.equal(gp, pp) and torch.equal(gc, pc) and np.abs(gT - pT).max() < 1e-11, voxel


def test_sor_and_normals_with_thousands_of_duplicates(ops, oracle, base_cloud):
    """exact duplicates all land in one grid cell whatever its size (the counting grid build ranks a point against its whole
    cell): 6000 copies of one point + 3000 of another inside an ordinary cloud -- keep list equal to the oracle's, normals finite"""
    pts = base_cloud[::12][:20000].copy()
    pts[:6000] = pts[0]
    pts[6000:9000] = pts[7000]
    rng = np.random.default_rng(3)
    pts = pts[rng.permutation(len(pts))]
    keep, stats, _ = ops.sor(pts, 20, 2.0)
    ok, ostats, _ = oracle.sor(pts, 20, 2.0)
    assert np.array_equal(npy(keep), ok)
    assert np.allclose(npy(stats), np.array(ostats), rtol=TOL_STATS)
    nrm = npy(ops.estimate_normals(pts, 70.0, 40))
    assert np.isfinite(nrm).all() and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)


_ICP_UPDATE_MODES = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, os.getcwd())
from kinectpy_amd import ops
from kinectpy_amd.pipeline import PipelineParams
from kinectpy_amd.utils import synth
P = PipelineParams()
xy, depth, rgb, inits, _ = synth.sensor_ring(4, 1)
d = torch.as_tensor(depth[0]).cuda()
fp, _, _, cnt = ops.depth_to_cloud(d, xy, None, 4, False, False, sync=False)
k = ops._count(cnt)
downs = [x[0] for x in ops.voxel_downsample_batch([fp[i, :k[i]] for i in range(4)], P.reg_voxel)]
tn = ops.estimate_normals(downs[0], 2.0 * P.reg_voxel, P.normals_nn)
out = {}
for mode in ("p2plane", "p2p"):
    r = ops.icp_batch(downs[1:], downs[0], P.icp_max_dist, inits, mode, tn, P.icp_max_iteration)
    out[mode + "_T"] = np.stack([x["transformation"] for x in r])
    out[mode + "_s"] = np.array([[x["fitness"], x["inlier_rmse"], x["iterations"], x["count"]] for x in r])
    # a batch small enough for the one-launch chain (its blocks must all be resident: <= 512), ragged sizes, and one registration alone
    for tag, srcs, ini in (("small", [downs[1][:9000], downs[2][:7001], downs[3][:12000]], inits), ("alone", [downs[3][:20001]], inits[2:3])):
        r = ops.icp_batch(srcs, downs[0], P.icp_max_dist, ini, mode, tn, P.icp_max_iteration)
        out[mode + "_" + tag + "_T"] = np.stack([x["transformation"] for x in r])
        out[mode + "_" + tag + "_s"] = np.array([[x["fitness"], x["inlier_rmse"], x["iterations"], x["count"]] for x in r])
out["chains"] = np.array([ops.icp_chain(-2)])
np.savez(sys.argv[1], **out)
"""


def test_icp_update_placements_and_light_skip_are_bit_identical(tmp_path):
    """The update step in the last block of the sweep (the grouped driver, the default), in the next sweep's prologue
    (KPX_ICP_BATCH_LAUNCH=0: per-registration chains) and in its own kernel behind the kernel boundary (KPX_ICP_BATCH_LAUNCH=0
    KPX_ICP_FUSE=0), and with the blocks that provably cannot find a partner left out of the sweeps (KPX_ICP_LIGHT_SKIP, default on)
    and the rows whose partner provably
    cannot change left out of the search (KPX_ICP_CERT, default on), and the whole chain in one launch (icp_chain_kernel, the default
    where a batch's blocks fit the device: the "small" and "alone" batches) against a launch per iteration (KPX_ICP_CHAIN=0): the
    exact fixed-point sums do not depend on which blocks add to them or when, and a certified row keeps exactly the partner a search
    would return, so transforms, fitness, rmse, iterations and counts agree to the last bit.  Round 5: the default iteration kernel is
    icp_rows_kernel (a wave per 64 rows) once most rows carry a certificate and icp_iter_batch_kernel (a wave per 16-row tile, blocks
    of four) before, chosen per launch from the progress words (KPX_ICP_ROWS=0: never, 2: always, KPX_ICP_ROWS_SHARE: the threshold) --
    the sums' contract (a tree per tile, tiles added exactly) makes the forms agree bit for bit as well."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for name, env in (("tail+skip", {}), ("nocert", {"KPX_ICP_CERT": "0"}), ("tail", {"KPX_ICP_LIGHT_SKIP": "0"}),
                      ("kernel", {"KPX_ICP_BATCH_LAUNCH": "0", "KPX_ICP_FUSE": "0"}), ("prologue", {"KPX_ICP_BATCH_LAUNCH": "0"}),
                      ("launches", {"KPX_ICP_CHAIN": "0"}), ("chain nocert", {"KPX_ICP_CERT": "0", "KPX_ICP_CHAIN": "1"}),
                      ("blocks of four", {"KPX_ICP_ROWS": "0"}), ("blocks of four nocert", {"KPX_ICP_ROWS": "0", "KPX_ICP_CERT": "0", "KPX_ICP_CHAIN": "0"}),
                      ("rows", {"KPX_ICP_ROWS": "2", "KPX_ICP_CHAIN": "0"}), ("rows nocert", {"KPX_ICP_ROWS": "2", "KPX_ICP_CERT": "0", "KPX_ICP_CHAIN": "0"}),
                      ("rows early", {"KPX_ICP_ROWS_SHARE": "100", "KPX_ICP_CHAIN": "0"})):
        f = str(tmp_path / (name.replace("+", "_").replace(" ", "_") + ".npz"))
        r = subprocess.run([sys.executable, "-c", _ICP_UPDATE_MODES, f], cwd=root, capture_output=True, text=True, timeout=300,
                           env={**os.environ, "KPX_ICP_CHAIN_LOCK": "0", **env})    # (this process may hold the device's chain lock; it is idle meanwhile)
        assert r.returncode == 0, r.stderr[-2000:]
        got[name] = dict(np.load(f))
    # the forms that were to be compared did run: four chains (two modes x two small batches) by default, none with KPX_ICP_CHAIN=0 or per-registration chains
    assert got["tail+skip"]["chains"][0] == 4 and got["chain nocert"]["chains"][0] == 4 and got["launches"]["chains"][0] == 0
    assert got["kernel"]["chains"][0] == 0 and got["prologue"]["chains"][0] == 0
    for name in ("nocert", "tail", "kernel", "prologue", "launches", "chain nocert", "blocks of four", "blocks of four nocert", "rows", "rows nocert", "rows early"):
        for key, v in got["tail+skip"].items():
            if key != "chains":
                assert np.array_equal(v, got[name][key]), (name, key)
    its = got["tail+skip"]["p2plane_s"][:, 2]
    assert its.max() >= 10, its                                        # a chain long enough for blocks to be skipped


def test_icp_chain_edge_sizes_equal_launch_per_iteration(ops, base_cloud):
    """the one-launch chain (kpx_icp_chain(1)) against a launch per iteration (0) in ONE process, at the edges: sources of 1, 17, 64 and
    65 rows (partial waves, partial blocks, a block boundary), seven registrations in one group (with the target: all the batch sort takes), max_iteration 0, 1, 62 (the last the
    chain's records hold) and 63 (one more: must fall back by itself), both estimation modes -- every output bit for bit"""
    if ops.icp_chain(-1) == 0:
        pytest.skip("KPX_ICP_CHAIN=0")
    src, tgt, T = synth.icp_pair(4000, base_cloud)
    tn = ops.estimate_normals(torch.as_tensor(tgt).cuda(), 70.0, 40)
    cases = [([src[:1]], 5), ([src[:17], src[:64], src[:65]], 5), ([src[i * 300:(i + 1) * 300 + 7 * i] for i in range(7)], 6),
             ([src[:2000]], 0), ([src[:2000]], 1), ([src[:1500], src[1500:2600]], 62), ([src[:1500]], 63)]
    before = ops.icp_chain(-2)
    try:
        for srcs, iters in cases:
            for mode, nrm in (("p2p", None), ("p2plane", tn)):
                inits = [np.eye(4)] * len(srcs)
                got = {}
                for form in (1, 0):
                    ops.icp_chain(form)
                    got[form] = ops.icp_batch(srcs, tgt, 100.0, inits, mode, nrm, iters)
                for a, b in zip(got[1], got[0]):
                    assert a["iterations"] == b["iterations"] and a["fitness"] == b["fitness"] and a["inlier_rmse"] == b["inlier_rmse"], (len(srcs), iters, mode)
                    assert np.array_equal(a["transformation"], b["transformation"]), (len(srcs), iters, mode)
    finally:
        ops.icp_chain(1)
    # the chain form ran for every case but max_iteration 63 (two modes each); with another process holding the card's chain lock nothing is compared
    ran = ops.icp_chain(-2) - before
    assert ran in (0, 12), ran


def test_icp_chain_fuzz_against_launches_and_oracle():
    """tools/fuzz_icp_chain.py: 40 random batches (1-7 registrations of 1-3000 rows, both modes, 0-40 iterations, three correspondence
    distances, random initial transforms) through the one-launch chain and through a launch per iteration -- bit-identical -- and every
    fifth against the CPU oracle where the update is well posed"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_icp_chain.py"), "40", "3"], cwd=root, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "KPX_ICP_CHAIN_LOCK": "0"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-1000:])
    assert "chains launched 40 mismatches 0" in r.stdout, r.stdout[-500:]


_ICP_CHAIN_ABORT = r"""
import os, sys, json, numpy as np, torch
sys.path.insert(0, os.getcwd())
from kinectpy_amd import ops
from kinectpy_amd.pipeline import PipelineParams
from kinectpy_amd.utils import synth
P = PipelineParams()
xy, depth, rgb, inits, _ = synth.sensor_ring(4, 1)
d = torch.as_tensor(depth[0]).cuda()
fp, _, _, cnt = ops.depth_to_cloud(d, xy, None, 4, False, False, sync=False)
k = ops._count(cnt)
downs = [x[0] for x in ops.voxel_downsample_batch([fp[i, :k[i]] for i in range(4)], P.reg_voxel)]
tn = ops.estimate_normals(downs[0], 2.0 * P.reg_voxel, P.normals_nn)
big = torch.cat(downs[1:])                            # ONE registration of ~94k rows: ~1470 blocks (several problems of a batch could
                                                      # still drain one after the other; one problem larger than the device cannot)
err, first = "", None
try:
    r = ops.icp_batch([big], downs[0], P.icp_max_dist, inits[:1], "p2plane", tn, 8)
    first = float(r[0]["fitness"])
except Exception as e:                                  # noqa: BLE001 -- the abort is THIS call's error
    err = str(e)
small = ops.icp_batch(downs[1:2], downs[0], P.icp_max_dist, inits[:1], "p2plane", tn, 8)      # an unrelated, healthy call right behind it: no error of its own
ops.icp_chain(0)
again = ops.icp_batch([big], downs[0], P.icp_max_dist, inits[:1], "p2plane", tn, 8)
print(json.dumps(dict(first=first, err=err, chains=ops.icp_chain(-2), small=float(small[0]["fitness"]), again=float(again[0]["fitness"]), iterations=int(again[0]["iterations"]),
                      blocks=int((big.shape[0] + 63) // 64))))
"""


def test_icp_chain_that_cannot_be_resident_fails_loudly():
    """The one-launch chain needs all its blocks resident; the host only admits chains that fit (chain_launch_if_fits).  Forced past
    that check (KPX_ICP_CHAIN_BUDGET far above what the device holds, a short KPX_ICP_CHAIN_WAIT_SECONDS), a chain whose blocks cannot
    all be resident must END -- every block's wait is bounded -- poison its results, and THAT call fails with a message that names the
    cause (round 5: per call, not at the next call); a healthy call right behind it and the launch-per-iteration form work in the same process."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _ICP_CHAIN_ABORT], cwd=root, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "KPX_ICP_CHAIN_LOCK": "0", "KPX_ICP_CHAIN_BUDGET": "1000000", "KPX_ICP_CHAIN_WAIT_SECONDS": "0.05"})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["blocks"] > 1024, out["blocks"]                          # more blocks than an MI355X holds at 3 per CU: the chain cannot be resident
    assert out["chains"] >= 1 and out["first"] is None, out
    assert "gave up waiting" in out["err"], out                          # reported by the call whose chain aborted, not by a later one
    assert 0.0 < out["small"] <= 1.0, out
    assert 0.0 < out["again"] <= 1.0 and out["iterations"] >= 1, out


_ICP_CERT_CHECK = r"""
import os, sys, json, numpy as np, torch
sys.path.insert(0, os.getcwd())
from kinectpy_amd import ops
from kinectpy_amd.pipeline import PipelineParams
from kinectpy_amd.utils import synth
P = PipelineParams()
xy, depth, rgb, inits, _ = synth.sensor_ring(4, 1)
d = torch.as_tensor(depth[0]).cuda()
fp, _, _, cnt = ops.depth_to_cloud(d, xy, None, 4, False, False, sync=False)
k = ops._count(cnt)
downs = [x[0] for x in ops.voxel_downsample_batch([fp[i, :k[i]] for i in range(4)], P.reg_voxel)]
tn = ops.estimate_normals(downs[0], 2.0 * P.reg_voxel, P.normals_nn)
ops.prof_icp_cert()
out = []
for mode in ("p2plane", "p2p"):
    for md in (P.icp_max_dist, 40.0):
        r = ops.icp_batch(downs[1:], downs[0], md, inits, mode, tn, P.icp_max_iteration)
        torch.cuda.synchronize()
        c = ops.prof_icp_cert()
        out.append(dict(mode=mode, max_dist=md, iterations=[x["iterations"] for x in r], certified=c["certified"], searched=c["searched"], mismatches=c["mismatches"]))
print(json.dumps(out))
"""


def test_icp_certificates_never_contradict_the_search():
    """KPX_ICP_CERT_CHECK=1: the rows a certificate would leave out of the correspondence search are searched all the same, and the
    search's winner is compared with the partner the certificate kept (kpx_prof_icp_cert): no disagreement in any iteration of the
    bench's registrations, both estimation modes, two correspondence distances -- and the certificates do cover most of the late
    iterations (otherwise the check checks nothing)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _ICP_CERT_CHECK], cwd=root, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "KPX_ICP_CERT_CHECK": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout.strip().splitlines()[-1])
    for row in rows:
        assert row["mismatches"] == 0, row
    plane = rows[0]
    assert max(plane["iterations"]) >= 10 and plane["certified"] > plane["searched"], plane


def test_update_placements_agree_with_four_frames_in_flight(tmp_path):
    """The same comparison under load: 24 frames through FrameStream with FOUR frames in flight (every kernel of four ICP chains
    sharing the device), update step in the last block of the sweep (default; its hand-off rests on returning device-scope atomics,
    a relaxed ticket and sc1 loads in the winning block -- the `sc1` form of the guide's valid hand-offs), in its own kernel behind the
    kernel boundary (KPX_ICP_BATCH_LAUNCH=0 KPX_ICP_FUSE=0: per-registration chains), and in the next sweep's prologue
    (KPX_ICP_BATCH_LAUNCH=0); the default again with the blocks-of-four and the rows kernel forced: every fused cloud and every
    transform identical to the last bit, and the repeats of a frame identical
    among themselves."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    envs = {"2": {}, "1": {"KPX_ICP_BATCH_LAUNCH": "0", "KPX_ICP_FUSE": "0"}, "0": {"KPX_ICP_BATCH_LAUNCH": "0"},
            "blocks": {"KPX_ICP_ROWS": "0"}, "rows": {"KPX_ICP_ROWS": "2"}}
    for mode, env in envs.items():
        f = str(tmp_path / f"split{mode}.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "ab_frames.py"), f, "4", "3"], cwd=root, capture_output=True, text=True,
                           timeout=600, env={**os.environ, **env, "GPU_MAX_HW_QUEUES": "8"})
        assert r.returncode == 0, r.stderr[-2000:]
        got[mode] = dict(np.load(f))
    for mode in ("1", "0", "blocks", "rows"):
        for key, v in got["2"].items():
            assert np.array_equal(v, got[mode][key]), (mode, key)
    for k in range(8):
        for rep in (1, 2):
            assert np.array_equal(got["2"][f"p{k}"], got["2"][f"p{k + 8 * rep}"]) and np.array_equal(got["2"][f"T{k}"], got["2"][f"T{k + 8 * rep}"])


@pytest.mark.parametrize("n,end_bit", [(1, 32), (63, 8), (2048, 9), (2049, 24), (100_003, 27), (1_130_000, 24), (1_130_000, 32), (300_000, 1),
                                       (4_194_304, 17), (4_200_000, 22), (65536, 22), (65537, 22), (4_194_305, 9), (1000, 33)])
def test_radix_sort_pairs_is_the_stable_sort(ops, n, end_bit):
    """kpx_sort_pairs_u32 (the library's own LSD radix sort up to 4M pairs, rocPRIM above) against numpy's stable argsort of the
    masked keys: keys AND values identical, i.e. equal keys keep their input order; few distinct keys, full-range keys, a
    partial last tile, all keys equal.  65536 / 65537: the own sort's first group-row boundary and the grid build's switch;
    4_194_305 at 9 bits: the vendor sort one pair past the own sort's limit, run below the 32 bits its temporary size was asked for;
    33 bits: more than the key has, refused."""
    from kinectpy_amd._lib import KinectPxError
    rng = np.random.default_rng(n + end_bit)
    if end_bit > 32:
        with pytest.raises(KinectPxError):
            ops.sort_pairs_u32(torch.zeros(n, dtype=torch.int32).cuda().view(torch.uint32), torch.arange(n, dtype=torch.int32).cuda(), end_bit)
        return
    mask = np.uint32((1 << end_bit) - 1) if end_bit < 32 else np.uint32(0xFFFFFFFF)
    for kind in ("random", "few", "equal"):
        if kind == "random":
            keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        elif kind == "few":
            keys = (rng.integers(0, 37, n, dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        else:
            keys = np.full(n, 0xDEADBEEF, dtype=np.uint32)
        vals = np.arange(n, dtype=np.int32)[::-1].copy()
        ko, vo = ops.sort_pairs_u32(torch.from_numpy(keys.view(np.int32)).cuda().view(torch.uint32), torch.from_numpy(vals).cuda(), end_bit)
        order = np.argsort(keys & mask, kind="stable")
        assert np.array_equal(npy(ko.view(torch.int32)).view(np.uint32), keys[order]), (kind, "keys")
        assert np.array_equal(npy(vo), vals[order]), (kind, "values")


def test_sor_select_equals_filter_then_selection(ops):
    """kpx_sor_select = kpx_sor + kpx_select_by_index: the same keep list, statistics and rows (points and one attribute array),
    also for an empty cloud and without attributes"""
    pts = torch.as_tensor(synth.filter_cloud(60_000)).cuda()
    col = torch.rand_like(pts)
    idx, stats, _ = ops.sor(pts, 20, 2.0)
    p, c, i2, st2 = ops.sor_select(pts, col, 20, 2.0)
    assert torch.equal(idx, i2) and torch.equal(stats, st2)
    assert torch.equal(p, pts[idx.long()]) and torch.equal(c, col[idx.long()])
    p3, c3, i3, _ = ops.sor_select(pts, None, 20, 2.0)
    assert c3 is None and torch.equal(p3, p) and torch.equal(i3, idx)
    pe, ce, ie, _ = ops.sor_select(torch.zeros((0, 3)), None, 20, 2.0)
    assert pe.shape[0] == 0 and ie.shape[0] == 0


def test_native_frame_step_from_pinned_host_memory(four_sensor_oracle):
    """SURVEY 8(d)'s interval: frames handed over in pinned host memory (kpx_frame_step_host stages them through the workspace
    on the frame's stream) -- same clouds as the oracle step, serially, with four frames in flight and with the output ring"""
    from kinectpy_amd.pipeline import FrameStream, NativeFramePipeline, PipelineParams
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    dh, ch = torch.as_tensor(depth).pin_memory(), torch.as_tensor(rgb).pin_memory()
    nat = NativeFramePipeline(xy, 4, inits, PipelineParams())
    for f in range(2):
        gp, gc, gT = nat.step(dh[f], ch[f])
        assert np.array_equal(npy(gp), ref[f][0]) and np.array_equal(npy(gc), ref[f][1]) and np.abs(gT - np.stack(ref[f][2])).max() < TOL_T
    gp, gc, gT = nat.step(torch.as_tensor(depth[1]), torch.as_tensor(rgb[1]))            # pageable host memory works too (synchronous copy)
    assert np.array_equal(npy(gp), ref[1][0])
    pipes = [NativeFramePipeline(xy, 4, inits, PipelineParams(), out_ring=2) for _ in range(4)]
    fs = FrameStream(pipes, 4)
    got = []
    for k in range(11):
        if fs.full():
            got.append([npy(t) if isinstance(t, torch.Tensor) else t for t in fs.pop()])      # copied out before the ring wraps
        fs.submit(dh[k % 2], ch[k % 2]) if k % 3 else fs.submit(torch.as_tensor(depth[k % 2]).cuda(), torch.as_tensor(rgb[k % 2]).cuda())
    while fs.pending:
        got.append([npy(t) if isinstance(t, torch.Tensor) else t for t in fs.pop()])
    fs.close()
    assert len(got) == 11
    for k, (gp, gc, gT) in enumerate(got):
        assert np.array_equal(gp, ref[k % 2][0]) and np.array_equal(gc, ref[k % 2][1]), k
    with pytest.raises(ValueError):
        nat.step(torch.as_tensor(depth[0].astype(np.int32)), torch.as_tensor(rgb[0]))


def test_native_frame_stream_equals_serial_steps_and_oracle(four_sensor_oracle):
    """kpx_stream (pipeline.NativeFrameStream: the frames in flight scheduled by C++ worker threads inside the library): 14 frames with
    four in flight, from device memory and from pinned host memory in turn, come back in submission order and equal the serial native
    step bit for bit (clouds, colours, transforms) and the oracle step (clouds identical, transforms within TOL_T); submit beyond the
    depth is refused; an error inside a frame surfaces in pop() with its message, and the stream goes on."""
    from kinectpy_amd.pipeline import NativeFramePipeline, NativeFrameStream, PipelineParams
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    dh, ch = torch.as_tensor(depth).pin_memory(), torch.as_tensor(rgb).pin_memory()
    dd, cd = torch.as_tensor(depth).cuda(), torch.as_tensor(rgb).cuda()
    nat = NativeFramePipeline(xy, 4, inits, PipelineParams())
    serial = []
    for f in range(2):
        gp, gc, gT = nat.step(dd[f], cd[f])
        serial.append((npy(gp), npy(gc), gT.copy()))
        assert np.array_equal(serial[f][0], ref[f][0]) and np.array_equal(serial[f][1], ref[f][1]) and np.abs(gT - np.stack(ref[f][2])).max() < TOL_T
    fs = NativeFrameStream(nat, 4)
    got = []
    for k in range(14):
        if fs.full():
            with pytest.raises(AssertionError):
                fs.submit(dd[0], cd[0])
            got.append([npy(t) if isinstance(t, torch.Tensor) else t.copy() for t in fs.pop()])
        fs.submit(dh[k % 2], ch[k % 2]) if k % 3 == 1 else fs.submit(dd[k % 2], cd[k % 2])
    while fs.pending:
        got.append([npy(t) if isinstance(t, torch.Tensor) else t.copy() for t in fs.pop()])
    assert len(got) == 14 and fs.last["n_out"] == got[-1][0].shape[0]
    for k, (gp, gc, gT) in enumerate(got):
        assert np.array_equal(gp, serial[k % 2][0]) and np.array_equal(gc, serial[k % 2][1]) and np.array_equal(gT, serial[k % 2][2]), k
    # a frame that fails (a voxel size far too small for the cloud's extent) reports in ITS pop; the frames around it are unaffected
    bad = NativeFramePipeline(xy, 4, inits, PipelineParams(filt_voxel=1e-6))
    fb = NativeFrameStream(bad, 2)
    fb.submit(dd[0], cd[0])
    with pytest.raises(Exception) as ei:
        fb.pop()
    assert "voxel_size is too small" in str(ei.value)
    fb.close()
    fs.submit(dd[1], cd[1])
    gp, gc, gT = fs.pop()
    assert np.array_equal(npy(gp), serial[1][0])
    fs.close()


def test_frame_step_with_fixed_transforms_equals_oracle(oracle, four_sensor_oracle):
    """KPX_ICP_FIXED (PipelineParams(icp_mode="fixed")): the reference's loop after its first frame (preprocessing/data.py:35-61 registers
    `if i == 0` and reuses the transforms): extract (mask + gate + colours) -> transform + vstack + voxel -> remove_statistical_outlier with
    GIVEN transforms.  The native step, the same step from pinned host memory, four frames in flight through kpx_stream and the Python
    operators all equal the oracle's pieces bit for bit, at the bench's filter (20, 2.0) and at filter_outliers' defaults (200, 3.0)."""
    from kinectpy_amd.pipeline import NativeFramePipeline, NativeFrameStream, PipelineParams, SensorGroupPipeline
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    dd, cd = torch.as_tensor(depth).cuda(), torch.as_tensor(rgb).cuda()
    dh, ch = torch.as_tensor(depth).pin_memory(), torch.as_tensor(rgb).pin_memory()
    Ts = [np.asarray(T, dtype=np.float64) for T in ref[0][2][1:]]               # the registered transforms of frame 0
    for k, ratio in ((20, 2.0), (200, 3.0)):
        P = PipelineParams(icp_mode="fixed", filt_k=k, filt_ratio=ratio)
        want = []
        for f in range(2):
            clouds, cols = [], []
            for i in range(4):
                r = oracle.unproject_u16(depth[f][i], xy)
                p_, c_, _ = oracle.rgbd_compact(r, rgb[f][i], True, True, oracle.median_z(r) + P.gate)
                clouds.append(p_); cols.append(c_)
            vp, vc = oracle.fuse_voxel_downsample(clouds, cols, [np.eye(4)] + Ts, P.filt_voxel)
            keep = oracle.sor(vp, k, ratio)[0]
            want.append((vp[keep], vc[keep]))
        nat = NativeFramePipeline(xy, 4, Ts, P)
        py = SensorGroupPipeline(xy, Ts, P)
        for f in range(2):
            for step, a, b in ((nat.step, dd[f], cd[f]), (nat.step, dh[f], ch[f]), (py.step, dd[f], cd[f])):
                gp, gc, gT = step(a, b)
                assert np.array_equal(npy(gp), want[f][0]) and np.array_equal(npy(gc), want[f][1]), (k, f)
                assert np.array_equal(np.asarray(gT)[1:], np.stack(Ts)) and np.array_equal(np.asarray(gT)[0], np.eye(4))
        fs = NativeFrameStream(nat, 4)
        got = []
        for j in range(10):
            if fs.full():
                got.append([npy(t) if isinstance(t, torch.Tensor) else t.copy() for t in fs.pop()])
            fs.submit(dh[j % 2], ch[j % 2]) if j % 3 == 1 else fs.submit(dd[j % 2], cd[j % 2])
        while fs.pending:
            got.append([npy(t) if isinstance(t, torch.Tensor) else t.copy() for t in fs.pop()])
        fs.close()
        assert len(got) == 10
        for j, (gp, gc, gT) in enumerate(got):
            assert np.array_equal(gp, want[j % 2][0]) and np.array_equal(gc, want[j % 2][1]), (k, j)


def test_native_frame_step_ten_sensors_equals_oracle(oracle):
    """ten sensors: nine registrations = two launch chains side by side on the library's lanes (each with its own update-in-the-
    last-block tickets and skip keys), the voxel batch in two groups (row-major clouds: the ICP batch sorts them itself)"""
    from kinectpy_amd.pipeline import NativeFramePipeline, PipelineParams
    xy, depth, rgb, inits, truth, ref = _oracle_steps(oracle, 10, 1)
    nat = NativeFramePipeline(xy, 10, inits, PipelineParams())
    gp, gc, gT = nat.step(torch.as_tensor(depth[0]).cuda(), torch.as_tensor(rgb[0]).cuda())
    rp, rc, rT, aux = ref[0]
    assert np.abs(gT - np.stack(rT)).max() < TOL_T
    assert [s[0] for s in nat.last["icp"]] == [it for it, _, _ in aux["icp"]]
    assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc)


def test_native_frame_step_eight_sensors_equals_oracle(oracle):
    """BASELINE configs[4]'s rig on one GPU through kpx_frame_step: seven registrations in one launch chain (the batch limit), three
    cloud bits in the Z-curve voxel keys, 2.2M pairs in the library's radix sort -- fused cloud and colours identical to the oracle
    step, transforms within TOL_T, iteration counts equal"""
    from kinectpy_amd.pipeline import NativeFramePipeline, PipelineParams
    xy, depth, rgb, inits, truth, ref = _oracle_steps(oracle, 8, 1)
    nat = NativeFramePipeline(xy, 8, inits, PipelineParams())
    gp, gc, gT = nat.step(torch.as_tensor(depth[0]).cuda(), torch.as_tensor(rgb[0]).cuda())
    rp, rc, rT, aux = ref[0]
    assert np.abs(gT - np.stack(rT)).max() < TOL_T
    assert [s[0] for s in nat.last["icp"]] == [it for it, _, _ in aux["icp"]]
    assert nat.last["n_down"] == [len(x) for x in aux["downs"]] and nat.last["n_fused"] == len(aux["fused"])
    assert np.array_equal(npy(gp), rp) and np.array_equal(npy(gc), rc)


def test_native_frame_step_without_a_person(four_sensor_oracle):
    """all masks empty: the registrations still run (they use every valid pixel), the fused frame is empty, nothing is read past it"""
    from kinectpy_amd.pipeline import NativeFramePipeline, PipelineParams
    xy, depth, rgb, inits, truth, ref = four_sensor_oracle
    nat = NativeFramePipeline(xy, 4, inits, PipelineParams())
    gp, gc, gT = nat.step(torch.as_tensor(depth[0]).cuda(), torch.zeros_like(torch.as_tensor(rgb[0])).cuda())
    assert gp.shape[0] == 0 and gc.shape[0] == 0
    assert np.abs(gT - np.stack(ref[0][2])).max() < TOL_T
    gp2, gc2, gT2 = nat.step(torch.as_tensor(depth[0]).cuda(), torch.as_tensor(rgb[0]).cuda())       # and the next frame is a normal one
    assert np.array_equal(npy(gp2), ref[0][0]) and np.array_equal(npy(gc2), ref[0][1])

"""GPU suite of the occupancy grids (kpx_voxelgrid_*, AC10): every index array and every colour bit for bit against the NumPy
restatement tests/voxelgrid_ref.py, on the synthetic ring of test_tsdf_gpu.py (four cameras of synth.small_xy(8), 80 x 72 pixels,
two time frames) and on small exact scenes."""
import functools
import os

import numpy as np
import pytest

import voxelgrid_ref as R
import voxelgrid_scenes as S

pytestmark = pytest.mark.gpu

W, H, K4 = S.RING_W, S.RING_H, S.RING_K4
SCALE, TRUNC = 1.0, 6000.0                                      # millimetres as they are, nothing cut
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxel_down_sample.npz")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(None)
def ring():
    """depth u16 (2, 4, n_px), rgb u8 (2, 4, n_px, 3), world -> camera extrinsics (4, 4, 4), camera -> world poses"""
    depth, rgb, poses = S.ring()
    return depth, rgb, np.stack([np.linalg.inv(p) for p in poses]), poses


@functools.lru_cache(None)
def cases():
    return {name: (pts, col, v) for name, pts, col, v in S.cloud_cases()}


def o3d():
    from kinectpy_amd import o3d as ns
    return ns


def intrinsic():
    return o3d().camera.PinholeCameraIntrinsic(W, H, *K4)


def cloud(pts, col=None, nrm=None):
    pc = o3d().geometry.PointCloud()
    pc.points = o3d().utility.Vector3dVector(pts)
    if col is not None:
        pc.colors = o3d().utility.Vector3dVector(col)
    if nrm is not None:
        pc.normals = o3d().utility.Vector3dVector(nrm)
    return pc


def indices(grid):
    a = grid.voxel_indices.cpu().numpy()
    assert a.dtype == np.int32 and a.shape == (len(a), 3)
    return a.astype(np.int64)


def assert_grid(grid, idx, col, origin, v):
    assert np.array_equal(indices(grid), idx)
    assert same(grid.voxel_colors.cpu().numpy(), col)
    assert np.array_equal(grid.origin, origin) and grid.voxel_size == v
    assert repr(grid) == f"VoxelGrid with {len(idx)} voxels." and grid.has_voxels() == (len(idx) > 0)


# ---- constructors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["normal1", "normal2", "normal63", "normal64", "normal65", "normal257", "identical65", "one_voxel", "own_voxels", "ring"])
def test_create_from_point_cloud(name):
    pts, col, v = cases()[name]
    VG = o3d().geometry.VoxelGrid
    for c in (col, None):
        idx, rc, origin = R.create_from_point_cloud(pts, v, c)
        grid = VG.create_from_point_cloud(cloud(pts, c), v)
        assert_grid(grid, idx, rc, origin, v)
        assert (c is None) == (not rc.any())
    assert len(idx) == {"identical65": 1, "one_voxel": 1, "own_voxels": len(pts)}.get(name, len(idx))
    # within bounds: the caller's origin, points beyond max_bound indexed like any other
    lo = pts.astype(np.float64).min(0) - np.array([3.0, 0.0, 0.125]) * v
    idx, rc, origin = R.create_from_point_cloud(pts, v, col, origin=lo)
    grid = VG.create_from_point_cloud_within_bounds(cloud(pts, col), v, lo, lo + v)
    assert_grid(grid, idx, rc, lo, v)
    assert 2 <= idx[:, 0].min() <= 3                       # shifted by the three cells (less a rounding) the origin lies below the cloud
    vox = grid.get_voxels()
    assert len(vox) == len(idx) and np.array_equal([t.grid_index for t in vox], idx) and same(np.float32([t.color for t in vox]), rc)
    lo_b, hi_b = R.bounds(idx, lo, v)
    assert np.array_equal(grid.get_min_bound(), lo_b) and np.array_equal(grid.get_max_bound(), hi_b) and np.array_equal(grid.get_center(), (lo_b + hi_b) * 0.5)


def test_create_from_point_cloud_errors_and_empty():
    VG = o3d().geometry.VoxelGrid
    pts = cases()["normal257"][0]
    with pytest.raises(RuntimeError, match="voxel_size is too small"):
        VG.create_from_point_cloud(cloud(pts), 1e-4)                                     # 600 / 1e-4 cells > 2^21
    with pytest.raises(RuntimeError, match="voxel_size is too small"):
        VG.create_from_point_cloud_within_bounds(cloud(pts), 1.0, pts.max(0), pts.max(0) + 1.0)          # points below the origin
    with pytest.raises(RuntimeError, match="voxel_size is too small"):
        VG.create_from_point_cloud(cloud(np.float32([[0, 0, 0], [np.nan, 0, 0]])), 1.0)
    g = VG.create_from_point_cloud(cloud(np.zeros((0, 3), np.float32)), 2.0)
    assert g.is_empty() and np.array_equal(g.origin, [-1.0, -1.0, -1.0]) and g.voxel_size == 2.0 and indices(g).shape == (0, 3)
    assert g.check_if_included([(0.0, 0.0, 0.0)]) == [False]


def test_voxel_down_sample_is_unchanged():
    """the grid steps moved into a shared header: voxel_down_sample's outputs equal the parent commit's, bit for bit (the fixture and
    the script that wrote it are under tests/golden/)"""
    import sys
    sys.path.insert(0, os.path.dirname(GOLDEN))
    try:
        import make_voxel_down_sample_golden as G
    finally:
        sys.path.pop(0)
    want = np.load(GOLDEN)
    seen = set()
    for name, (pts, col, v) in cases().items():
        for tag, c, n in G.variants(pts, col):
            for kind, a in zip(("pts", "col", "nrm"), G.down_sample(pts, c, n, v)):
                key = f"{name}.{tag}.{kind}"
                assert (a is not None) == (key in want.files), key
                if a is not None:
                    assert same(a, want[key]), key
                    seen.add(key)
    assert seen == set(want.files) and len(seen) == 10 * (1 + 2 + 3)


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 3, 5), (64, 1, 1), (17, 33, 9)])
def test_create_dense(dims):
    v, origin, colour = 0.25, (1.0, -2.0, 0.5), (0.1, 0.2, 0.7)
    extent = [d * v + e for d, e in zip(dims, (0.1, -0.1, 0.124))]                    # round(extent / v) == dims
    idx, col, org = R.create_dense(origin, colour, v, *extent)
    assert len(idx) == dims[0] * dims[1] * dims[2] and np.array_equal(idx[-1], np.array(dims) - 1)
    assert np.array_equal(idx, np.array(sorted(map(tuple, idx))).reshape(-1, 3))
    grid = o3d().geometry.VoxelGrid.create_dense(origin, colour, v, *extent)
    assert_grid(grid, idx, col, org, v)
    keys = grid._keys.cpu().numpy()
    assert np.array_equal(keys, R.keys_of(idx)) and (np.diff(keys) > 0).all()


# ---- carving ---------------------------------------------------------------------------------------------------------------------------
def images(count):
    """(depth u16, person mask u8, extrinsic, camera number 0..7) of frame 0's four cameras, frame 1's four, and round again"""
    depth, rgb, extr, _ = ring()
    return [(depth[(i // 4) % 2, i % 4], rgb[(i // 4) % 2, i % 4].any(1).astype(np.uint8), extr[i % 4], i % 8) for i in range(count)]


@functools.lru_cache(None)
def grid_def(name):
    """(idx, colours, origin, voxel size) of the restatement"""
    if name == "cloud":
        pts, col, _ = cases()["ring"]
        return R.create_from_point_cloud(pts, 50.0, col) + (50.0,)
    dims, v, origin = {"dense3": ((3, 3, 3), 600.0, (-900.0, -900.0, -900.0)), "dense16": ((16, 16, 16), 125.0, (-1000.0, -1100.0, -1000.0)),
                       "dense33x17x65": ((33, 17, 65), 60.0, (-990.0, -500.0, -1950.0))}[name]
    return R.create_dense(origin, (0.25, 0.5, 0.75), v, *(d * v for d in dims)) + (v,)


def gpu_grid(name):
    VG = o3d().geometry.VoxelGrid
    idx, col, origin, v = grid_def(name)
    if name == "cloud":
        pts, c, _ = cases()["ring"]
        g = VG.create_from_point_cloud(cloud(pts, c), v)
    else:
        g = VG.create_dense(origin, (0.25, 0.5, 0.75), v, *((idx.max(0) + 1) * v))
    assert np.array_equal(indices(g), idx)
    return g


@functools.lru_cache(None)
def projection(name, cam):
    """the corners of grid `name` in camera `cam` (0..3): the restatement's u, v, z, computed once"""
    idx, _, origin, v = grid_def(name)
    return R.project(R.corners(idx, origin, v), K4, ring()[2][cam])


def ref_survivors(name, ims, mode, keep_outside, keep_unmeasured):
    idx = grid_def(name)[0]
    alive = np.ones(len(idx), bool)
    for d, m, _, cam in ims:
        image = (R.depth_from_u16(d, SCALE, TRUNC) if mode == "depth" else R.mask_from_u8(m)).reshape(H, W)
        alive &= R.corner_keeps(image, *projection(name, cam % 4), mode, keep_outside, keep_unmeasured).any(1)
    return np.flatnonzero(alive)


def params(E):
    return o3d().camera.PinholeCameraParameters(intrinsic(), E)


@pytest.mark.parametrize("count", [1, 4, 8, 9, 17])
@pytest.mark.parametrize("name", ["dense3", "dense16", "dense33x17x65", "cloud"])
def test_carve_against_the_restatement(name, count):
    """the one-pass batch forms (uint16 frames / uint8 masks, more images than a launch holds) == single float32 calls in three
    orders == the restatement"""
    Image = o3d().geometry.Image
    idx, col, _, _ = grid_def(name)
    ims = images(count)
    orders = [list(range(count)), list(range(count))[::-1], [(5 * i + 3) % count for i in range(count)] if count % 5 else list(np.roll(range(count), 2))]
    assert all(sorted(o) == list(range(count)) for o in orders)
    base = gpu_grid(name)
    sizes = set()
    for mode, keep_outside, keep_unmeasured in [("depth", False, False), ("depth", True, False), ("depth", False, True), ("depth", True, True),
                                                ("silhouette", False, False), ("silhouette", True, False)]:
        want = ref_survivors(name, ims, mode, keep_outside, keep_unmeasured)
        sizes.add(len(want))
        g = o3d().geometry.VoxelGrid(base)
        E = np.stack([e for _, _, e, _ in ims])
        if mode == "depth":
            assert g.carve_depth_maps(np.stack([d for d, _, _, _ in ims]), intrinsic(), E, keep_outside, SCALE, TRUNC, keep_unmeasured) is g
        else:
            assert g.carve_silhouettes(np.stack([m for _, m, _, _ in ims]), intrinsic(), E, keep_outside) is g
        tag = (mode, keep_outside, keep_unmeasured)
        assert np.array_equal(indices(g), idx[want]), tag
        assert same(g.voxel_colors.cpu().numpy(), col[want]), tag
        for order in orders:
            g = o3d().geometry.VoxelGrid(base)
            for i in order:
                d, m, e, _ = ims[i]
                if mode == "depth":
                    assert g.carve_depth_map(Image(R.depth_from_u16(d, SCALE, TRUNC).reshape(H, W)), params(e), keep_outside, keep_unmeasured) is g
                else:
                    assert g.carve_silhouette(Image(R.mask_from_u8(m).reshape(H, W)), params(e), keep_outside) is g
            assert np.array_equal(indices(g), idx[want]), (tag, order[:3])
            assert same(g.voxel_colors.cpu().numpy(), col[want])
        assert np.array_equal(indices(base), idx)                   # the copies are carved, not the grid they were made from
    if name != "dense3":
        assert len(sizes) >= 4 and 0 < min(sizes) and max(sizes) < len(idx), sizes          # the flags matter and nothing is trivial


def test_a_grid_no_image_sees():
    """every corner projects outside all four images: empty with keep_voxels_outside_image False, unchanged with True"""
    VG = o3d().geometry.VoxelGrid
    depth, rgb, extr, _ = ring()
    origin, v = (-500.0, -40000.0, -500.0), 125.0
    idx, col, _ = R.create_dense(origin, (1.0, 0.0, 0.0), v, 1000.0, 1000.0, 1000.0)
    for cam in range(4):
        u, w, z = R.project(R.corners(idx, origin, v), K4, extr[cam])
        assert not R.sample(np.ones((H, W), np.float32), u, w)[0].any()
    for keep, left in ((False, 0), (True, len(idx))):
        g = VG.create_dense(origin, (1.0, 0.0, 0.0), v, 1000.0, 1000.0, 1000.0).carve_depth_maps(depth[0], intrinsic(), extr, keep, SCALE, TRUNC)
        assert len(indices(g)) == left and g.is_empty() == (left == 0)
        g = VG.create_dense(origin, (1.0, 0.0, 0.0), v, 1000.0, 1000.0, 1000.0).carve_silhouettes(rgb[0].any(2), intrinsic(), extr, keep)
        assert len(indices(g)) == left
        if left:
            assert np.array_equal(indices(g), idx) and same(g.voxel_colors.cpu().numpy(), col)


def test_edge_decisions_on_the_device():
    ns = o3d()
    cam = ns.camera.PinholeCameraParameters(ns.camera.PinholeCameraIntrinsic(S.W, S.H, *S.K4), np.eye(4))
    for name, origin, image, mode, survives in S.edge_scenes():
        g = ns.geometry.VoxelGrid.create_dense(origin, (0.0, 0.0, 0.0), 1.0, 1.0, 1.0, 1.0)
        assert len(indices(g)) == 1
        if mode == "depth":
            g.carve_depth_map(ns.geometry.Image(image), cam)
        else:
            g.carve_silhouette(ns.geometry.Image(image), cam)
        assert g.has_voxels() == survives, name
    # a voxel behind the camera (test_voxelgrid_cpu.py): a depth map never keeps it, a silhouette keeps its mirrored projection
    cam9 = ns.camera.PinholeCameraParameters(ns.camera.PinholeCameraIntrinsic(9, 9, 4.0, 4.0, 4.0, 4.0), np.eye(4))
    behind = lambda: ns.geometry.VoxelGrid.create_dense((0.0, 0.0, -2.0), (0.0, 0.0, 0.0), 1.0, 1.0, 1.0, 1.0)
    ones = np.ones((9, 9), np.float32)
    assert behind().carve_depth_map(ns.geometry.Image(np.full((9, 9), 0.5, np.float32)), cam9, True).is_empty()
    assert behind().carve_silhouette(ns.geometry.Image(ones), cam9).has_voxels()
    left = ones.copy()
    left[:, :5] = 0.0
    assert behind().carve_silhouette(ns.geometry.Image(left), cam9).is_empty()
    assert behind().carve_depth_map(ns.geometry.Image(left), cam9, False, keep_unmeasured=True).has_voxels()
    assert behind().carve_silhouette(ns.geometry.Image(np.full((9, 9), np.nan, np.float32)), cam9, True).is_empty()


def test_empty_grid_and_no_images():
    ns = o3d()
    depth, rgb, extr, _ = ring()
    g = ns.geometry.VoxelGrid.create_dense((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 10.0, 4.0, 100.0, 100.0)               # round(0.4) = 0 cells
    assert g.is_empty() and g.carve_depth_maps(depth[0], intrinsic(), extr).is_empty() and g.carve_silhouettes(rgb[0].any(2), intrinsic(), extr).is_empty()
    cam = params(extr[0])
    assert g.carve_depth_map(ns.geometry.Image(np.ones((H, W), np.float32)), cam).is_empty() and indices(g).shape == (0, 3)
    # a grid carved to nothing stays a valid empty grid
    g = gpu_grid("dense3").carve_depth_maps(np.zeros((1, H * W), np.uint16), intrinsic(), extr[:1])
    assert g.is_empty() and g.get_voxels() == [] and g.carve_depth_maps(depth[0], intrinsic(), extr).is_empty()
    assert np.array_equal(g.get_min_bound(), g.origin) and g.check_if_included([g.origin + 1.0]) == [False]
    # no image: nothing is carved
    g = gpu_grid("dense3").carve_depth_maps(np.zeros((0, H * W), np.uint16), intrinsic(), np.zeros((0, 4, 4)))
    assert len(indices(g)) == 27


@pytest.mark.parametrize("m", [1, 64, 65, 257])
def test_only_the_last_voxel_survives(m):
    """a row of m voxels along x (the ends of waves and blocks); the mask's one lit column is reached only by the last voxel's far face"""
    ns = o3d()
    # x in [0, m], y in [0, 1], z in [1, 2]; K = (1, 1, 0, 0): u = x / z, v = y / z.  The far corner (m, ., 1) projects to u = m.
    Wm = m + 2
    mask = np.zeros((3, Wm), np.float32)
    mask[:, m] = 1.0
    cam = ns.camera.PinholeCameraParameters(ns.camera.PinholeCameraIntrinsic(Wm, 3, 1.0, 1.0, 0.0, 0.0), np.eye(4))
    idx, col, origin = R.create_dense((0.0, 0.0, 1.0), (0.5, 0.5, 0.5), 1.0, float(m), 1.0, 1.0)
    want = np.flatnonzero(R.carve(idx, origin, 1.0, mask, (1.0, 1.0, 0.0, 0.0), np.eye(4), "silhouette"))
    # the sample is positive for m - 1 < u < m + 1: the last voxel's corner at u = m, and the one before only at u = m - 1 exactly (weight 0)
    assert list(want) == [m - 1]
    g = ns.geometry.VoxelGrid.create_dense((0.0, 0.0, 1.0), (0.5, 0.5, 0.5), 1.0, float(m), 1.0, 1.0).carve_silhouette(ns.geometry.Image(mask), cam)
    assert np.array_equal(indices(g), idx[want])
    g = ns.geometry.VoxelGrid.create_dense((0.0, 0.0, 1.0), (0.5, 0.5, 0.5), 1.0, float(m), 1.0, 1.0)
    g.carve_silhouettes((mask != 0)[None], cam.intrinsic, np.eye(4)[None])
    assert np.array_equal(indices(g), idx[want]) and same(g.voxel_colors.cpu().numpy(), col[want])


# ---- inclusion -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense3", "cloud", "one", "none"])
def test_check_if_included(name):
    import torch
    ns = o3d()
    if name in ("one", "none"):
        idx, origin, v = np.array([[5, 0, 7]][: name == "one"], np.int64).reshape(-1, 3), np.array([0.5, -1.0, 2.0]), 0.25
        g = ns.geometry.VoxelGrid.create_from_point_cloud_within_bounds(cloud(np.float32([[1.8, -0.9, 3.8]][: name == "one"])), v, origin, origin + 1.0)
        assert np.array_equal(indices(g), idx)
    else:
        idx, _, origin, v = grid_def(name)
        g = gpu_grid(name)
    first = idx[0] if len(idx) else np.array([5, 0, 7])
    q = np.concatenate([R.centres(idx, origin, v)[:3000],
                        R.corners([first], origin, v)[0],                                    # face membership by floor: only the low corner is inside
                        origin[None] - v * np.array([[0.5, 0, 0], [0, 1e-9, 0], [0, 0, 3.0]]),     # below the origin
                        origin[None] + v * np.array([[2.0 ** 21, 0, 0], [0, 2.0 ** 21 + 0.5, 0], [1e30, 0, 0]]),          # beyond 2^21 cells
                        [[np.nan, 0.0, 0.0], [0.0, np.nan, 0.0], [np.inf, 0.0, 0.0], [-np.inf, 0.0, 0.0]],
                        R.centres(idx[-3:] + [[0, 0, 1]], origin, v)])
    for dtype in (np.float64, np.float32):
        qq = q.astype(dtype)
        want = R.included(idx, origin, v, qq)
        mask = g.included_mask(torch.as_tensor(qq).cuda())
        assert mask.dtype == torch.bool and mask.is_cuda and np.array_equal(mask.cpu().numpy(), want), dtype
        assert g.check_if_included(qq) == list(want)
        assert np.array_equal(g.included_mask(qq).cpu().numpy(), want)
    n_own = min(len(idx), 3000)
    want = R.included(idx, origin, v, q)
    assert want[:n_own].all() and not want[n_own + 8: n_own + 18].any()
    if name == "one":
        assert list(want[n_own: n_own + 8]) == [True] + [False] * 7          # an isolated voxel owns its low corner only
    elif name == "dense3":
        assert want[n_own: n_own + 8].all()                                  # the other corners belong to the neighbours
    assert g.check_if_included(ns.utility.Vector3dVector(q)) == list(R.included(idx, origin, v, q.astype(np.float32)))


# ---- the rig's filter ------------------------------------------------------------------------------------------------------------------
def streak_points(depth, extr, count=200, z0=4000.0, voxel=20.0):
    """`count` points on rays of camera 0 at z0 -- halfway between the person (2500 from the camera) and the far wall (5500) -- chosen
    by geometry alone: a candidate qualifies when some other camera measures THROUGH it, i.e. every pixel a corner of its voxel can
    sample there (the footprint of a `voxel` cube around the point, plus the bilinear taps) holds a depth more than two voxels behind
    it.  Such a voxel has no corner that this camera keeps, whatever the drop-outs elsewhere do."""
    fx, fy, cx, cy = K4
    pix = np.arange(H * W)
    cand = np.stack([((pix % W) - cx) / fx * z0, ((pix // W) - cy) / fy * z0, np.full(len(pix), z0)], 1)
    clean = np.zeros(len(pix), bool)
    for s in range(1, len(extr)):
        d = depth[s].reshape(H, W).astype(np.float64)
        p = cand @ extr[s][:3, :3].T + extr[s][:3, 3]
        for i in np.flatnonzero(p[:, 2] > voxel):
            e = fx * voxel / (p[i, 2] - voxel)
            u, v = fx * p[i, 0] / p[i, 2] + cx, fy * p[i, 1] / p[i, 2] + cy
            u0, u1, v0, v1 = int(np.floor(u - e)), int(np.floor(u + e)) + 1, int(np.floor(v - e)), int(np.floor(v + e)) + 1
            if u0 >= 0 and v0 >= 0 and u1 <= W - 1 and v1 <= H - 1 and d[v0:v1 + 1, u0:u1 + 1].min() > p[i, 2] + 2.0 * voxel:
                clean[i] = True
    sel = np.flatnonzero(clean)
    assert len(sel) >= count
    return cand[sel[np.linspace(0, len(sel) - 1, count).astype(int)]].astype(np.float32)


@functools.lru_cache(None)
def streak_scene():
    """the fused ring cloud in the master's frame + 200 flying pixels of camera 0 halfway between the person and the far wall"""
    from kinectpy_amd.utils import synth
    _, depth, _, _, truth = synth.sensor_ring(4, xy=synth.small_xy(8))
    to_master = [np.eye(4)] + list(truth)
    parts = [S.unproject(depth[0, s], to_master[s])[0] for s in range(4)]
    streak = streak_points(depth[0], [np.linalg.inv(T) for T in to_master])
    assert len(np.unique(streak, axis=0)) == 200
    return np.concatenate(parts + [streak]), depth[0], truth


def test_remove_free_space_points_on_the_ring():
    """the streak lies where cameras 1..3 measure through: at 20 mm voxels every streak point goes, and the kept indices are the
    restatement's"""
    from kinectpy_amd.preprocessing.fusion import remove_free_space_points
    pts, depth, truth = streak_scene()
    n0 = len(pts) - 200
    extr = [np.eye(4)] + [np.linalg.inv(T) for T in truth]
    idx, _, origin = R.create_from_point_cloud(pts, 20.0)
    alive = R.carve_all(idx, origin, 20.0, [R.depth_from_u16(d, 1.0, 6000.0).reshape(H, W) for d in depth], K4, extr, "depth", True, True)
    want = np.flatnonzero(R.included(idx[alive], origin, 20.0, pts))
    assert not (want >= n0).any() and len(want) > 0.9 * n0, (len(want), n0)
    out, kept = remove_free_space_points(cloud(pts), depth, intrinsic(), truth, 20.0)
    kept = kept.cpu().numpy()
    assert np.array_equal(kept, want)
    assert same(out._pts.cpu().numpy(), pts[want])
    # Open3D's rule (keep_unmeasured False) lets every drop-out pixel carve its ray: fewer points stay
    _, strict = remove_free_space_points(cloud(pts), depth, intrinsic(), truth, 20.0, keep_unmeasured=False)
    alive = R.carve_all(idx, origin, 20.0, [R.depth_from_u16(d, 1.0, 6000.0).reshape(H, W) for d in depth], K4, extr, "depth", True, False)
    assert np.array_equal(strict.cpu().numpy(), np.flatnonzero(R.included(idx[alive], origin, 20.0, pts))) and len(strict) <= len(kept)


def test_image_format_errors():
    ns = o3d()
    depth, rgb, extr, _ = ring()
    g = gpu_grid("dense3")
    cam = params(extr[0])
    f32 = R.depth_from_u16(depth[0, 0], SCALE, TRUNC)
    for method in (g.carve_depth_map, g.carve_silhouette):
        with pytest.raises(RuntimeError, match="Unsupported image format"):          # still uint16
            method(ns.geometry.Image(depth[0, 0].reshape(H, W)), cam)
        with pytest.raises(RuntimeError, match="Unsupported image format"):          # three channels
            method(ns.geometry.Image(rgb[0, 0].reshape(H, W, 3)), cam)
        with pytest.raises(RuntimeError, match="not compatible with the provided camera_parameters"):
            method(ns.geometry.Image(f32.reshape(W, H)), cam)
        with pytest.raises(RuntimeError, match="not compatible with the provided camera_parameters"):
            method(ns.geometry.Image(f32.reshape(H, W)), ns.camera.PinholeCameraParameters(ns.camera.PinholeCameraIntrinsic(W + 1, H, *K4), extr[0]))
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        g.carve_depth_maps(depth[0, :, :-1], intrinsic(), extr)
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        g.carve_silhouettes(depth[0], intrinsic(), extr)
    assert len(indices(g)) == 27

"""GPU suite of the TSDF integration (kpx_tsdf_*, AC9): every volume, point, normal and colour bit for bit against the NumPy
restatement tests/tsdf_ref.py on the synthetic ring (four cameras of synth.small_xy(8), 80 x 72 pixels, two time frames)."""
import functools

import numpy as np
import pytest

import tsdf_ref as R

pytestmark = pytest.mark.gpu

W, H, K4 = 80, 72, (63.0, 63.0, 40.0, 36.0)
LENGTH, ORIGIN = 2000.0, (-1000.0, -1100.0, -1000.0)           # the person stands at the world's origin
SCALE, TRUNC = 1.0, 6000.0                                      # millimetres as they are, nothing cut


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(None)
def ring():
    """depth u16 (2, 4, n_px), rgb u8 (2, 4, n_px, 3), world -> camera extrinsics of the four ring cameras"""
    from kinectpy_amd.utils import synth
    _, depth, rgb, _, _ = synth.sensor_ring(4, 2, synth.small_xy(8))
    extr = np.stack([np.linalg.inv(synth.camera_pose(g, 4)) for g in range(4)])
    return depth, rgb, extr


def intrinsic():
    from kinectpy_amd import o3d
    return o3d.camera.PinholeCameraIntrinsic(W, H, *K4)


def gpu_volume(res, color=True, origin=ORIGIN, length=LENGTH):
    from kinectpy_amd import o3d
    ns = o3d.pipelines.integration
    return ns.UniformTSDFVolume(length, res, 4.0 * length / res, ns.TSDFVolumeColorType.RGB8 if color else ns.TSDFVolumeColorType.NoColor, origin)


def ref_volume(res, color=True, origin=ORIGIN, length=LENGTH):
    return R.Volume(length, res, 4.0 * length / res, origin, color)


def rgbd(depth_u16, rgb_u8, scale=SCALE, trunc=TRUNC):
    from kinectpy_amd import o3d
    return o3d.geometry.RGBDImage.create_from_color_and_depth(rgb_u8.reshape(H, W, 3), depth_u16.reshape(H, W), scale, trunc, False)


def images(count):
    """the first `count` (depth, rgb, extrinsic) of frame 0's four cameras, frame 1's four, and round again"""
    depth, rgb, extr = ring()
    return [(depth[(i // 4) % 2, i % 4], rgb[(i // 4) % 2, i % 4], extr[i % 4]) for i in range(count)]


def ref_integrate(vol, ims, scale=SCALE, trunc=TRUNC):
    for d, c, E in ims:
        R.integrate(vol, R.depth_from_u16(d, scale, trunc), c, K4, W, H, E)
    return vol


def gpu_arrays(vol):
    v = vol._vol.cpu().numpy()
    return np.ascontiguousarray(v[:, 0]), np.ascontiguousarray(v[:, 1]), None if vol._col is None else vol._col.cpu().numpy()


def assert_volume(vol, ref):
    f, w, c = gpu_arrays(vol)
    assert same(w, ref.w), f"weights differ at {np.flatnonzero(w != ref.w)[:5]}"
    assert same(f, ref.tsdf), f"tsdf differs at {np.flatnonzero(bits(f) != bits(ref.tsdf))[:5]}"
    if ref.col is not None:
        assert same(c, ref.col)


def upload(vol, ref):
    import torch
    vol._vol.copy_(torch.from_numpy(np.stack([ref.tsdf, ref.w], 1)))
    if ref.col is not None:
        vol._col.copy_(torch.from_numpy(ref.col))


def assert_extractions(vol, ref):
    pc = vol.extract_point_cloud()
    pts, nrm, col = R.extract_point_cloud(ref)
    g = pc._pts.cpu().numpy()
    assert g.shape == pts.shape, (g.shape, pts.shape)
    assert same(g, pts)
    assert same(pc._nrm.cpu().numpy(), nrm)
    if ref.col is not None:
        assert same(pc._col.cpu().numpy(), col)
    else:
        assert pc._col is None
    vc = vol.extract_voxel_point_cloud()
    vp, vg = R.extract_voxel_point_cloud(ref)
    assert same(vc._pts.cpu().numpy(), vp) and same(vc._col.cpu().numpy(), vg)
    return len(pts), len(vp)


@functools.lru_cache(None)
def integrated(res):
    """(device volume, restatement) after the four ring poses of frame 0 and of frame 1, one integrate() call per image"""
    vol, ref = gpu_volume(res), ref_volume(res)
    for d, c, E in images(8):
        vol.integrate(rgbd(d, c), intrinsic(), E)
    return vol, ref_integrate(ref, images(8))


RESOLUTIONS = (2, 3, 16, 33, 64, 96)          # odd volumes, rows that are no multiple of the pair, the wave or the block


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_integrate_two_frames_of_four_poses(res):
    vol, ref = integrated(res)
    assert_volume(vol, ref)
    if res >= 16:
        assert ref.w.max() == 8.0 and ref.w.min() < 8.0 and (ref.w > 0).mean() > 0.5


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_extraction_of_the_integrated_volumes(res):
    vol, ref = integrated(res)
    n_surface, n_voxels = assert_extractions(vol, ref)
    assert (n_surface > 0) == (res >= 3) and n_voxels > 0          # resolution 2 has no neighbour below res - 1


@pytest.mark.parametrize("res,npts", [(32, 687), (48, 1442), (64, 2356)])
def test_extraction_counts_of_the_prototype(res, npts):
    """frame 0's four cameras in one integrate_frames call; the prototype of the issue extracted 687 / 1442 / 2356 points"""
    depth, rgb, extr = ring()
    vol, ref = gpu_volume(res), ref_integrate(ref_volume(res), images(4))
    vol.integrate_frames(depth[0], rgb[0], intrinsic(), extr, SCALE, TRUNC)
    assert_volume(vol, ref)
    assert assert_extractions(vol, ref)[0] == npts


def test_camera_inside_the_volume():
    """voxels behind the camera (z <= 0) are skipped"""
    depth, rgb, _ = ring()
    E = np.eye(4)
    E[:3, 3] = (0.0, 200.0, 300.0)                  # the camera sits at (0, -200, -300), inside the volume, looking along +z
    vol, ref = gpu_volume(33), ref_volume(33)
    vol.integrate(rgbd(depth[0, 0], rgb[0, 0]), intrinsic(), E)
    ref_integrate(ref, [(depth[0, 0], rgb[0, 0], E)])
    gz = ref.centres()[2]
    assert (gz + 300.0 <= 0).sum() > 5 and not ref.w.reshape(33, 33, 33)[:, :, gz + 300.0 <= 0].any() and ref.w.any()
    assert_volume(vol, ref)
    assert_extractions(vol, ref)


def test_depth_trunc_cuts_part_of_the_image():
    depth, rgb, extr = ring()
    cut = 2600.0
    assert 0.2 < (depth[0] > cut).mean() < 0.8
    vol, ref = gpu_volume(33), ref_integrate(ref_volume(33), images(4), SCALE, cut)
    vol.integrate_frames(depth[0], rgb[0], intrinsic(), extr, SCALE, cut)
    assert_volume(vol, ref)
    full = ref_integrate(ref_volume(33), images(4))
    assert not np.array_equal(full.w, ref.w)
    # a scale that does not divide evenly: the float32 division in the kernel is the host's
    vol, ref = gpu_volume(33), ref_integrate(ref_volume(33), images(4), 1.7, 1500.0)
    vol.integrate_frames(depth[0], rgb[0], intrinsic(), extr, 1.7, 1500.0)
    assert_volume(vol, ref)


def test_volume_outside_every_frustum_is_untouched():
    import torch
    depth, rgb, extr = ring()
    vol = gpu_volume(33, origin=(-1000.0, -30000.0, -1000.0))
    g = torch.Generator().manual_seed(1)
    vol._vol.copy_(torch.rand(vol._vol.shape, generator=g))
    vol._col.copy_(torch.rand(vol._col.shape, generator=g))
    before = [t.clone() for t in (vol._vol, vol._col)]
    vol.integrate_frames(depth[0], rgb[0], intrinsic(), extr, SCALE, TRUNC)
    for d, c, E in images(4):
        vol.integrate(rgbd(d, c), intrinsic(), E)
    assert torch.equal(vol._vol, before[0]) and torch.equal(vol._col, before[1])
    ref = ref_integrate(ref_volume(33, origin=(-1000.0, -30000.0, -1000.0)), images(4))
    assert not ref.w.any()


@pytest.mark.parametrize("count", [1, 2, 4, 8, R.MAX_SENSORS + 3])
def test_batch_equals_sequential_equals_restatement(count):
    """integrate_frames (uint16 frames converted in the kernel, up to KPX_TSDF_MAX_SENSORS per launch) == one integrate() per
    host-converted float32 image == the restatement"""
    ims = images(count)
    ref = ref_integrate(ref_volume(33), ims)
    seq = gpu_volume(33)
    for d, c, E in ims:
        seq.integrate(rgbd(d, c), intrinsic(), E)
    assert_volume(seq, ref)
    batch = gpu_volume(33)
    batch.integrate_frames(np.stack([d for d, _, _ in ims]), np.stack([c for _, c, _ in ims]), intrinsic(), np.stack([E for _, _, E in ims]), SCALE, TRUNC)
    assert_volume(batch, ref)
    nocol = gpu_volume(33, color=False)
    nocol.integrate_frames(np.stack([d for d, _, _ in ims]), None, intrinsic(), np.stack([E for _, _, E in ims]), SCALE, TRUNC)
    f, w, c = gpu_arrays(nocol)
    assert c is None and same(f, ref.tsdf) and same(w, ref.w)


def test_image_format_errors():
    from kinectpy_amd import o3d
    depth, rgb, extr = ring()
    vol = gpu_volume(8)
    with pytest.raises(RuntimeError, match="Unsupported image format"):          # depth still uint16
        vol.integrate(o3d.geometry.RGBDImage(rgb[0, 0].reshape(H, W, 3), depth[0, 0].reshape(H, W)), intrinsic(), extr[0])
    with pytest.raises(RuntimeError, match="Unsupported image format"):          # intensity image into an RGB8 volume
        vol.integrate(o3d.geometry.RGBDImage.create_from_color_and_depth(rgb[0, 0].reshape(H, W, 3), depth[0, 0].reshape(H, W)), intrinsic(), extr[0])
    with pytest.raises(RuntimeError, match="Unsupported image format"):          # size differs from the intrinsic
        vol.integrate(rgbd(depth[0, 0], rgb[0, 0]), o3d.camera.PinholeCameraIntrinsic(W + 1, H, *K4), extr[0])
    with pytest.raises(RuntimeError, match="Unsupported image format"):
        vol.integrate_frames(depth[0, :, :-1], rgb[0, :, :-1], intrinsic(), extr, SCALE, TRUNC)
    assert not vol._vol.any()


def test_empty_volume_and_single_crossing():
    vol, ref = gpu_volume(16), ref_volume(16)
    assert assert_extractions(vol, ref) == (0, 0)
    a, b = (5 * 16 + 7) * 16 + 9, (6 * 16 + 7) * 16 + 9            # neighbours along x
    ref.tsdf[[a, b]], ref.w[[a, b]] = (0.25, -0.5), (1.0, 3.0)
    ref.col[a], ref.col[b] = (10.0, 20.0, 30.0), (200.0, 100.0, 50.0)
    upload(vol, ref)
    assert assert_extractions(vol, ref) == (1, 2)
    lin, axis = R.crossings(ref)
    assert list(lin) == [a] and list(axis) == [0]


def random_volume(res, density, seed, color=True):
    """a volume whose voxels are valid with probability ~density, signs at random: crossings in every position of a counting block"""
    rng = np.random.default_rng(seed)
    ref = ref_volume(res, color)
    n = res ** 3
    ref.tsdf[:] = rng.uniform(-1.1, 1.1, n).astype(np.float32)
    ref.w[:] = (rng.random(n) < density) * rng.integers(1, 5, n)
    if color:
        ref.col[:] = rng.uniform(0, 255, (n, 3)).astype(np.float32)
    return ref


def test_crossings_at_the_edges_of_the_counting_blocks():
    """found with the restatement, as batch_edge_cases does for FGR: crossings in the last voxel of a counting block and in the
    first voxel of the next one, blocks without any, and a last block that is not full (21^3 = 18 * 512 + 45)"""
    ref = random_volume(21, 0.5, 3)
    lin, _ = R.crossings(ref)
    blocks = lin // R.COUNT_BLOCK
    last, first = set(blocks[lin % R.COUNT_BLOCK == R.COUNT_BLOCK - 1]), set(blocks[lin % R.COUNT_BLOCK == 0])
    assert any(b + 1 in first for b in last) and blocks.max() == 21 ** 3 // R.COUNT_BLOCK
    vol = gpu_volume(21)
    upload(vol, ref)
    assert assert_extractions(vol, ref)[0] == len(lin)
    sparse = random_volume(21, 0.02, 4)
    lin, _ = R.crossings(sparse)
    assert 0 < len(set(lin // R.COUNT_BLOCK)) < 21 ** 3 // R.COUNT_BLOCK          # some blocks count nothing
    upload(vol, sparse)
    assert assert_extractions(vol, sparse)[0] == len(lin)


def test_extraction_at_resolution_128():
    """4096 counting blocks: more than one count per thread of the scan"""
    ref = random_volume(128, 0.05, 5, color=False)
    vol = gpu_volume(128, color=False)
    upload(vol, ref)
    n_surface, n_voxels = assert_extractions(vol, ref)
    assert n_surface > 1000 and n_voxels > 50000


def test_reset_then_integrate_equals_a_fresh_volume():
    depth, rgb, extr = ring()
    vol = gpu_volume(33)
    vol.integrate_frames(depth[1], rgb[1], intrinsic(), extr, SCALE, TRUNC)
    assert vol._vol.any()
    vol.reset()
    assert not vol._vol.any() and not vol._col.any()
    vol.integrate_frames(depth[0], rgb[0], intrinsic(), extr, SCALE, TRUNC)
    assert_volume(vol, ref_integrate(ref_volume(33), images(4)))


def test_fuse_depth_tsdf_on_the_ring():
    from kinectpy_amd.preprocessing.fusion import fuse_depth_tsdf
    from kinectpy_amd.utils import synth
    _, depth, rgb, _, truth = synth.sensor_ring(4, xy=synth.small_xy(8))
    origin = (-1000.0, -1100.0, 1500.0)                 # the master's frame: the person stands 2500 in front of it
    pc = fuse_depth_tsdf(depth[0], rgb[0], intrinsic(), truth, LENGTH, 32, origin)
    ref = ref_volume(32, origin=origin)
    for s, E in enumerate([np.eye(4)] + [np.linalg.inv(T) for T in truth]):
        R.integrate(ref, R.depth_from_u16(depth[0, s], 1.0, 6000.0), rgb[0, s], K4, W, H, E)
    pts, nrm, col = R.extract_point_cloud(ref)
    assert len(pts) == 687
    assert same(pc._pts.cpu().numpy(), pts) and same(pc._nrm.cpu().numpy(), nrm) and same(pc._col.cpu().numpy(), col)
    nocol = fuse_depth_tsdf(depth[0], None, intrinsic(), truth, LENGTH, 32, origin)
    assert same(nocol._pts.cpu().numpy(), pts) and nocol._col is None

"""GPU suite of the block-sparse TSDF volume (ScalableTSDFVolume, kpx_tsdf_blocks_*, AC16): block indices, every block's voxels and
every extracted point, normal, colour, vertex and triangle bit for bit against the NumPy restatement tests/tsdf_blocks_ref.py on
the synthetic ring (four cameras of synth.small_xy(8), 80 x 72 pixels, two time frames, millimetres, the person at the world's
origin so that block indices of both signs occur).  depth_trunc 2600 keeps the person and cuts the far walls: the restatement
integrates block by block, and a scene of a few hundred blocks keeps every case at a second or two."""
import functools

import numpy as np
import pytest

import tsdf_blocks_ref as B
import tsdf_mesh_ref as M
import tsdf_ref as R

pytestmark = pytest.mark.gpu

W, H, K4 = 80, 72, (63.0, 63.0, 40.0, 36.0)
VL = 2000.0 / 64
SCALE, TRUNC = 1.0, 2600.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}.get(a.dtype, a.dtype))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(None)
def ring():
    from kinectpy_amd.utils import synth
    _, depth, rgb, _, _ = synth.sensor_ring(4, 2, synth.small_xy(8))
    extr = np.stack([np.linalg.inv(synth.camera_pose(g, 4)) for g in range(4)])
    return depth, rgb, extr


def intrinsic():
    from kinectpy_amd import o3d
    return o3d.camera.PinholeCameraIntrinsic(W, H, *K4)


def images(count, start=0):
    """`count` (depth u16, rgb u8, extrinsic) from image `start` on: frame 0's four cameras, frame 1's four, and round again"""
    depth, rgb, extr = ring()
    return [(depth[(i // 4) % 2, i % 4], rgb[(i // 4) % 2, i % 4], extr[i % 4]) for i in range(start, start + count)]


def f32(depth_u16):
    return R.depth_from_u16(depth_u16, SCALE, TRUNC).reshape(H, W)


def rgbd(depth_f32, rgb_u8):
    from kinectpy_amd import o3d
    return o3d.geometry.RGBDImage(rgb_u8.reshape(H, W, 3), np.ascontiguousarray(depth_f32, dtype=np.float32).reshape(H, W))


def gpu_volume(res, t_vox, stride, color, vl=VL, **kw):
    from kinectpy_amd import o3d
    ns = o3d.pipelines.integration
    return ns.ScalableTSDFVolume(vl, t_vox * vl, ns.TSDFVolumeColorType.RGB8 if color else ns.TSDFVolumeColorType.NoColor, res, stride, **kw)


def gpu_frames(vol, ims):
    vol.integrate_frames(np.stack([d for d, _, _ in ims]), np.stack([c for _, c, _ in ims]) if vol._col is not None else None, intrinsic(),
                         np.stack([E for _, _, E in ims]), SCALE, TRUNC)
    return vol


def gpu_single(vol, ims):
    for d, c, E in ims:
        vol.integrate(rgbd(f32(d), c), intrinsic(), E)
    return vol


def ref_integrate(blk, ims):
    for d, c, E in ims:
        B.integrate(blk, f32(d), c, K4, W, H, E)
    return blk


def assert_units(vol, blk):
    idx = vol.volume_unit_indices()
    assert idx.dtype == np.int32 and np.array_equal(idx, blk.indices()), (idx.shape, blk.indices().shape)
    assert vol.volume_unit_count() == len(blk.units)
    tw, col = vol.unit_arrays()
    rtw, rcol = blk.arrays()
    assert same(tw[..., 1], rtw[..., 1]), "weights differ"
    assert same(tw[..., 0], rtw[..., 0]), "tsdf differs"
    if blk.color:
        assert same(col, rcol)
    else:
        assert col is None


def gpu_extractions(vol):
    pc, vc, m = vol.extract_point_cloud(), vol.extract_voxel_point_cloud(), vol.extract_triangle_mesh()
    host = lambda t: None if t is None else t.cpu().numpy()
    return (host(pc._pts), host(pc._nrm), host(pc._col)), (host(vc._pts), host(vc._col)), (host(m._vert), host(m._vcol), host(m._tri))


def assert_extractions(vol, blk):
    (pts, nrm, col), (vp, vg), (vert, vcol, tri) = gpu_extractions(vol)
    rp, rn, rc = B.extract_point_cloud(blk)
    assert pts.shape == rp.shape, (pts.shape, rp.shape)
    assert same(pts, rp) and same(nrm, rn)
    assert (col is None and rc is None) or same(col, rc)
    rvp, rvg = B.extract_voxel_point_cloud(blk)
    assert same(vp, rvp) and same(vg, rvg)
    rv, rvc, rt, _ = B.extract_triangle_mesh(blk)
    assert vert.shape == rv.shape and tri.shape == rt.shape, (vert.shape, rv.shape, tri.shape, rt.shape)
    assert same(vert, rv) and np.array_equal(tri, rt) and tri.dtype == np.int32
    assert (vcol is None and rvc is None) or same(vcol, rvc)
    return len(rp), len(rvp), len(rv), len(rt)


# ---- the main grid ---------------------------------------------------------------------------------------------------------------
# 3 does not divide 80; 100 leaves only pixel (0, 0), which holds no depth in any ring image: those cases are the empty volume (one
# valid pixel alone is test_one_pixel_on_a_block_corner)
RES, STRIDES = (3, 8, 16, 32), (1, 3, 4, 100)
GRID = [(res, stride, (a + b) % 2 == 0, 1 if res == 32 else (1, 4, 9)[(a + b) % 3]) for a, res in enumerate(RES) for b, stride in enumerate(STRIDES)]


def t_vox(res):
    return 1.5 if res == 3 else 4.0


@functools.lru_cache(None)
def integrated(case):
    """(device volume after ONE integrate_frames call with the case's images, restatement after as many integrate steps)"""
    res, stride, color, count = case
    vol = gpu_frames(gpu_volume(res, t_vox(res), stride, color), images(count))
    return vol, ref_integrate(B.Blocks(VL, t_vox(res) * VL, res, stride, color), images(count))


@pytest.mark.parametrize("case", GRID, ids=lambda c: "R%d-s%d-%s-%dimg" % (c[0], c[1], "rgb" if c[2] else "nocolor", c[3]))
def test_integrate_grid(case):
    vol, blk = integrated(case)
    assert_units(vol, blk)
    if case[1] < 100:
        idx = blk.indices()
        assert (idx < 0).any() and (idx > 0).any() and len(idx) > 8


@pytest.mark.parametrize("case", GRID, ids=lambda c: "R%d-s%d-%s-%dimg" % (c[0], c[1], "rgb" if c[2] else "nocolor", c[3]))
def test_extract_grid(case):
    vol, blk = integrated(case)
    n_pts, n_vox, n_vert, n_tri = assert_extractions(vol, blk)
    if case[1] < 100:
        assert n_pts > 100 and n_vox > n_pts and n_vert > 100 and n_tri > 100


# ---- forms of one integration ----------------------------------------------------------------------------------------------------
def test_batch_equals_single_calls():
    """nine uint16 frames in one integrate_frames call (two launches: eight and one) against nine integrate() calls of float32 images"""
    a = gpu_frames(gpu_volume(16, 4.0, 4, True), images(9))
    b = gpu_single(gpu_volume(16, 4.0, 4, True), images(9))
    assert np.array_equal(a.volume_unit_indices(), b.volume_unit_indices()) and a.volume_unit_count() > 8
    (ta, ca), (tb, cb) = a.unit_arrays(), b.unit_arrays()
    assert same(ta, tb) and same(ca, cb)
    for x, y in zip(gpu_extractions(a), gpu_extractions(b)):
        for p, q in zip(x, y):
            assert same(p, q)


def test_float32_images_against_uint16_frames():
    ims = images(4)
    a = gpu_frames(gpu_volume(8, 4.0, 3, False), ims)
    b = gpu_single(gpu_volume(8, 4.0, 3, False), ims)
    blk = ref_integrate(B.Blocks(VL, 4.0 * VL, 8, 3, False), ims)
    assert_units(a, blk)
    assert_units(b, blk)


def test_second_frame_leaves_untouched_blocks_alone():
    """frame 0's cameras 0 and 1, then ONE image of frame 1 from camera 2: the existing blocks it does not touch keep their bits,
    the ones it touches and the new ones are the restatement's"""
    vol = gpu_frames(gpu_volume(8, 4.0, 4, True), images(2))
    blk = ref_integrate(B.Blocks(VL, 4.0 * VL, 8, 4, True), images(2))
    assert_units(vol, blk)
    before_idx, (before_tw, before_col) = vol.volume_unit_indices(), vol.unit_arrays()
    (d, c, E), = images(1, start=6)
    touched = set(B.touched(blk, f32(d), K4, W, H, E))
    existing = set(map(tuple, before_idx.tolist()))
    assert existing - touched and existing & touched and touched - existing
    gpu_frames(vol, [(d, c, E)])
    ref_integrate(blk, [(d, c, E)])
    assert_units(vol, blk)
    after_idx, (after_tw, after_col) = vol.volume_unit_indices(), vol.unit_arrays()
    where = {tuple(b): i for i, b in enumerate(after_idx.tolist())}
    for i, b in enumerate(map(tuple, before_idx.tolist())):
        if b not in touched:
            assert same(after_tw[where[b]], before_tw[i]) and same(after_col[where[b]], before_col[i])
    assert_extractions(vol, blk)


def test_all_zero_depth_image():
    vol = gpu_volume(16, 4.0, 4, True)
    vol.integrate(rgbd(np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.uint8)), intrinsic(), np.eye(4))
    assert vol.volume_unit_count() == 0 and vol.volume_unit_indices().shape == (0, 3)
    assert vol.unit_arrays()[0].shape == (0, 16 ** 3, 2)
    pc, vc, m = vol.extract_point_cloud(), vol.extract_voxel_point_cloud(), vol.extract_triangle_mesh()
    assert pc._pts.shape == (0, 3) and vc._pts.shape == (0, 3) and m._vert.shape == (0, 3) and m._tri.shape == (0, 3)


@pytest.mark.parametrize("t_blocks,expect", [(0.5, 8), (1.0, 27)])
def test_one_pixel_on_a_block_corner(t_blocks, expect):
    """the principal pixel (36, 40) at depth 4 ul with the identity pose: the world point (0, 0, 4 ul) is a block corner.  With
    sdf_trunc = ul / 2 the box is [-1, 0]^2 x [3, 4]; with sdf_trunc = ul it is [-1, 1]^2 x [3, 5]."""
    res, ul = 8, 8 * VL
    depth = np.zeros((H, W), np.float32)
    depth[36, 40] = 4 * ul
    vol = gpu_volume(res, t_blocks * res, 4, False)
    vol.integrate(rgbd(depth, np.zeros((H, W, 3), np.uint8)), intrinsic(), np.eye(4))
    blk = B.Blocks(VL, t_blocks * ul, res, 4, False)
    want = B.integrate(blk, depth, None, K4, W, H, np.eye(4))
    lo, hi = (-1, 0) if expect == 8 else (-1, 1)
    box = sorted((x, y, z) for x in range(lo, hi + 1) for y in range(lo, hi + 1) for z in range(3, 3 + hi - lo + 1))
    assert want == box and len(box) == expect
    assert_units(vol, blk)
    assert_extractions(vol, blk)


def test_sdf_trunc_equal_to_the_unit_length():
    ims = images(4)
    vol = gpu_frames(gpu_volume(4, 4.0, 4, True), ims)
    blk = ref_integrate(B.Blocks(VL, 4.0 * VL, 4, 4, True), ims)
    assert blk.trunc == blk.ul
    assert_units(vol, blk)
    assert_extractions(vol, blk)


def test_pool_growth():
    """a pool that starts with room for one block and doubles its way up holds the same bits as one that never grew"""
    small, large = gpu_volume(8, 4.0, 4, True, _capacity=1), gpu_volume(8, 4.0, 4, True, _capacity=4096)
    for v in (small, large):
        gpu_frames(v, images(9))
        gpu_single(v, images(2, start=1))
    assert small._pool.shape[0] < 4096 and large._pool.shape[0] == 4096 and small.volume_unit_count() > 64
    assert np.array_equal(small.volume_unit_indices(), large.volume_unit_indices())
    (ta, ca), (tb, cb) = small.unit_arrays(), large.unit_arrays()
    assert same(ta, tb) and same(ca, cb)
    for x, y in zip(gpu_extractions(small), gpu_extractions(large)):
        for p, q in zip(x, y):
            assert same(p, q)


def test_reset_then_reuse():
    vol = gpu_frames(gpu_volume(16, 4.0, 4, True), images(4))
    assert vol.volume_unit_count() > 0
    vol.reset()
    assert vol.volume_unit_count() == 0 and vol.extract_point_cloud()._pts.shape == (0, 3)
    ims = images(2, start=2)
    gpu_frames(vol, ims)
    blk = ref_integrate(B.Blocks(VL, 4.0 * VL, 16, 4, True), ims)
    assert_units(vol, blk)
    assert_extractions(vol, blk)
    assert "ScalableTSDFVolume" in repr(vol)


def test_block_index_out_of_range_raises():
    vol = gpu_volume(1, 1.0, 4, False, vl=1e-4)
    (d, c, E), = images(1)
    with pytest.raises(RuntimeError, match="2\\^20"):
        vol.integrate(rgbd(f32(d), c), intrinsic(), E)


# ---- extraction across block seams -------------------------------------------------------------------------------------------------
SPHERE_VL = 1.0


@functools.lru_cache(None)
def sphere(removed=None):
    """tsdf_mesh_ref.sphere_volume over 16^3 voxels cut into 2 x 2 x 2 blocks of 8^3 with indices in {-1, 0}: the centre sits near the
    common corner, so the surface crosses faces, edges and the corner between blocks.  Colours vary voxel by voxel.  Where the
    surface passes within ~1e-3 voxels of a voxel centre, marching cubes leaves slivers whose float32 vertices can make two of them
    overlap (is_watertight then says no, for the uniform volume's mesh as well); this centre is one without such a sliver, which
    test_tsdf_blocks_cpu.py holds against the restatement of the mesh checks."""
    f, w = M.sphere_volume(16, 5.3, (8.29, 7.92, 8.04))
    col = (np.arange(16 ** 3 * 3, dtype=np.float32).reshape(-1, 3) * np.float32(0.37)) % np.float32(255.0)
    return B.from_dense(f, w, col, 16, SPHERE_VL, 8, (-1, -1, -1), None if removed is None else (lambda b: b != removed))


def upload(blk, order=None):
    from kinectpy_amd import o3d
    ns = o3d.pipelines.integration
    vol = ns.ScalableTSDFVolume(blk.vl, blk.trunc, ns.TSDFVolumeColorType.RGB8 if blk.color else ns.TSDFVolumeColorType.NoColor, blk.R, blk.stride)
    idx = blk.indices()
    tw, col = blk.arrays()
    order = np.arange(len(idx)) if order is None else order
    vol._set_units(idx[order], tw[order], None if col is None else col[order])
    return vol


def test_sphere_across_eight_blocks():
    from kinectpy_amd import ops
    blk = sphere()
    vol = upload(blk)
    assert_units(vol, blk)
    n_pts, _, n_vert, n_tri = assert_extractions(vol, blk)
    assert n_pts > 300 and n_vert > 300
    m = vol.extract_triangle_mesh()
    assert ops.mesh_is_watertight(m._vert, m._tri), "duplicate or missing seam vertices"
    assert m.euler_poincare_characteristic() == 2
    assert n_tri == 2 * n_vert - 4


def test_sphere_with_one_block_removed():
    gone = (0, -1, 0)
    blk = sphere(gone)
    assert len(blk.units) == 7
    vol = upload(blk)
    assert_extractions(vol, blk)
    # no triangle from a cube that has a corner in the absent block: every vertex's lower voxel and its upper end lie in the blocks
    # that are there, and every cube of the full sphere that touches the absent block has lost its triangles
    full = sphere()
    _, _, ft, fk = B.extract_triangle_mesh(full)
    vert, _, tri, keys = B.extract_triangle_mesh(blk)
    assert len(tri) < len(ft) and not (keys[:, :3] == np.asarray(gone)).all(1).any()
    g = keys[:, :3] * 8 + np.stack([keys[:, 3] // 64, (keys[:, 3] // 8) % 8, keys[:, 3] % 8], 1)
    g[np.arange(len(g)), keys[:, 4]] += 1
    assert not ((g // 8) == np.asarray(gone)).all(1).any()
    m = vol.extract_triangle_mesh()
    assert m._tri.shape[0] == len(tri) and m.euler_poincare_characteristic() != 2          # the sphere is open now


def test_sphere_blocks_uploaded_in_shuffled_order():
    blk = sphere()
    a = upload(blk)
    b = upload(blk, np.random.default_rng(5).permutation(8))
    assert np.array_equal(a.volume_unit_indices(), b.volume_unit_indices())
    for x, y in zip(gpu_extractions(a), gpu_extractions(b)):
        for p, q in zip(x, y):
            assert same(p, q)


@functools.lru_cache(None)
def small_sphere(unit_resolution, removed=None):
    """a sphere of radius 2.1 voxels in 6^3 voxels cut into blocks of 1^3 (216, from (-3, -3, -3)) or 2^3 (27, from (-1, -1, -1)): the
    unit resolutions below the ring's.  At R = 1 every neighbour is another block, and a normal's tap reaches two blocks away: the only
    input on which the view looks a block up by its key and not in the 27-neighbour table."""
    f, w = M.sphere_volume(6, 2.1, (3.29, 2.92, 3.04))
    col = (np.arange(6 ** 3 * 3, dtype=np.float32).reshape(-1, 3) * np.float32(0.37)) % np.float32(255.0)
    first = {1: (-3, -3, -3), 2: (-1, -1, -1)}[unit_resolution]
    return B.from_dense(f, w, col, 6, SPHERE_VL, unit_resolution, first, None if removed is None else (lambda b: b != removed))


# The removed block is one the surface passes through: at R = 1 voxel (3, 2, 4) of the 6^3, inside the sphere with its +z neighbour
# outside; at R = 2 the corner block of voxels 4..5 on every axis.  (The block round the centre, (0, 0, 0) at R = 2, holds no voxel of
# the band: without it the restatement loses triangles and no point.)  The counts are the restatement's.
@pytest.mark.parametrize("unit_resolution,gone,left", [(1, (0, -1, 1), (81, 81, 148)), (2, (1, 1, 1), (80, 80, 149))], ids=["R1", "R2"])
def test_small_sphere_at_unit_resolutions_one_and_two(unit_resolution, gone, left):
    whole = small_sphere(unit_resolution)
    assert len(whole.units) == (6 // unit_resolution) ** 3
    vol = upload(whole)
    assert_units(vol, whole)
    assert assert_extractions(vol, whole) == (82, 116, 82, 160)
    holed = small_sphere(unit_resolution, gone)
    assert len(holed.units) == len(whole.units) - 1
    n_pts, _, n_vert, n_tri = assert_extractions(upload(holed), holed)
    assert (n_pts, n_vert, n_tri) == left and 0 < n_pts < 82


# ---- fuse_depth_tsdf ---------------------------------------------------------------------------------------------------------------
def test_fuse_depth_tsdf_scalable_and_default():
    from kinectpy_amd import o3d
    from kinectpy_amd.preprocessing.fusion import fuse_depth_tsdf
    from kinectpy_amd.utils import synth
    depth, rgb, extr = ring()
    poses =[synth.camera_pose(g, 4) for g in range(4)]
    to_master = [np.linalg.inv(poses[0]) @ poses[g] for g in range(1, 4)]
    ns = o3d.pipelines.integration
    E = np.stack([np.eye(4)] + [np.linalg.inv(T) for T in to_master])
    k = intrinsic()
    for mesh in (False, True):
        got = fuse_depth_tsdf(depth[0], rgb[0], k, to_master, 2000.0, 64, (0.0, 0.0, 0.0), None, SCALE, TRUNC, mesh=mesh, scalable=True,
                              volume_unit_resolution=8, depth_sampling_stride=3)
        vol = ns.ScalableTSDFVolume(2000.0 / 64, 4.0 * 2000.0 / 64, ns.TSDFVolumeColorType.RGB8, 8, 3)
        vol.integrate_frames(depth[0], rgb[0], k, E, SCALE, TRUNC)
        if mesh:
            want = vol.extract_triangle_mesh().compute_vertex_normals()
            assert same(got._vert.cpu().numpy(), want._vert.cpu().numpy()) and np.array_equal(got._tri.cpu().numpy(), want._tri.cpu().numpy())
            assert same(got._vnrm.cpu().numpy(), want._vnrm.cpu().numpy()) and got._tri.shape[0] > 100
        else:
            want = vol.extract_point_cloud()
            assert same(got._pts.cpu().numpy(), want._pts.cpu().numpy()) and same(got._nrm.cpu().numpy(), want._nrm.cpu().numpy())
            assert same(got._col.cpu().numpy(), want._col.cpu().numpy()) and got._pts.shape[0] > 100
    # the default path is the uniform volume's, as before
    origin = (-1000.0, -1100.0, 0.0)
    got = fuse_depth_tsdf(depth[0], rgb[0], k, to_master, 2000.0, 64, origin, None, SCALE, TRUNC)
    uni = ns.UniformTSDFVolume(2000.0, 64, 4.0 * 2000.0 / 64, ns.TSDFVolumeColorType.RGB8, origin)
    uni.integrate_frames(depth[0], rgb[0], k, E, SCALE, TRUNC)
    want = uni.extract_point_cloud()
    assert same(got._pts.cpu().numpy(), want._pts.cpu().numpy()) and same(got._nrm.cpu().numpy(), want._nrm.cpu().numpy())

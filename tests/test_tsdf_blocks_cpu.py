"""CPU suite of the block-sparse TSDF volume (AC16): the restatement tests/tsdf_blocks_ref.py against the dense restatements it is
built on, the public names and signatures of ScalableTSDFVolume, the argument errors that come before any device work, and the ABI."""
import inspect
import os
import re

import numpy as np
import pytest

import tsdf_blocks_ref as B
import tsdf_mesh_ref as M
import tsdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VL = 1.0


def sphere_blocks(keep=None, color=True):
    f, w = M.sphere_volume(16, 5.3, (8.29, 7.92, 8.04))
    col = (np.arange(16 ** 3 * 3, dtype=np.float32).reshape(-1, 3) * np.float32(0.37)) % np.float32(255.0) if color else None
    return B.from_dense(f, w, col, 16, VL, 8, (-1, -1, -1), keep), f, w, col


def assemble(blk):
    """the blocks in one dense array from the lowest block on, absent blocks at weight 0 -> (tsdf, weight, colours, res, origin)"""
    r = blk.R
    idx = blk.indices().astype(np.int64)
    lo = idx.min(0)
    n = int((idx.max(0) - lo).max()) + 1
    res = n * r
    f, w = np.zeros((res,) * 3, np.float32), np.zeros((res,) * 3, np.float32)
    c = np.zeros((res,) * 3 + (3,), np.float32) if blk.color else None
    for b in map(tuple, idx.tolist()):
        s = tuple(slice((b[k] - int(lo[k])) * r, (b[k] - int(lo[k]) + 1) * r) for k in range(3))
        u = blk.units[b]
        f[s], w[s] = u.tsdf.reshape(r, r, r), u.w.reshape(r, r, r)
        if c is not None:
            c[s] = u.col.reshape(r, r, r, 3)
    return f.reshape(-1), w.reshape(-1), None if c is None else c.reshape(-1, 3), res, lo.astype(np.float64) * blk.ul


def match(va, vb):
    """the permutation that sends the vertices va to the vertices vb: both sorted by their rounded position"""
    ka = np.lexsort(np.round(va.astype(np.float64) / (VL * 1e-3)).T[::-1])
    kb = np.lexsort(np.round(vb.astype(np.float64) / (VL * 1e-3)).T[::-1])
    to_b = np.empty(len(va), np.int64)
    to_b[ka] = kb
    return to_b


@pytest.mark.parametrize("gone", [None, (0, -1, 0), (-1, -1, -1)])
def test_block_mesh_agrees_with_the_dense_restatement(gone):
    blk, _, _, _ = sphere_blocks(None if gone is None else (lambda b: b != gone))
    vert, col, tri, keys = B.extract_triangle_mesh(blk)
    f, w, c, res, origin = assemble(blk)
    dv, dc, dt, _ = M.extract_triangle_mesh(f, w, c, res, VL, origin)
    assert len(vert) == len(dv) > 300 and len(tri) == len(dt) > 600
    to_dense = match(vert, dv)
    # positions to 1e-9 relative: the two add the centre up differently (b ul + (i + 0.5) vl against (x + 0.5) vl + origin)
    scale = np.abs(dv.astype(np.float64)).max()
    assert np.abs(vert.astype(np.float64) - dv[to_dense].astype(np.float64)).max() <= 1e-9 * scale + np.spacing(np.float32(scale))
    assert np.abs(col.astype(np.float64) - dc[to_dense].astype(np.float64)).max() <= 1e-6
    mine = np.sort(np.sort(to_dense[tri], 1).view([("", np.int64)] * 3).reshape(-1))
    theirs = np.sort(np.sort(dt.astype(np.int64), 1).view([("", np.int64)] * 3).reshape(-1))
    assert np.array_equal(mine, theirs)
    # same orientation, not only the same vertex sets: rotate every triangle to start at its smallest index
    rot = lambda t: np.stack([np.roll(r, -int(np.argmin(r))) for r in t])
    assert np.array_equal(np.sort(rot(to_dense[tri]).view([("", np.int64)] * 3).reshape(-1)),
                          np.sort(rot(dt.astype(np.int64)).view([("", np.int64)] * 3).reshape(-1)))
    # vertices ascend in their key
    assert keys.tolist() == sorted(keys.tolist())
    if gone is None:
        import mesh_checks_ref as C
        assert len(tri) == 2 * len(vert) - 4                      # closed, genus 0
        assert C.is_watertight(vert, tri) and C.euler_poincare_characteristic(len(vert), tri) == 2          # what the GPU suite asks of this sphere


def test_block_clouds_agree_with_the_dense_restatement():
    """away from the dense volume's excluded last layers the two extractions give the same points; the block form has no such layer"""
    blk, f, w, col = sphere_blocks()
    pts, nrm, pc = B.extract_point_cloud(blk)
    dense = R.Volume(16 * VL, 16, 8 * VL, (-8 * VL,) * 3, True)
    dense.tsdf[:], dense.w[:], dense.col[:] = f, w, col
    dp, dn, dc = R.extract_point_cloud(dense)
    assert len(pts) == len(dp) > 300                               # the sphere stays clear of the last layers
    o, d = np.lexsort(np.round(pts / (VL * 1e-3)).T[::-1]), np.lexsort(np.round(dp / (VL * 1e-3)).T[::-1])
    assert np.abs(pts[o].astype(np.float64) - dp[d]).max() <= 1e-6 * 8 * VL
    assert np.abs(nrm[o].astype(np.float64) - dn[d]).max() <= 1e-5 and np.abs(pc[o].astype(np.float64) - dc[d]).max() <= 1e-6
    vp, vg = B.extract_voxel_point_cloud(blk)
    dvp, dvg = R.extract_voxel_point_cloud(dense)
    o, d = np.lexsort(vp.T[::-1]), np.lexsort(dvp.T[::-1])
    assert np.array_equal(vp[o], dvp[d]) and np.array_equal(vg[o], dvg[d])


def test_a_block_equals_a_uniform_volume_with_the_images_that_touch_it():
    """AC16's consequence on one synthetic image pair: every block is tsdf_ref's uniform volume at origin b ul after the images whose
    touched set holds it, and an image leaves the blocks it does not touch alone"""
    W, H, K4 = 16, 12, (12.0, 12.0, 8.0, 6.0)
    rng = np.random.default_rng(3)
    depth = [(1.0 + 0.3 * rng.random((H, W))).astype(np.float32), (1.1 + 0.3 * rng.random((H, W))).astype(np.float32)]
    depth[0][:, :3] = 0.0
    shift = np.eye(4)
    shift[0, 3] = 0.4
    extr = [np.eye(4), shift]
    blk = B.Blocks(0.05, 0.2, 4, 2, False)
    t0 = B.integrate(blk, depth[0], None, K4, W, H, extr[0])
    snapshot = blk.copy()
    t1 = B.integrate(blk, depth[1], None, K4, W, H, extr[1])
    assert set(t0) - set(t1) and set(t1) - set(t0) and set(t0) & set(t1)
    for b, u in blk.units.items():
        v = R.Volume(blk.ul, 4, 0.2, [k * blk.ul for k in b], False)
        v.vl = blk.vl
        for i, t in enumerate((t0, t1)):
            if b in t:
                R.integrate(v, depth[i], None, K4, W, H, extr[i])
        assert np.array_equal(u.tsdf, v.tsdf) and np.array_equal(u.w, v.w)
        if b not in t1:
            assert np.array_equal(u.tsdf, snapshot.units[b].tsdf) and np.array_equal(u.w, snapshot.units[b].w)


def test_touched_box_of_a_point_on_a_block_corner():
    W, H, K4 = 16, 12, (12.0, 12.0, 8.0, 6.0)
    depth = np.zeros((H, W), np.float32)
    depth[6, 8] = 2.0                                             # the principal pixel: the world point (0, 0, 2) = corner of block (0, 0, 4)
    half = B.Blocks(0.0625, 0.25, 8, 2, False)                    # ul = 0.5, trunc = ul / 2
    assert B.touched(half, depth, K4, W, H, np.eye(4)) == sorted((x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (3, 4))
    full = B.Blocks(0.0625, 0.5, 8, 2, False)                     # trunc = ul: three blocks per axis
    assert B.touched(full, depth, K4, W, H, np.eye(4)) == sorted((x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (3, 4, 5))
    assert B.touched(B.Blocks(0.0625, 0.25, 8, 5, False), depth, K4, W, H, np.eye(4)) == []          # stride 5 misses pixel (6, 8)
    far = B.Blocks(1e-7, 1e-7, 1, 2, False)
    with pytest.raises(OverflowError):
        B.touched(far, depth, K4, W, H, np.eye(4))


# ---- the public names ---------------------------------------------------------------------------------------------------------------
def test_scalable_volume_is_a_class_with_open3d_members():
    from kinectpy_amd import integration, o3d
    cls = o3d.pipelines.integration.ScalableTSDFVolume
    assert cls is integration.ScalableTSDFVolume and inspect.isclass(cls)
    for name in ("integrate", "integrate_frames", "extract_point_cloud", "extract_voxel_point_cloud", "extract_triangle_mesh", "reset", "volume_unit_count",
                 "volume_unit_indices", "unit_arrays", "_set_units"):
        assert callable(getattr(cls, name)), name
    assert "__repr__" in vars(cls)
    p = inspect.signature(cls.__init__).parameters
    assert list(p)[1:6] == ["voxel_length", "sdf_trunc", "color_type", "volume_unit_resolution", "depth_sampling_stride"]
    assert p["volume_unit_resolution"].default == 16 and p["depth_sampling_stride"].default == 4
    p = inspect.signature(cls.integrate_frames).parameters
    assert list(p)[1:] == ["depths", "colors", "intrinsic", "extrinsics", "depth_scale", "depth_trunc"]
    assert p["depth_scale"].default == 1000.0 and p["depth_trunc"].default == 3.0
    from kinectpy_amd.preprocessing.fusion import fuse_depth_tsdf
    p = inspect.signature(fuse_depth_tsdf).parameters
    assert p["scalable"].default is False and p["volume_unit_resolution"].default == 16 and p["depth_sampling_stride"].default == 4


def test_argument_errors_come_before_any_device_work():
    from kinectpy_amd import integration, o3d
    ns = o3d.pipelines.integration
    rgb = ns.TSDFVolumeColorType.RGB8
    with pytest.raises(NotImplementedError, match="Gray32"):
        ns.ScalableTSDFVolume(0.01, 0.04, ns.TSDFVolumeColorType.Gray32)
    for args in ((0.01, 0.04, rgb, 0), (0.01, 0.04, rgb, 33), (0.01, 0.04, rgb, 16, 0), (0.0, 0.04, rgb), (-1.0, 0.04, rgb), (0.01, 0.0, rgb),
                 (0.01, 0.17, rgb), (0.01, 0.09, rgb, 8)):
        with pytest.raises(RuntimeError) as e:
            ns.ScalableTSDFVolume(*args)
        assert not isinstance(e.value, NotImplementedError), args
    # the image checks need no device either: a shell is enough
    k = o3d.camera.PinholeCameraIntrinsic(5, 6, 4.0, 4.0, 2.5, 3.0)
    for col_vol, color, depth in ((None, np.zeros((6, 5, 3), np.uint8), np.zeros((6, 5), np.uint16)),
                                  (None, np.zeros((6, 5, 3), np.uint8), np.zeros((5, 6), np.float32)),
                                  (None, np.zeros((5, 5, 3), np.uint8), np.zeros((6, 5), np.float32)),
                                  (object(), np.zeros((6, 5), np.float32), np.zeros((6, 5), np.float32))):
        shell = object.__new__(integration.ScalableTSDFVolume)
        shell._col = col_vol
        with pytest.raises(RuntimeError, match=r"\[ScalableTSDFVolume::Integrate\] Unsupported image format\."):
            shell.integrate(o3d.geometry.RGBDImage(color, depth), k, np.eye(4))


NAMES = ("kpx_tsdf_blocks_touch_workspace_bytes", "kpx_tsdf_blocks_touch", "kpx_tsdf_blocks_insert", "kpx_tsdf_blocks_integrate",
         "kpx_tsdf_blocks_extract_workspace_bytes", "kpx_tsdf_blocks_extract_count", "kpx_tsdf_blocks_extract_fill", "kpx_tsdf_blocks_mesh_count",
         "kpx_tsdf_blocks_mesh_fill")


def test_header_declares_and_library_exports_the_entry_points():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    header = open(os.path.join(ROOT, "include", "kinectpx.h")).read()
    for name in NAMES:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES, name
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    # host-side answers that need no device
    assert lib.kpx_tsdf_blocks_extract_workspace_bytes(10, 0, 0) == 0 and lib.kpx_tsdf_blocks_extract_workspace_bytes(10, 33, 1) == 0
    assert lib.kpx_tsdf_blocks_extract_workspace_bytes(-1, 16, 0) == 0
    cloud, mesh = lib.kpx_tsdf_blocks_extract_workspace_bytes(1000, 16, 0), lib.kpx_tsdf_blocks_extract_workspace_bytes(1000, 16, 1)
    assert 1000 * 27 * 4 <= cloud < mesh < 1000 * 16 ** 3 * 2 + 1000 * 27 * 4 + 4096
    assert lib.kpx_tsdf_blocks_touch_workspace_bytes(0, 80, 72, 4, 1.0, 0.5) == 0                # no image
    assert lib.kpx_tsdf_blocks_touch_workspace_bytes(9, 80, 72, 4, 1.0, 0.5) == 0                # more than a launch holds
    assert lib.kpx_tsdf_blocks_touch_workspace_bytes(1, 80, 72, 0, 1.0, 0.5) == 0                # stride
    assert lib.kpx_tsdf_blocks_touch_workspace_bytes(1, 80, 72, 4, 1.0, 1.5) == 0                # sdf_trunc above the unit length
    assert lib.kpx_tsdf_blocks_extract_count(None, None, 1, None, 40, 0, None, None, 0, None) == -1 and b"unit resolution" in lib.kpx_last_error()
    assert lib.kpx_tsdf_blocks_mesh_count(None, None, 1, None, 16, None, None, 0, None) == -1 and b"null pointer" in lib.kpx_last_error()
    assert lib.kpx_tsdf_blocks_mesh_fill(None, None, 1, None, None, 16, 1.0, 1 << 31, 1, None, None, None, None, 0, None) == -3

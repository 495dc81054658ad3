"""GPU suite of the lens undistortion (AC22): kpx_undistort_map, kpx_remap_u8 and kpx_remap_depth against the float64
restatement tests/undistort_ref.py, bit for bit; buffer discipline of the packed and the 8-byte stores; the rig end to end into
fuse_depth_tsdf."""
import functools

import numpy as np
import pytest

from tests import sensor_ref as R
from tests import undistort_ref as U
from tests.test_sensor_gpu import toy_sensor

SW, SH = 31, 17                # the source image of the remap cases: an odd row length in bytes for 1 and for 3 channels (and in u16)
OW, OH = 41, 27                # their output: 1107 pixels, one block and a bit, no multiple of 4
BORDERS = ("outside_left", "outside_right", "outside_top", "outside_bottom")
MID_GAP = 100.0


def _same_f32(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern"
    bad = np.nonzero(got.view(np.int32)[~nan] != want.view(np.int32)[~nan])[0]
    assert bad.size == 0, f"{bad.size} finite values differ in their bits, first at {bad[:5]}: {got[~nan][bad[:5]]} vs {want[~nan][bad[:5]]}"


def _same(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {want.size} elements differ, first {bad[:5].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def ref_map(cam, target):
    return U.undistort_map(R.cam_of(cam), U.pinhole_of(target), target.width, target.height)


# ---- the map --------------------------------------------------------------------------------------------------------------------------
def _map_cases():
    """name -> (lens, target).  The sized cases: the synthetic depth lens on a small image, the target its fit="same" camera at the
    output size; "toy": the 24 x 20 toy depth lens and a target of 0.6 times its focal lengths, which looks beyond the metric radius"""
    from kinectpy_amd.calibration import CameraIntrinsics
    from kinectpy_amd.utils import synth
    d = synth.sensor_calibration(0).depth.to_dict()
    cases = {}
    for w, h in ((1, 1), (9, 7), (13, 5), (257, 1), (41, 25)):
        lens = CameraIntrinsics(**dict(d, width=w, height=h, cx=0.4 * w, cy=0.6 * h, fx=0.8 * max(w, h, 8), fy=0.81 * max(w, h, 8)))
        cases[f"{w}x{h}"] = (lens, lens.undistorted())
    toy = toy_sensor(0).depth
    cases["toy"] = (toy, CameraIntrinsics(toy.width, toy.height, 0.6 * toy.fx, 0.6 * toy.fy, toy.cx, toy.cy))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1", "9x7", "13x5", "257x1", "41x25", "toy"])
def test_undistort_map_is_the_restatement_bit_for_bit(name):
    from kinectpy_amd import ops
    lens, target = _map_cases()[name]
    want = ref_map(lens, target)
    nan = np.isnan(want[..., 0])
    assert np.array_equal(nan, np.isnan(want[..., 1])) and (~nan).any()
    if name == "toy":
        x0, y0 = np.floor(want[..., 0].astype(np.float64)), np.floor(want[..., 1].astype(np.float64))
        inside = ~nan & (x0 >= 0) & (x0 <= lens.width - 2) & (y0 >= 0) & (y0 <= lens.height - 2)
        assert 0.2 < nan.mean() < 0.35 and 0.6 < inside.mean() < 0.75 and (~nan & ~inside).any()        # every class: 27 % NaN, 69 % inside
    got = ops.undistort_map(lens, target)
    assert tuple(got.shape) == (target.height, target.width, 2) and got.dtype.is_floating_point
    _same_f32(got.cpu().numpy(), want)
    if name == "toy":                                        # the cached map of the camera object, and an o3d pinhole as the target
        assert lens.undistort_map(target) is lens.undistort_map(target)
        _same_f32(lens.undistort_map(target).cpu().numpy(), want)
        _same_f32(ops.undistort_map(lens, target.to_pinhole()).cpu().numpy(), want)


# ---- the remaps -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def remap_maps(M):
    """f32 (M, OH, OW, 2) restatement maps into the SW x SH source image: a lens that has a ray at every source pixel, and targets of a
    shorter focal length with shifted principal points -- they look past the image on all four sides and, in their corners, past the
    metric radius"""
    from kinectpy_amd.calibration import CameraIntrinsics
    maps = []
    for i in range(M):
        s = float(i)
        lens = CameraIntrinsics(SW, SH, 20.0 + 0.7 * s, 19.5 + 0.4 * s, 15.3 - 0.6 * s, 8.2 + 0.5 * s, k1=4.9 + 0.1 * s, k2=3.1, k3=0.17, k4=5.23 + 0.1 * s, k5=4.7,
                                k6=0.88, p1=7e-4, p2=-4e-4)
        target = CameraIntrinsics(OW, OH, 12.0 + 0.5 * s, 10.0 + 0.3 * s, 20.9 - 1.3 * s, 12.6 + 1.1 * s)
        maps.append(ref_map(lens, target))
    maps = np.stack(maps)
    maps.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def u8_case(F, M, C, interpolation):
    rng = np.random.default_rng(100 * F + 10 * M + C)
    src = rng.integers(1, 256, size=(F, SH, SW, C), dtype=np.uint8)
    want, cls = U.remap_u8(src, remap_maps(M), interpolation)
    for a in (src, want):
        a.setflags(write=False)
    return src, want, cls


@functools.lru_cache(maxsize=None)
def depth_case(F, M, interpolation, gap):
    """plateaus (a 2 x 2 block of equal values survives max_gap_mm = 0), a noisy band, steps of 1500 mm below row 9 and of 700 mm right
    of column 16, 10 % zeros"""
    rng = np.random.default_rng(7 + 100 * F + M)
    src = np.full((F, SH, SW), 1000, np.int64)
    src[:, :, 8:14] += rng.integers(-20, 21, size=(F, SH, 6))
    src[:, 9:, :] += 1500
    src[:, :, 16:] += 700
    src[rng.random(src.shape) < 0.1] = 0
    src = src.astype(np.uint16)
    want, cls = U.remap_depth(src, remap_maps(M), interpolation, gap)
    for a in (src, want):
        a.setflags(write=False)
    return src, want, cls


def assert_classes(cls, names):
    for k in names:
        assert cls[k].any(), f"no pixel of class {k} in the test data"


@pytest.mark.gpu
@pytest.mark.parametrize("C, interpolation", [(3, "bilinear"), (3, "nearest"), (1, "bilinear"), (1, "nearest")])
@pytest.mark.parametrize("F, M", [(1, 1), (3, 1), (3, 3), (6, 3)])
def test_remap_u8_is_the_restatement_bit_for_bit(F, M, C, interpolation):
    from kinectpy_amd import ops
    src, want, cls = u8_case(F, M, C, interpolation)
    assert_classes(cls, ("nan_map", "sampled") + BORDERS)
    assert (want[cls["sampled"]] != 0).any() and not want[~cls["sampled"]].any()
    got = ops.remap(src, remap_maps(M) if M > 1 else remap_maps(1)[0], interpolation)
    assert tuple(got.shape) == (F, OH, OW, C)
    _same(got, want)
    if C == 1:                                               # a (F, H, W) mask stack comes back as (F, H', W')
        flat = ops.remap(src[..., 0], remap_maps(M), interpolation)
        assert tuple(flat.shape) == (F, OH, OW)
        _same(flat, want[..., 0])


@pytest.mark.gpu
@pytest.mark.parametrize("interpolation, gap", [("nearest", None), ("bilinear", 0.0), ("bilinear", MID_GAP), ("bilinear", float("inf"))])
@pytest.mark.parametrize("F, M", [(1, 1), (6, 3)])
def test_remap_depth_is_the_restatement_bit_for_bit(F, M, interpolation, gap):
    from kinectpy_amd import ops
    src, want, cls = depth_case(F, M, interpolation, gap)
    assert_classes(cls, ("nan_map", "sampled") + BORDERS)
    if interpolation == "bilinear":
        assert_classes(cls, ("zero_neighbour",) + (("gap",) if gap != float("inf") else ()))
        assert not cls["gap"].any() or gap != float("inf")
    else:
        assert (want[cls["sampled"]] == 0).any()             # a zero copied as a zero
    assert (want[cls["sampled"]] != 0).any() and not want[~cls["sampled"]].any()
    got = ops.remap_depth(src, remap_maps(M), interpolation, gap)
    assert tuple(got.shape) == (F, OH, OW)
    _same(got, want)


def test_the_three_gaps_differ_where_they_should():
    """(on the restatement's outputs the device is compared with: no device here) 0 keeps only plateaus, the mid value drops the step,
    +inf blends across it"""
    zero, mid, inf = (depth_case(6, 3, "bilinear", g) for g in (0.0, MID_GAP, float("inf")))
    assert zero[2]["sampled"].sum() < mid[2]["sampled"].sum() < inf[2]["sampled"].sum()
    across = inf[2]["sampled"] & mid[2]["gap"]
    assert across.sum() > 20 and (np.abs(inf[1][across].astype(np.int64)[:, None] - [1000, 1700, 2500, 3200]).min(1) > 20).any()


@pytest.mark.gpu
def test_vector_paths_of_an_output_that_is_a_multiple_of_four():
    """40 x 27 = 1080 pixels: the 16-byte map loads and the 8-byte depth stores run (the 41 x 27 cases take the element paths)"""
    from kinectpy_amd import ops
    maps = np.ascontiguousarray(remap_maps(3)[:, :, :40])
    src, _, _ = u8_case(6, 3, 3, "bilinear")
    want, cls = U.remap_u8(src, maps, "bilinear")
    assert_classes(cls, ("nan_map", "sampled"))
    _same(ops.remap(src, maps, "bilinear"), want)
    dsrc, _, _ = depth_case(6, 3, "bilinear", MID_GAP)
    for interpolation in ("nearest", "bilinear"):
        want, cls = U.remap_depth(dsrc, maps, interpolation, MID_GAP)
        assert_classes(cls, ("nan_map", "sampled"))
        _same(ops.remap_depth(dsrc, maps, interpolation, MID_GAP), want)


@pytest.mark.gpu
def test_an_empty_source_gives_zeros_fully_written():
    import torch
    from kinectpy_amd import ops, _lib
    dev = _lib.device()
    maps = remap_maps(1)
    out = torch.full((2, OH, OW, 3), 0xA5, dtype=torch.uint8, device=dev)
    got = ops.remap(torch.zeros((2, 0, SW, 3), dtype=torch.uint8, device=dev), maps, "bilinear", out=out)
    assert got.data_ptr() == out.data_ptr() and not got.cpu().numpy().any()
    out = torch.full((2, OH, OW), -1, dtype=torch.int16, device=dev).view(torch.uint16)
    got = ops.remap_depth(torch.zeros((2, SH, 0), dtype=torch.int16, device=dev).view(torch.uint16), maps, "nearest", out=out)
    assert got.data_ptr() == out.data_ptr() and not got.cpu().numpy().any()


@pytest.mark.gpu
def test_buffer_discipline_bases_off_by_one_element_guards_and_poisoned_outputs():
    """every input and every output starts one element into its buffer (off every boundary beyond its element size); each output lies
    between guard bands and is pre-filled, under two fills: a byte the kernel skipped cannot hold the right value under both.  None of
    the three entries takes device scratch."""
    import torch
    import scratch_harness as H
    from kinectpy_amd import ops, _lib
    dev = _lib.device()
    F, M, guard = 3, 3, 4096

    def off_by_one(a, dtype):
        t = torch.as_tensor(np.ascontiguousarray(a).reshape(-1).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a).reshape(-1))
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
        buf[1:].copy_(t.to(dev))
        v = buf[1:].view(dtype) if dtype != t.dtype else buf[1:]
        return v.view(*a.shape)

    maps = off_by_one(remap_maps(M), torch.float32)
    assert maps.data_ptr() % 16 == 4

    def run(call, want, np_dtype):
        n = want.size
        tdtype = torch.uint8 if np_dtype == np.uint8 else torch.int16
        for fill in (0xA5, 0x5A):
            poison = 0xA5 if np_dtype == np.uint8 else 0xA5A5 - 0x10000
            inner = fill if np_dtype == np.uint8 else (fill * 0x101 if fill * 0x101 < 0x8000 else fill * 0x101 - 0x10000)
            raw = torch.full((guard + 1 + n + guard,), poison, dtype=tdtype, device=dev)
            raw[guard + 1:guard + 1 + n].fill_(inner)
            buf = raw if np_dtype == np.uint8 else raw.view(torch.uint16)
            out = buf[guard + 1:guard + 1 + n]
            assert out.data_ptr() % 16 == (1 if np_dtype == np.uint8 else 2)
            with H.scratch(0xFF, exact=True) as s:
                ret = call(out)
            assert s.handouts == 0 and ret.data_ptr() == out.data_ptr()
            host = buf.cpu().numpy()
            canary = 0xA5 if np_dtype == np.uint8 else 0xA5A5
            assert (host[:guard + 1] == canary).all() and (host[guard + 1 + n:] == canary).all(), f"guard damaged, fill {fill:#x}"
            got = host[guard + 1:guard + 1 + n].reshape(want.shape)
            assert np.array_equal(got, want), f"fill {fill:#x}: {(got != want).sum()} elements differ"

    for C, interpolation in ((3, "bilinear"), (1, "nearest")):
        src, want, _ = u8_case(F, M, C, interpolation)
        d_src = off_by_one(src, torch.uint8)
        run(lambda out: ops.remap(d_src, maps, interpolation, out=out), want, np.uint8)
    for interpolation in ("nearest", "bilinear"):
        src, want, _ = depth_case(F, M, interpolation, MID_GAP)
        d_src = off_by_one(src, torch.uint16)
        assert d_src.data_ptr() % 16 == 2
        run(lambda out: ops.remap_depth(d_src, maps, interpolation, MID_GAP, out=out), want, np.uint16)
    with H.scratch(0xFF, exact=True) as s:
        lens, target = _map_cases()["toy"]
        ops.undistort_map(lens, target)
    assert s.handouts == 0


# ---- cameras and the rig, end to end --------------------------------------------------------------------------------------------------
def small_rig(scale=8):
    """the four synthetic sensors on images 1 / scale the size (80 x 72 depth, 160 x 90 colour)"""
    from kinectpy_amd.calibration import CameraIntrinsics, SensorCalibration, SensorRig
    from kinectpy_amd.utils import synth

    def small(cam):
        d = cam.to_dict()
        return CameraIntrinsics(**dict(d, width=d["width"] // scale, height=d["height"] // scale, fx=d["fx"] / scale, fy=d["fy"] / scale, cx=d["cx"] / scale,
                                       cy=d["cy"] / scale))
    cals = [synth.sensor_calibration(i) for i in range(4)]
    return SensorRig([SensorCalibration(small(c.depth), small(c.color), c.depth_to_color) for c in cals])


@pytest.mark.gpu
def test_tilted_plane_through_the_device_stays_inside_its_source_block():
    from tests.test_undistort_cpu import assert_plane_bracket, plane_scene, reduced
    from kinectpy_amd.calibration import SensorCalibration
    cam = reduced(2)
    cal = SensorCalibration(cam, cam, np.eye(4))
    z, img = plane_scene(cam)
    target = cam.undistorted("inside")
    m = ref_map(cam, target)
    for interpolation, gap in (("nearest", None), ("bilinear", 50.0)):
        got = cal.undistort_depth(img, interpolation, gap, pinhole=target)
        assert tuple(got.shape) == (target.height, target.width)
        _same(got, U.remap_depth(img[None], m, interpolation, gap)[0][0])
        assert assert_plane_bracket(got.cpu().numpy(), m, z) >= 0.9
    # the default target is the fit="same" camera, a flat (H * W,) image is accepted
    m = ref_map(cam, cam.undistorted())
    _same(cal.undistort_depth(img.reshape(-1)), U.remap_depth(img[None], m, "nearest")[0][0])


@pytest.mark.gpu
def test_sensor_methods_undistort_colour_and_masks():
    rig = small_rig()
    cal = rig.calibrations[1]
    rng = np.random.default_rng(9)
    color = rng.integers(1, 256, size=(cal.color.height, cal.color.width, 3), dtype=np.uint8)
    target = cal.color.undistorted("inside")
    m = ref_map(cal.color, target)
    want, cls = U.remap_u8(color[None], m, "bilinear")
    assert cls["sampled"].all()
    got = cal.undistort_color(color, pinhole=target)
    assert tuple(got.shape) == (target.height, target.width, 3)
    _same(got, want[0])
    mask = (color[..., 0] > 128).astype(np.uint8) * 255
    got = cal.undistort_mask(mask, pinhole=target)
    _same(got, U.remap_u8(mask[None, ..., None], m, "nearest")[0][0, ..., 0])
    assert set(np.unique(got.cpu().numpy())) == {0, 255}
    dmask = (rng.random((cal.depth.height, cal.depth.width)) < 0.5).astype(np.uint8)
    got = cal.undistort_mask(dmask, camera="depth")
    _same(got, U.remap_u8(dmask[None, ..., None], ref_map(cal.depth, cal.depth.undistorted()), "nearest")[0][0, ..., 0])
    und = cal.undistorted("inside")
    assert und.color == target and und.color.to_pinhole().is_valid()


@pytest.mark.gpu
def test_rig_undistorts_a_batch_in_one_call_and_feeds_the_tsdf_fusion():
    from kinectpy_amd.preprocessing.fusion import fuse_depth_tsdf, remove_free_space_points
    from kinectpy_amd.utils import synth
    rig = small_rig()
    S = len(rig)
    _, depth, rgb, _, truth = synth.sensor_ring(4, xy=synth.small_xy(8))
    depth, rgb = depth[0], rgb[0]                            # (4, 72 * 80), (4, 72 * 80, 3): the frames as the lenses took them
    common = rig.common_pinhole()
    maps = np.stack([ref_map(c.depth, common) for c in rig.calibrations])
    want, cls = U.remap_depth(depth.reshape(S, 72, 80), maps, "nearest")
    assert cls["sampled"].all() and (want != 0).mean() > 0.5
    batch = rig.undistort_depths(depth)
    assert tuple(batch.shape) == (S, 72, 80) and rig.undistort_maps() is rig.undistort_maps()
    _same_f32(rig.undistort_maps().cpu().numpy(), maps)
    _same(batch, want)
    for s, cal in enumerate(rig.calibrations):               # one call for the batch = one call per sensor
        _same(cal.undistort_depth(depth[s], pinhole=common), want[s])
    two = rig.undistort_depths(np.concatenate([depth, depth[::-1]]))          # frame f of sensor f % S
    _same(two[:S], want)
    _same(two[S:], U.remap_depth(depth[::-1].reshape(S, 72, 80), maps, "nearest")[0])
    want_rgb, _ = U.remap_u8(rgb.reshape(S, 72, 80, 3), maps, "nearest")
    pre_rgb = rig.undistort_colors(rgb, camera="depth", interpolation="nearest")
    _same(pre_rgb, want_rgb)
    masks = (rgb[..., 0] > 0).astype(np.uint8).reshape(S, 72, 80)
    _same(rig.undistort_masks(masks, camera="depth"), U.remap_u8(masks[..., None], maps, "nearest")[0][..., 0])
    # the fusion with the rig = the fusion of the pre-undistorted frames with the common pinhole camera
    origin = (-1000.0, -1100.0, 1500.0)
    pin = common.to_pinhole()
    got = fuse_depth_tsdf(depth, rgb, None, truth, 2000.0, 32, origin, rig=rig)
    ref = fuse_depth_tsdf(batch.reshape(S, -1), pre_rgb.reshape(S, -1, 3), pin, truth, 2000.0, 32, origin)
    assert len(ref._pts) > 300
    for a, b in ((got._pts, ref._pts), (got._nrm, ref._nrm), (got._col, ref._col)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    plain = fuse_depth_tsdf(depth, rgb, pin, truth, 2000.0, 32, origin)      # the distorted frames passed through: another cloud
    assert len(plain._pts) != len(ref._pts) or not np.array_equal(plain._pts.cpu().numpy(), ref._pts.cpu().numpy())
    kept, idx = remove_free_space_points(ref, depth, None, truth, 40.0, rig=rig)
    kept_ref, idx_ref = remove_free_space_points(ref, batch.reshape(S, -1), pin, truth, 40.0)
    assert np.array_equal(idx.cpu().numpy(), idx_ref.cpu().numpy()) and len(idx_ref) > 0

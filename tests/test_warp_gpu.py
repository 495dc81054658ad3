"""GPU suite of the depth -> colour warp and the occlusion test (AC21): kpx_depth_to_color and
kpx_color_to_depth_visible against the float64 restatement tests/warp_ref.py, bit for bit -- u16 and u8 outputs of an fp64 contract
whose minimum does not depend on the order in which threads arrive."""
import numpy as np
import pytest

from tests import sensor_ref as R
from tests import warp_ref as WR
from tests import warp_scenes as WS

SIZES = {"2x2": (2, 2, 31, 17), "24x20": (24, 20, 31, 17), "65x3": (65, 3, 80, 17), "257x3": (257, 3, 272, 17), "64x48": (64, 48, 96, 54),
         "160x144": (160, 144, 320, 180)}
SCENE_SIZED = ("64x48", "160x144")


def _poisoned_out(F, hc, wc):
    import torch
    from kinectpy_amd import _lib
    return torch.full((F, hc, wc), -1, dtype=torch.int16, device=_lib.device()).view(torch.uint16)         # 0xFFFF everywhere


def _same(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {want.size} elements differ, first {bad[:5].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.gpu
@pytest.mark.parametrize("w, h", [(1, 1), (1, 7), (7, 1)])
def test_an_image_without_a_quad_gives_zeros_fully_written(w, h):
    from kinectpy_amd import ops
    cal = WS.sensor(0, w, h, 31, 17)
    depth = np.full((2, w * h), 1500, np.uint16)
    out = _poisoned_out(2, 17, 31)
    got = ops.depth_to_color(depth, WS.table(0, w, h, 31, 17), w, h, [cal], WS.MAX_GAP_MM, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (2, 17, 31)
    assert not got.cpu().numpy().any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES))
def test_warp_is_the_restatement_bit_for_bit(name):
    """2 x 2: one quad; 24 x 20 -> 31 x 17: an odd colour width for the packed u16 stores; widths 65 and 257: a block's tile of quads
    ends inside a row; 160 x 144 -> 320 x 180: many tiles and resolve blocks"""
    from kinectpy_amd import ops
    w, h, wc, hc = SIZES[name]
    depth, xy, _, cals = WS.scene(1, 1, w, h, wc, hc)
    want, cls, hits, spread = WS.reference(1, 1, w, h, wc, hc)
    assert cls["drawn"].any() and (want != 0).any()
    if name in SCENE_SIZED:
        WS.assert_every_class(cls, want, hits, spread)
    got = ops.depth_to_color(depth, xy, w, h, cals, WS.MAX_GAP_MM, out=_poisoned_out(1, hc, wc))
    _same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("F, S", [(1, 1), (4, 2), (6, 3)])
def test_warp_batches_with_a_calibration_per_sensor(F, S):
    from kinectpy_amd import ops
    w, h, wc, hc = SIZES["64x48"]
    depth, xy, _, cals = WS.scene(F, S, w, h, wc, hc, seed=1)
    assert len({c.color.fx for c in cals}) == S
    want, cls, hits, spread = WS.reference(F, S, w, h, wc, hc, seed=1)
    WS.assert_every_class(cls, want, hits, spread)
    _same(ops.depth_to_color(depth, xy, w, h, cals, WS.MAX_GAP_MM), want)
    # max_gap_mm = +inf: no triangle is left out for its depth range (rubber sheets and all)
    loose = WR.depth_to_color(depth[:S], xy, w, h, WR.calibrations_of(cals), wc, hc, np.inf)
    assert (loose != want[:S]).any()
    _same(ops.depth_to_color(depth[:S], xy, w, h, cals, float("inf")), loose)


@pytest.mark.gpu
def test_warp_with_a_long_focal_length_skips_the_boxes_that_are_too_wide():
    """bounding boxes 15 or 16 columns wide (tests/test_warp_cpu.py shows that some are too wide only before they are clamped to the
    image: the comparison is on the unclamped doubles)"""
    from kinectpy_amd import ops
    w, h, wc, hc = SIZES["64x48"]
    depth, xy, _, cals = WS.scene(2, 2, w, h, wc, hc, True)
    want, cls, _, _ = WS.reference(2, 2, w, h, wc, hc, True)
    for k in ("invalid_vertex", "span", "drawn"):
        assert cls[k].any(), k
    assert (want != 0).any() and (want == 0).any()
    _same(ops.depth_to_color(depth, xy, w, h, cals, WS.MAX_GAP_MM, out=_poisoned_out(2, hc, wc)), want)


@pytest.mark.gpu
def test_buffer_discipline_bases_off_by_one_element_guards_and_poisoned_exact_scratch():
    """three 24 x 20 -> 31 x 17 frames: the second frame's output starts 1054 bytes behind the first's, off every boundary beyond 2.
    depth, xy and out each start one element into their buffers; out lies between guard bands and is pre-filled with 0xFF; the
    z-buffer arrives exact-size and poisoned, so the call's own clear is what makes it empty."""
    import torch
    import scratch_harness as H
    from kinectpy_amd import ops, _lib
    F, S = 3, 3
    w, h, wc, hc = SIZES["24x20"]
    depth, xy, _, cals = WS.scene(F, S, w, h, wc, hc)
    want, cls, _, _ = WS.reference(F, S, w, h, wc, hc)
    assert cls["drawn"].any() and (want == 0).any() and (want != 0).any()
    dev = _lib.device()
    dbuf = torch.zeros(depth.size + 1, dtype=torch.uint16, device=dev)
    xbuf = torch.zeros(xy.size + 1, dtype=torch.float32, device=dev)
    d_off, x_off = dbuf[1:].view(F, w * h), xbuf[1:].view(S, w * h, 2)
    d_off.copy_(torch.as_tensor(depth.copy()).to(dev))
    x_off.copy_(torch.as_tensor(xy.copy()).to(dev))
    assert d_off.data_ptr() % 16 == 2 and x_off.data_ptr() % 16 == 4
    n, guard = F * hc * wc, 2048
    state = None
    for pattern in H.PATTERNS:
        raw = torch.full((guard + 1 + n + guard,), 0xA5A5 - 0x10000, dtype=torch.int16, device=dev)
        raw[guard + 1:guard + 1 + n].fill_(-1)                                  # 0xFFFF
        buf = raw.view(torch.uint16)
        out = buf[guard + 1:guard + 1 + n]
        assert out.data_ptr() % 16 == 2
        with H.scratch(pattern, exact=True, state=state) as s:
            ret = ops.depth_to_color(d_off, x_off, w, h, cals, WS.MAX_GAP_MM, out=out)
        state = s
        assert ret.data_ptr() == out.data_ptr()
        assert s.handouts == 1 and s.largest == n * 4, (s.handouts, s.largest)
        host = buf.cpu().numpy()
        assert (host[:guard + 1] == 0xA5A5).all() and (host[guard + 1 + n:] == 0xA5A5).all(), f"guard damaged, scratch pattern {pattern}"
        got = host[guard + 1:guard + 1 + n].reshape(F, hc, wc)
        assert np.array_equal(got, want), f"scratch pattern {pattern}: {(got != want).sum()} elements differ"


@pytest.mark.gpu
@pytest.mark.parametrize("C, interpolation", [(3, "bilinear"), (1, "nearest")])
def test_occlusion_tested_registration_is_the_restatement_bit_for_bit(C, interpolation):
    from kinectpy_amd import ops
    F, S = 4, 2
    w, h, wc, hc = SIZES["64x48"]
    depth, xy, wall, cals = WS.scene(F, S, w, h, wc, hc, seed=1)
    warped = WS.reference(F, S, w, h, wc, hc, seed=1)[0]
    color = np.random.default_rng(C).integers(1, 256, size=(F, hc, wc, C), dtype=np.uint8)
    pairs = WR.calibrations_of(cals)
    want, occluded = WR.visible(depth, xy, color, pairs, interpolation, warped, WS.OCCLUSION_MM)
    assert occluded.sum() > 20 * F and wall[occluded].all() and want.any(-1).sum() > 1000 * F
    got = ops.color_to_depth(depth, xy, color, cals, interpolation, warped=warped, occlusion_mm=WS.OCCLUSION_MM)
    assert tuple(got.shape) == (F, w * h, C)
    _same(got, want)
    assert not got.cpu().numpy()[occluded].any()
    # +inf: never occluded -- the old entry's bytes
    plain = ops.color_to_depth(depth, xy, color, cals, interpolation)
    _same(plain, R.color_to_depth(depth, xy, color, pairs, interpolation))
    never = ops.color_to_depth(depth, xy, color, cals, interpolation, warped=warped, occlusion_mm=float("inf"))
    assert np.array_equal(never.cpu().numpy(), plain.cpu().numpy()) and plain.cpu().numpy()[occluded].any()


@pytest.mark.gpu
def test_rig_registers_masks_with_the_occlusion_test():
    from kinectpy_amd.calibration import SensorRig
    F, S = 4, 2
    w, h, wc, hc = SIZES["64x48"]
    depth, xy, wall, cals = WS.scene(F, S, w, h, wc, hc, seed=1)
    warped = WS.reference(F, S, w, h, wc, hc, seed=1)[0]
    rig = SensorRig(cals)
    _same(rig.warp_depths(depth, WS.MAX_GAP_MM), warped)
    masks = (np.random.default_rng(4).random((F, hc, wc)) < 0.7).astype(np.uint8) * 255
    want, occluded = WR.visible(depth, xy, masks[..., None], WR.calibrations_of(cals), "nearest", warped, WS.OCCLUSION_MM)
    assert occluded.any()
    got = rig.register_masks(depth, masks, occlusion_mm=WS.OCCLUSION_MM, max_gap_mm=WS.MAX_GAP_MM)
    assert tuple(got.shape) == (F, w * h)
    _same(got, want[..., 0])
    plain = rig.register_masks(depth, masks).cpu().numpy()
    assert plain[occluded].any() and np.array_equal(plain[~occluded], want[..., 0][~occluded])
    colors = np.random.default_rng(5).integers(1, 256, size=(F, hc, wc, 3), dtype=np.uint8)
    want_rgb, _ = WR.visible(depth, xy, colors, WR.calibrations_of(cals), "bilinear", warped, WS.OCCLUSION_MM)
    _same(rig.register_colors(depth, colors, occlusion_mm=WS.OCCLUSION_MM, max_gap_mm=WS.MAX_GAP_MM), want_rgb)
    one = cals[1].register_mask(depth[1], masks[1], occlusion_mm=WS.OCCLUSION_MM, max_gap_mm=WS.MAX_GAP_MM)
    _same(one, want[1, :, 0])


@pytest.mark.gpu
def test_warped_depth_and_the_raw_colour_image_give_a_cloud_at_colour_resolution(oracle):
    """SensorCalibration.warp_depth -> ops.depth_to_cloud with color_xy_table() and the colour image as it came from the camera,
    against the restatement's warp and table fed to the oracle's unproject + compact"""
    from kinectpy_amd import ops
    w, h, wc, hc = SIZES["64x48"]
    depth, xy, _, cals = WS.scene(1, 1, w, h, wc, hc)
    want = WS.reference(1, 1, w, h, wc, hc)[0][0]
    cal = cals[0]
    warped = cal.warp_depth(depth[0], WS.MAX_GAP_MM)
    assert tuple(warped.shape) == (hc, wc)
    _same(warped, want)
    ctab = cal.color_xy_table()
    assert cal.color_xy_table() is ctab and tuple(ctab.shape) == (hc * wc, 2)
    ref_tab = R.xy_table(R.cam_of(cal.color), wc, hc)
    assert np.array_equal(ctab.cpu().numpy().view(np.int32), ref_tab.view(np.int32))      # (the whole image has rays: no NaN)
    color = np.random.default_rng(6).integers(1, 256, size=(hc * wc, 3), dtype=np.uint8)
    (pts, col, idx), = ops.depth_to_cloud(warped.reshape(-1), ctab, color, 1, True, False, want_idx=True)
    rp, rc, ri = oracle.rgbd_compact(oracle.unproject_u16(want.reshape(-1), ref_tab), color, True, False)
    assert len(rp) > 1000
    assert np.array_equal(pts.cpu().numpy(), rp) and np.array_equal(col.cpu().numpy(), rc) and np.array_equal(idx.cpu().numpy(), ri)

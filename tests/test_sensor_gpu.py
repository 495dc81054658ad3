"""GPU suite of the sensor calibration (AC20): kpx_xy_table and kpx_color_to_depth against the float64 restatement
tests/sensor_ref.py, bit for bit; the identity rig; buffer discipline of the packed store; the rig end to end into depth_to_cloud."""
import functools

import numpy as np
import pytest

from tests import sensor_ref as R

DW, DH = 24, 20                # the depth camera of the toy sensors
CW, CH = 31, 17                # the colour camera: an odd row length in bytes for 1 and for 3 channels
CLASSES = ("zero_depth", "nan_table", "behind", "beyond_radius", "outside", "sampled")
BORDERS = ("left", "right", "top", "bottom")


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


@functools.lru_cache(maxsize=None)
def toy_sensor(i):
    """SensorCalibration i of the toy rig.  The depth lens is so wide that the image corners lie beyond the metric radius (NaN table
    entries); the colour camera is turned far enough that part of the scene lies behind it, part beyond its metric radius and part
    outside its small image on every side."""
    from kinectpy_amd.calibration import CameraIntrinsics, SensorCalibration
    s = float(i)
    depth = CameraIntrinsics(DW, DH, 10.5 + 0.3 * s, 10.2 + 0.2 * s, 11.6 - 0.4 * s, 9.7 + 0.3 * s, k1=4.9 + 0.1 * s, k2=3.1, k3=0.17, k4=5.23 + 0.1 * s, k5=4.7,
                             k6=0.88, p1=7e-4, p2=-4e-4)
    color = CameraIntrinsics(CW, CH, 17.0 + 1.5 * s, 12.5 + 1.2 * s, 15.2 + 0.6 * s, 8.1 - 0.5 * s, k1=0.61, k2=-2.7, k3=1.5, k4=0.49, k5=-2.5, k6=1.44 + 0.02 * s,
                             p1=5e-3, p2=-2e-3)
    T = np.eye(4)
    T[:3, :3] = _rot("y", 12.0 + 7.0 * s) @ _rot("x", 6.0 - 11.0 * s) @ _rot("z", 3.0 * s)
    T[:3, 3] = [-32.0 - 40.0 * s, -2.0 + 25.0 * s, -450.0 - 60.0 * s]                  # the colour camera sits 45 cm into the scene
    return SensorCalibration(depth, color, T)


@functools.lru_cache(maxsize=None)
def toy_table(i):
    """float32 (DH * DW, 2) reference table of toy sensor i (the restatement's, not the device's)"""
    t = R.xy_table(R.cam_of(toy_sensor(i).depth), DW, DH)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def scene(F, S, n_px, C, seed=0):
    """-> depth u16 (F, n_px), xy f32 (S, n_px, 2), color u8 (F, CH, CW, C), the S calibrations.  n_px == DW * DH: the toy image;
    otherwise a strip whose table entries are drawn from the toy tables (the operator is a map over pixels)."""
    rng = np.random.default_rng(1000 * seed + 100 * F + 10 * S + C + n_px)
    cals = tuple(toy_sensor(i) for i in range(S))
    if n_px == DW * DH:
        xy = np.stack([toy_table(i) for i in range(S)])
    else:
        xy = np.stack([toy_table(i)[rng.integers(0, DW * DH, n_px)] for i in range(S)])
    depth = rng.integers(300, 3000, size=(F, n_px)).astype(np.uint16)
    depth[rng.random((F, n_px)) < 0.1] = 0
    depth[:, -1] = 1234                                   # the last pixel of every frame is live whatever the draw
    color = rng.integers(1, 256, size=(F, CH, CW, C), dtype=np.uint8)
    for a in (depth, xy, color):
        a.setflags(write=False)
    return depth, xy, color, cals


@functools.lru_cache(maxsize=None)
def reference(F, S, n_px, C, interpolation, seed=0):
    depth, xy, color, cals = scene(F, S, n_px, C, seed)
    out, cls = R.color_to_depth(depth, xy, color, [(R.cam_of(c.color), c.depth_to_color) for c in cals], interpolation, want_classes=True)
    out.setflags(write=False)
    return out, cls


def _same_f32(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern"
    bad = np.nonzero(got.view(np.int32)[~nan] != want.view(np.int32)[~nan])[0]
    assert bad.size == 0, f"{bad.size} finite values differ in their bits, first at {bad[:5]}: {got[~nan][bad[:5]]} vs {want[~nan][bad[:5]]}"


def _wide(w, h):
    """distortion strong enough that part of a w x h image lies beyond the metric radius"""
    from kinectpy_amd.calibration import CameraIntrinsics
    return CameraIntrinsics(w, h, 22.0, 22.5, 0.48 * w, 0.47 * h, k1=4.9, k2=3.1, k3=0.17, k4=5.23, k5=4.7, k6=0.88, p1=7e-5, p2=-4e-5)


def _table_cases():
    from kinectpy_amd.calibration import CameraIntrinsics
    from kinectpy_amd.utils import synth
    d = synth.sensor_calibration(0).depth.to_dict()
    mild = lambda w, h: CameraIntrinsics(**dict(d, width=w, height=h, cx=0.4 * w, cy=0.6 * h, fx=0.8 * max(w, h, 8), fy=0.81 * max(w, h, 8)))
    return {"1x1": mild(1, 1), "9x7": mild(9, 7), "13x5": mild(13, 5), "257x1": mild(257, 1), "64x48": _wide(64, 48)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1", "9x7", "13x5", "257x1", "64x48"])
def test_xy_table_is_the_restatement_bit_for_bit(name):
    from kinectpy_amd import ops
    intr = _table_cases()[name]
    want = R.xy_table(R.cam_of(intr), intr.width, intr.height)
    nan = np.isnan(want[:, 0])
    assert (~nan).any()
    if name == "64x48":
        assert 0.2 * nan.size < nan.sum() < 0.8 * nan.size
    got = ops.xy_table(intr)
    assert got.dtype.is_floating_point and tuple(got.shape) == (intr.width * intr.height, 2)
    _same_f32(got.cpu().numpy(), want)


@pytest.mark.gpu
def test_xy_table_of_the_synthetic_sensor_plugs_into_unproject():
    """the real size, and the table taken by the existing entry unchanged: NaN entries give no point"""
    from kinectpy_amd import ops
    from kinectpy_amd.utils import synth
    cal = synth.sensor_calibration(1)
    want = R.xy_table(R.cam_of(cal.depth), 640, 576)
    tab = cal.xy_table()
    assert cal.xy_table() is tab
    _same_f32(tab.cpu().numpy(), want)
    w = _wide(64, 48)
    t = ops.xy_table(w)
    dep = np.full(w.width * w.height, 1000, np.uint16)
    xyz = ops.unproject_u16(dep, t, 1).cpu().numpy()[0]
    nan = np.isnan(t.cpu().numpy()[:, 0])
    assert nan.any() and (xyz[nan] == 0).all() and (xyz[~nan, 2] == 1000).all()


@pytest.mark.gpu
@pytest.mark.parametrize("C, interpolation", [(3, "bilinear"), (1, "nearest")])
@pytest.mark.parametrize("F, S", [(1, 1), (4, 2), (6, 3)])
def test_color_to_depth_is_the_restatement_bit_for_bit(F, S, C, interpolation):
    from kinectpy_amd import ops
    depth, xy, color, cals = scene(F, S, DW * DH, C)
    want, cls = reference(F, S, DW * DH, C, interpolation)
    for k in CLASSES + (BORDERS if interpolation == "bilinear" else ()):
        assert cls[k].any(), f"no pixel of class {k} in the test data"
    assert (want[cls["sampled"]] != 0).any() and not want[~cls["sampled"]].any()
    got = ops.color_to_depth(depth, xy, color, cals, interpolation)
    assert tuple(got.shape) == (F, DW * DH, C)
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first {bad[:5].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.gpu
@pytest.mark.parametrize("C, interpolation", [(3, "bilinear"), (1, "nearest")])
@pytest.mark.parametrize("n_px", [255, 256, 257, 1025])
def test_color_to_depth_strips_run_every_form_of_the_packed_store(n_px, C, interpolation):
    """3 frames of n_px pixels: with n_px = 255, 257, 1025 the second and third frame's output starts off a 4- and 16-byte boundary;
    1025 is one whole block and one pixel"""
    from kinectpy_amd import ops
    depth, xy, color, cals = scene(3, 3, n_px, C)
    want, cls = reference(3, 3, n_px, C, interpolation)
    for k in CLASSES + (BORDERS if interpolation == "bilinear" else ()):
        assert cls[k].any(), f"no pixel of class {k} in the test data"
    got = ops.color_to_depth(depth, xy, color, cals, interpolation).cpu().numpy()
    assert np.array_equal(got, want)
    # depth and table bases off their 16-byte boundaries (by one element each): the element loads, the same bytes
    import torch
    from kinectpy_amd import _lib
    dev = _lib.device()
    dbuf = torch.zeros(depth.size + 1, dtype=torch.uint16, device=dev)
    xbuf = torch.zeros(xy.size + 1, dtype=torch.float32, device=dev)
    d_off, x_off = dbuf[1:].view(3, n_px), xbuf[1:].view(3, n_px, 2)
    d_off.copy_(torch.as_tensor(depth.copy()).to(dev))
    x_off.copy_(torch.as_tensor(xy.copy()).to(dev))
    assert d_off.data_ptr() % 16 == 2 and x_off.data_ptr() % 16 == 4
    assert np.array_equal(ops.color_to_depth(d_off, x_off, color, cals, interpolation).cpu().numpy(), want)
    if C == 1:                                            # a (F, Hc, Wc) mask stack comes back as (F, n_px)
        flat = ops.color_to_depth(depth, xy, color[..., 0], cals, interpolation)
        assert tuple(flat.shape) == (3, n_px) and np.array_equal(flat.cpu().numpy(), want[..., 0])


@pytest.mark.gpu
@pytest.mark.parametrize("C, interpolation", [(3, "bilinear"), (3, "nearest"), (1, "bilinear"), (1, "nearest")])
def test_identity_rig_returns_the_colour_image(C, interpolation):
    """Both cameras the same distortion-free intrinsics with fx, fy, cx, cy powers of two, identity transform: every step of AC20 is
    exact and a depth pixel samples the colour pixel with its own coordinates.  The bilinear rule wants all four neighbours inside the
    image whatever their weight, so the last row and column have no depth here -- and come out zero when they have."""
    from kinectpy_amd import ops
    from kinectpy_amd.calibration import CameraIntrinsics, SensorCalibration
    w, h = 40, 28
    cam = CameraIntrinsics(w, h, 32.0, 16.0, 16.0, 8.0)
    cal = SensorCalibration(cam, cam, np.eye(4))
    rng = np.random.default_rng(8)
    color = rng.integers(1, 256, size=(1, h, w, C), dtype=np.uint8)
    depth = rng.integers(1, 65536, size=(h, w)).astype(np.uint16)
    depth[rng.random((h, w)) < 0.1] = 0
    depth[:, -1] = 0
    depth[-1, :] = 0
    xy = ops.xy_table(cam)
    out = ops.color_to_depth(depth.reshape(1, -1), xy, color, [cal], interpolation).cpu().numpy().reshape(h, w, C)
    live = depth > 0
    assert live.sum() > 0.8 * live.size
    assert np.array_equal(out[live], color[0][live]) and not out[~live].any()
    full = np.full((h, w), 777, np.uint16)
    out = ops.color_to_depth(full.reshape(1, -1), xy, color, [cal], interpolation).cpu().numpy().reshape(h, w, C)
    assert np.array_equal(out[:-1, :-1], color[0, :-1, :-1])
    if interpolation == "bilinear":
        assert not out[-1].any() and not out[:, -1].any()
    else:
        assert np.array_equal(out, color[0])


@pytest.mark.gpu
@pytest.mark.parametrize("C, interpolation", [(3, "bilinear"), (1, "nearest")])
def test_buffer_discipline_every_byte_written_guards_intact_any_alignment(C, interpolation):
    import torch
    import scratch_harness as H
    from kinectpy_amd import ops, _lib
    F, S, n_px = 3, 3, 1025
    depth, xy, color, cals = scene(F, S, n_px, C)
    want, _ = reference(F, S, n_px, C, interpolation)
    assert (want == H.CANARY).sum() < want.size // 20      # (a result byte may equal the fill by chance; most do not)
    dev = _lib.device()
    d_dep, d_xy = torch.as_tensor(depth).to(dev), torch.as_tensor(xy).to(dev)
    nbytes, guard = F * n_px * C, 4096
    cbytes = color.size
    for off, fill in ((0, H.CANARY), (0, 0x5A), (1, H.CANARY), (1, 0x5A), (3, H.CANARY), (3, 0x5A)):
        # (two fills: a byte the kernel skipped cannot hold the right value under both)
        buf = torch.full((guard + off + nbytes + guard,), H.CANARY, dtype=torch.uint8, device=dev)
        out = buf[guard + off:guard + off + nbytes]
        out.fill_(fill)
        assert out.data_ptr() % 4 == (buf.data_ptr() + guard + off) % 4
        cbuf = torch.full((cbytes + 8,), H.CANARY, dtype=torch.uint8, device=dev)
        col = cbuf[off:off + cbytes]
        col.copy_(torch.as_tensor(color).reshape(-1).to(dev))
        col = col.view(F, CH, CW, C)
        assert col.data_ptr() == cbuf.data_ptr() + off
        with H.scratch(0xFF, exact=True) as s:             # neither entry takes device scratch
            ret = ops.color_to_depth(d_dep, d_xy, col, cals, interpolation, out=out)
        assert s.handouts == 0
        assert ret.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        assert (host[:guard + off] == H.CANARY).all() and (host[guard + off + nbytes:] == H.CANARY).all(), f"guard damaged at offset {off}"
        assert np.array_equal(host[guard + off:guard + off + nbytes].reshape(F, n_px, C), want), f"offset {off}"
    with H.scratch(0xFF, exact=True) as s:
        ops.xy_table(cals[0].depth)
    assert s.handouts == 0


@pytest.mark.gpu
def test_rig_registers_colours_into_depth_to_cloud(oracle):
    """SensorRig.register_colors -> ops.depth_to_cloud(..., rgb, color_mask=True), one call per sensor (one table each), against the
    restatement's registration fed to the oracle's unproject + compact; masks through register_masks the same way"""
    import torch
    from kinectpy_amd import ops
    from kinectpy_amd.calibration import SensorRig
    S, n_px = 2, DW * DH
    depth, xy, color, cals = scene(S, S, n_px, 3, seed=1)
    rig = SensorRig(cals)
    tables = rig.xy_tables()
    assert tuple(tables.shape) == (S, n_px, 2) and rig.xy_tables() is tables
    _same_f32(tables.cpu().numpy(), xy)
    rgb = rig.register_colors(depth, color)
    want_rgb, cls = reference(S, S, n_px, 3, "bilinear", seed=1)
    assert np.array_equal(rgb.cpu().numpy(), want_rgb)
    some = 0
    for s in range(S):
        (pts, col, idx), = ops.depth_to_cloud(torch.as_tensor(depth[s]).cuda(), tables[s], rgb[s], 1, True, False, want_idx=True)
        rp, rc, ri = oracle.rgbd_compact(oracle.unproject_u16(depth[s], xy[s]), want_rgb[s], True, False)
        assert np.array_equal(pts.cpu().numpy(), rp) and np.array_equal(col.cpu().numpy(), rc) and np.array_equal(idx.cpu().numpy(), ri)
        assert 0 < len(rp) < cls["sampled"][s].sum() + 1
        some += len(rp)
    assert some > 50
    masks = (color[..., 0] > 128).astype(np.uint8) * 255
    got = rig.register_masks(depth, masks).cpu().numpy()
    want = R.color_to_depth(depth, xy, masks[..., None], [(R.cam_of(c.color), c.depth_to_color) for c in cals], "nearest")[..., 0]
    assert got.shape == (S, n_px) and np.array_equal(got, want) and set(np.unique(got)) == {0, 255}
    one = cals[0].register_color(depth[0], color[0]).cpu().numpy()
    assert one.shape == (n_px, 3) and np.array_equal(one, want_rgb[0])
    assert np.array_equal(cals[1].register_mask(depth[1], masks[1]).cpu().numpy(), want[1])

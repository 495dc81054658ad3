"""CPU suite of the depth -> colour warp and the occlusion test (AC21): the restatement tests/warp_ref.py judged on
rigs whose answer is known in closed form and on the scenes the GPU suite uses, the C entries' argument checks, the Python layers'."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import sensor_ref as R
from tests import warp_ref as WR
from tests import warp_scenes as WS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("kpx_depth_to_color_workspace_bytes", "kpx_depth_to_color", "kpx_color_to_depth_visible")
W, H = 24, 20


def _pinhole_rig(tx=0.0):
    from kinectpy_amd.calibration import CameraIntrinsics, SensorCalibration
    cam = CameraIntrinsics(W, H, 20.3, 19.7, 11.6, 9.4)
    T = np.eye(4)
    T[0, 3] = tx
    return SensorCalibration(cam, cam, T)


def test_identity_rig_of_two_equal_pinhole_cameras_returns_the_depth_image():
    """The float32 table puts a vertex ~1e-7 px to either side of its pixel centre, so a border pixel is covered or not: it equals
    the depth pixel or is 0.  An interior pixel lies inside the mesh whatever the rounding, and every triangle that reaches it
    interpolates to within 1e-5 mm of its own depth."""
    cal = _pinhole_rig()
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.rint(1000.0 + 40.0 * np.sin(c / 5.0) + 30.0 * np.cos(r / 4.0)).astype(np.uint16)
    xy = R.xy_table(R.cam_of(cal.depth), W, H)
    warped, cls, hits, _ = WR.depth_to_color(depth.reshape(1, -1), xy, W, H, WR.calibrations_of([cal]), W, H, 50.0, want_classes=True)
    assert cls["drawn"].all()                              # smooth: no gap exceeded, nothing invalid
    warped = warped[0]
    assert np.array_equal(warped[1:-1, 1:-1], depth[1:-1, 1:-1])
    assert ((warped == depth) | (warped == 0)).all()
    assert (hits[0][1:-1, 1:-1] >= 1).all()


def test_lateral_shift_moves_a_plane_by_its_disparity():
    """a fronto-parallel plane at Z under a pure x-translation: every covered pixel is Z, and the covered columns are the depth
    image's columns moved by fx t_x / Z (-4.466 px: no column edge within 0.4 px of a pixel centre)"""
    Z, tx = 1500, -330.0
    cal = _pinhole_rig(tx)
    disparity = cal.color.fx * tx / Z
    assert 0.3 < disparity - np.floor(disparity) < 0.7
    depth = np.full((1, W * H), Z, np.uint16)
    xy = R.xy_table(R.cam_of(cal.depth), W, H)
    warped = WR.depth_to_color(depth, xy, W, H, WR.calibrations_of([cal]), W, H, 10.0)[0]
    assert set(np.unique(warped)) == {0, Z}
    lo, hi = max(0, int(np.ceil(0 + disparity))), min(W - 1, int(np.floor(W - 1 + disparity)))
    assert (lo, hi) == (0, 18)
    assert (warped[1:-1, lo:hi + 1] == Z).all() and not warped[:, hi + 1:].any()


@pytest.fixture(scope="module")
def person():
    return WS.scene(1, 1, 64, 48, 96, 54), WS.reference(1, 1, 64, 48, 96, 54)


def test_person_before_a_wall_has_every_class_and_occludes_wall_pixels_only(person):
    (depth, xy, wall, cals), (warped, cls, hits, spread) = person
    print({k: int(v.sum()) for k, v in cls.items()}, "empty", int((warped == 0).sum()), "reached twice, unequal", int(spread.sum()))
    WS.assert_every_class(cls, warped, hits, spread)
    assert not cls["span"].any()
    rng = np.random.default_rng(3)
    pairs = WR.calibrations_of(cals)
    for C_, interpolation in ((1, "nearest"), (3, "bilinear")):
        color = rng.integers(1, 256, size=(1, 54, 96, C_), dtype=np.uint8)
        out, occluded = WR.visible(depth, xy, color, pairs, interpolation, warped, WS.OCCLUSION_MM)
        plain = R.color_to_depth(depth, xy, color, pairs, interpolation)
        print(interpolation, "occluded", int(occluded.sum()), "of", int((plain != 0).any(-1).sum()), "sampled")
        assert occluded.sum() > 20 and wall[occluded].all()
        assert not out[occluded].any() and np.array_equal(out[~occluded], plain[~occluded]) and plain[occluded].any()
        never, none = WR.visible(depth, xy, color, pairs, interpolation, warped, np.inf)
        assert not none.any() and np.array_equal(never, plain)


def test_long_focal_length_makes_boxes_too_wide_some_only_before_clamping():
    args = (1, 1, 64, 48, 96, 54, True)
    (depth, xy, _, cals), (warped, cls, hits, _) = WS.scene(*args), WS.reference(*args)
    assert cls["span"].any() and cls["drawn"].any() and (warped != 0).any()
    u, v, z, valid = WR.vertices(depth[0], xy[0], WR.calibrations_of(cals)[0])
    tri = WR.triangle_indices(64, 48)[:, cls["span"][0]]
    x0, x1 = np.ceil(u[tri].min(0)), np.floor(u[tri].max(0))
    y0, y1 = np.ceil(v[tri].min(0)), np.floor(v[tri].max(0))
    clamped = np.minimum(x1, 95.0) - np.maximum(x0, 0.0)
    partly_inside = (clamped >= 0) & (clamped < WR.MAX_SPAN) & (x1 - x0 >= WR.MAX_SPAN) & (np.minimum(y1, 53.0) >= np.maximum(y0, 0.0)) & (y1 - y0 < WR.MAX_SPAN)
    assert partly_inside.any(), "no triangle whose box is too wide only before it is clamped to the image"


def test_the_order_of_the_triangles_does_not_matter(person):
    (depth, xy, _, cals), (warped, _, _, spread) = person
    assert spread.any()
    back = WR.depth_to_color(depth, xy, 64, 48, WR.calibrations_of(cals), 96, 54, WS.MAX_GAP_MM, reverse=True)
    assert np.array_equal(back, warped)


def test_abi_symbols_in_header_and_signatures():
    from kinectpy_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "kinectpx.h")).read()
    assert hdr.count("arithmetic contract AC21") == 1
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+KPX_WARP_MAX_SPAN\s+16\b", hdr) and WR.MAX_SPAN == 16
    i32, i64, f64, vp, sz = C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_size_t
    assert _lib.SIGNATURES["kpx_depth_to_color_workspace_bytes"] == (sz, [i32, i32, i32])
    assert _lib.SIGNATURES["kpx_depth_to_color"] == (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp, i32, f64, vp, vp, sz, vp])
    assert _lib.SIGNATURES["kpx_color_to_depth_visible"] == (C.c_int, _lib.SIGNATURES["kpx_color_to_depth"][1][:11] + [vp, f64, vp, vp])
    assert callable(ops.depth_to_color)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.load()


def test_c_entries_reject_bad_arguments_on_the_host(lib):
    """nothing here reaches a device: this suite runs without one"""
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    q = lib.kpx_depth_to_color_workspace_bytes
    assert q(4, 1280, 720) == 4 * 720 * 1280 * 4 and q(1, 31, 17) == 31 * 17 * 4 and q(65535, 4096, 4096) == 65535 * 4096 * 4096 * 4
    assert q(0, 8, 8) == 0 and q(3, 0, 8) == 0 and q(3, 8, 0) == 0
    err = lambda: lib.kpx_last_error()
    dummy = C.c_void_p(4096)
    cal0 = WS.sensor(0, 64, 48, 96, 54)
    cal = np.concatenate([cal0.color.packed(), cal0.depth_to_color.reshape(16)])
    cals = np.tile(cal, 17)
    hc = cals.ctypes.data_as(C.c_void_p)
    inf, nan = float("inf"), float("nan")

    good = dict(depth=dummy, xy=dummy, w=8, h=6, frames=4, wc=8, hc_=6, cal=hc, s=2, gap=50.0, out=dummy, ws=dummy, wsz=4 * 6 * 8 * 4)

    def warp(**kw):
        a = dict(good, **kw)
        return lib.kpx_depth_to_color(a["depth"], a["xy"], a["w"], a["h"], a["frames"], a["wc"], a["hc_"], a["cal"], a["s"], a["gap"], a["out"], a["ws"],
                                      a["wsz"], None)

    for name in ("depth", "xy", "out", "ws"):
        assert warp(**{name: None}) == -1 and b"null pointer" in err(), name
    assert warp(cal=None) == -1 and b"null calibrations" in err()
    for name in ("w", "h", "frames", "wc", "hc_"):
        assert warp(**{name: -1}) == -1 and b"negative" in err(), name
    assert warp(frames=65536, s=1, wsz=1 << 40) == -1 and b"65535" in err()
    for s in (0, -1, 17):
        assert warp(s=s) == -1 and b"calibrations" in err()
    assert warp(s=3) == -1 and b"do not divide" in err()
    for i in (0, 12, 13 + 5):                              # a focal length, the metric radius, the transform: of the second calibration
        bad = cals.copy()
        bad[29 + i] = nan if i != 12 else -1.0
        assert warp(cal=bad.ctypes.data_as(C.c_void_p)) == -1 and b"calibration 1" in err(), i
    for gap in (nan, -1.0, -inf):
        assert warp(gap=gap) == -1 and b"max_gap_mm" in err(), gap
    assert warp(wsz=good["wsz"] - 1) != 0 and b"workspace too small" in err()
    # nothing to do: KPX_OK without a launch, null pointers and all
    assert warp(frames=0, depth=None, xy=None, out=None, ws=None, wsz=0) == 0
    assert warp(wc=0, depth=None, xy=None, out=None, ws=None, wsz=0) == 0 and warp(hc_=0, depth=None, xy=None, out=None, ws=None, wsz=0) == 0
    assert warp(frames=0, s=3, wsz=0) == 0                 # 3 divides 0

    f = lib.kpx_color_to_depth_visible
    good_v = dict(depth=dummy, xy=dummy, color=dummy, n_px=100, frames=4, wc=8, hc_=6, ch=3, cal=hc, s=2, interp=1, warped=dummy, occ=30.0, out=dummy)

    def vis(**kw):
        a = dict(good_v, **kw)
        return f(a["depth"], a["xy"], a["color"], a["n_px"], a["frames"], a["wc"], a["hc_"], a["ch"], a["cal"], a["s"], a["interp"], a["warped"], a["occ"],
                 a["out"], None)

    for name in ("depth", "xy", "color", "warped", "out"):
        assert vis(**{name: None}) == -1 and b"null pointer" in err(), name
    assert vis(cal=None) == -1 and b"null calibrations" in err()
    assert vis(n_px=-1) == -1 and b"negative" in err() and vis(frames=-2) == -1
    assert vis(frames=65536, s=1) == -1 and b"65535" in err()
    assert vis(wc=0) == -1 and b"colour image size" in err()
    for ch in (0, 2, 4):
        assert vis(ch=ch) == -1 and b"channels" in err()
    for interp in (-1, 2):
        assert vis(interp=interp) == -1 and b"interpolation" in err()
    for s in (0, 17):
        assert vis(s=s) == -1 and b"calibrations" in err()
    assert vis(s=3) == -1 and b"do not divide" in err()
    for occ in (nan, -1.0, -inf):
        assert vis(occ=occ) == -1 and b"occlusion_mm" in err(), occ
    assert vis(frames=0, depth=None, xy=None, color=None, warped=None, out=None) == 0
    assert vis(n_px=0, depth=None, xy=None, color=None, warped=None, out=None, occ=inf) == 0


def test_python_layers_reject_half_given_arguments_without_a_device(lib):
    from kinectpy_amd import ops
    from kinectpy_amd.calibration import SensorCalibration, SensorRig
    a, b = WS.sensor(0, 64, 48, 96, 54), WS.sensor(1, 64, 48, 96, 54)
    depth, mask, color = np.zeros(64 * 48, np.uint16), np.zeros((54, 96), np.uint8), np.zeros((54, 96, 3), np.uint8)
    xy = np.zeros((64 * 48, 2), np.float32)
    with pytest.raises(ValueError, match="go together"):
        ops.color_to_depth(depth[None], xy, mask[None], [a], "nearest", warped=np.zeros((1, 54, 96), np.uint16))
    with pytest.raises(ValueError, match="go together"):
        ops.color_to_depth(depth[None], xy, mask[None], [a], "nearest", occlusion_mm=30.0)
    rig = SensorRig([a, b])
    for call in (lambda: a.register_mask(depth, mask, occlusion_mm=30.0), lambda: a.register_color(depth, color, occlusion_mm=30.0),
                 lambda: rig.register_masks(np.stack([depth] * 2), np.stack([mask] * 2), occlusion_mm=30.0),
                 lambda: rig.register_colors(np.stack([depth] * 2), np.stack([color] * 2), occlusion_mm=30.0)):
        with pytest.raises(ValueError, match="needs max_gap_mm"):
            call()
    with pytest.raises(ValueError, match="give occlusion_mm"):
        a.register_mask(depth, mask, max_gap_mm=50.0)
    other = WS.sensor(1, 64, 48, 80, 54)
    mixed = SensorRig([a, SensorCalibration(other.depth, other.color, other.depth_to_color)])
    with pytest.raises(ValueError, match="differ in size"):
        mixed.warp_depths(np.stack([depth] * 2), 50.0)
    import inspect
    for fn in (ops.depth_to_color, type(a).warp_depth, SensorRig.warp_depths):
        assert inspect.signature(fn).parameters["max_gap_mm"].default is inspect.Parameter.empty          # no invented default
    for fn in (type(a).register_color, type(a).register_mask, SensorRig.register_colors, SensorRig.register_masks):
        p = inspect.signature(fn).parameters
        assert p["occlusion_mm"].default is None and p["max_gap_mm"].default is None

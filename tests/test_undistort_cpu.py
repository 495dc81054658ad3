"""CPU suite of the lens undistortion (AC22): the C entries' declarations and argument checks, the restatement
tests/undistort_ref.py judged against itself and against AC20's inverse, the view-rectangle fits of CameraIntrinsics.undistorted,
and what the Python layers reject before they reach a device."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import sensor_ref as R
from tests import undistort_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"kpx_undistort_map": ["ptr", "ptr", "i32", "i32", "ptr", "ptr"],
               "kpx_remap_u8": ["ptr", "ptr", "i32", "i32", "i32", "i32", "i32", "i32", "i32", "i32", "ptr", "ptr"],
               "kpx_remap_depth": ["ptr", "ptr", "i32", "i32", "i32", "i32", "i32", "i32", "i32", "f64", "ptr", "ptr"]}


@functools.lru_cache(maxsize=None)
def reduced(i, camera="depth", scale=4):
    """synthetic sensor i's lens on an image 1 / scale the size: the same rays per image fraction, the same distortion"""
    from kinectpy_amd.calibration import CameraIntrinsics
    from kinectpy_amd.utils import synth
    d = getattr(synth.sensor_calibration(i), camera).to_dict()
    return CameraIntrinsics(**dict(d, width=d["width"] // scale, height=d["height"] // scale, fx=d["fx"] / scale, fy=d["fy"] / scale, cx=d["cx"] / scale,
                                   cy=d["cy"] / scale))


def wide_camera():
    """a 64 x 48 lens so wide that the image corners lie beyond the metric radius (it ends ~35 px from the principal point)"""
    from kinectpy_amd.calibration import CameraIntrinsics
    return CameraIntrinsics(64, 48, 35.0, 35.5, 30.7, 22.9, k1=4.9, k2=3.1, k3=0.17, k4=5.23, k5=4.7, k6=0.88, p1=7e-5, p2=-4e-5)


def ref_map(cam, target):
    return U.undistort_map(R.cam_of(cam), U.pinhole_of(target), target.width, target.height)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_in_header_and_signatures():
    from kinectpy_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "kinectpx.h")).read()
    assert "AC22" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    ctype_cls = {C.c_void_p: "ptr", C.c_int32: "i32", C.c_int: "i32", C.c_double: "f64"}
    for name, want in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, f"{name} is not declared in include/kinectpx.h"
        params = [" ".join(q.split()) for q in m.group(1).split(",")]
        assert ["ptr" if "*" in q else "f64" if q.startswith("double") else "i32" for q in params] == want, (name, params)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and [ctype_cls[a] for a in args] == want, name
    for fn in ("undistort_map", "remap", "remap_depth"):
        assert callable(getattr(ops, fn))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.load()


def test_c_entries_reject_bad_arguments_on_the_host(lib):
    """nothing here reaches a device: every call either fails a host check or has nothing to do"""
    from kinectpy_amd.utils import synth
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
    err = lambda: lib.kpx_last_error()
    dummy = C.c_void_p(4096)
    cam = synth.sensor_calibration(0).depth.packed()
    pin = np.array([500.0, 501.0, 320.0, 288.0])
    hcam, hpin = cam.ctypes.data_as(C.c_void_p), pin.ctypes.data_as(C.c_void_p)
    m = lib.kpx_undistort_map
    who = b"kpx_undistort_map"
    assert m(None, hpin, 4, 4, dummy, None) == -1 and who in err() and b"null camera" in err()
    assert m(hcam, None, 4, 4, dummy, None) == -1 and who in err() and b"null pinhole" in err()
    assert m(hcam, hpin, 4, 4, None, None) == -1 and who in err() and b"null pointer" in err()
    assert m(hcam, hpin, -1, 4, dummy, None) == -1 and who in err() and b"negative" in err()
    assert m(hcam, hpin, 4, -1, dummy, None) == -1 and who in err()
    for i, bad in ((0, 0.0), (1, 0.0), (12, 0.0), (12, -1.0), (5, np.nan), (3, np.inf)):
        c = cam.copy()
        c[i] = bad
        assert m(c.ctypes.data_as(C.c_void_p), hpin, 4, 4, dummy, None) == -1 and who in err() and b"camera" in err(), (i, bad)
    for i, bad in ((0, 0.0), (1, 0.0), (0, np.nan), (1, np.inf), (2, np.nan), (3, -np.inf)):
        p = pin.copy()
        p[i] = bad
        assert m(hcam, p.ctypes.data_as(C.c_void_p), 4, 4, dummy, None) == -1 and who in err() and b"pinhole" in err(), (i, bad)
    assert m(hcam, hpin, 0, 4, None, None) == 0 and m(hcam, hpin, 4, 0, None, None) == 0          # an empty image is a no-op

    good = dict(src=dummy, map=dummy, ws=8, hs=6, ch=3, wo=5, ho=4, frames=4, maps=2, interp=1, gap=10.0, out=dummy)

    def u8(**kw):
        a = dict(good, **kw)
        return lib.kpx_remap_u8(a["src"], a["map"], a["ws"], a["hs"], a["ch"], a["wo"], a["ho"], a["frames"], a["maps"], a["interp"], a["out"], None)

    def dep(**kw):
        a = dict(good, **kw)
        return lib.kpx_remap_depth(a["src"], a["map"], a["ws"], a["hs"], a["wo"], a["ho"], a["frames"], a["maps"], a["interp"], C.c_double(a["gap"]), a["out"], None)

    for call, who in ((u8, b"kpx_remap_u8"), (dep, b"kpx_remap_depth")):
        for name in ("src", "map", "out"):
            assert call(**{name: None}) == -1 and who in err() and b"null pointer" in err(), name
        for name in ("ws", "hs", "wo", "ho", "frames"):
            assert call(**{name: -1}) == -1 and who in err() and b"negative" in err(), name
        assert call(frames=65536, maps=1) == -1 and who in err() and b"65535" in err()
        for interp in (-1, 2):
            assert call(interp=interp) == -1 and who in err() and b"interpolation" in err()
        for maps in (0, -1, 17):
            assert call(maps=maps) == -1 and who in err() and b"maps" in err()
        assert call(maps=3) == -1 and who in err() and b"do not divide" in err()
        # nothing to do: KPX_OK without a launch, null pointers and all
        assert call(frames=0, src=None, map=None, out=None) == 0
        assert call(wo=0, src=None, map=None, out=None) == 0 and call(ho=0, src=None, map=None, out=None) == 0
        assert call(frames=0, maps=3) == 0                                                       # 3 divides 0
    for ch in (0, 2, 4):
        assert u8(ch=ch) == -1 and b"kpx_remap_u8" in err() and b"channels" in err()
    for gap in (np.nan, -1.0, -np.inf):
        for interp in (0, 1):                                                                    # checked for nearest too
            assert dep(gap=gap, interp=interp) == -1 and b"kpx_remap_depth" in err() and b"max_gap_mm" in err(), gap


# ---- the restatement against itself ---------------------------------------------------------------------------------------------------
def test_a_pinhole_camera_mapped_to_itself_is_the_identity():
    """fx, fy, cx, cy powers of two: every step of the chain is exact.  A general pinhole camera: the fp64 round trip
    fx ((c - cx) / fx) + cx leaves a few ulps of cx, which the one float32 rounding absorbs wherever the coordinate is not 0; at
    column / row 0 the float32 keeps a residue of at most 2 ulps of cx (one rounding of the quotient scaled back by fx, one of the
    product, one of the sum: 1.5 ulps at the magnitude of cx), and the nearest sampler still takes pixel 0."""
    from kinectpy_amd.calibration import CameraIntrinsics
    w, h = 40, 28
    exact = CameraIntrinsics(w, h, 32.0, 16.0, 16.0, 8.0)
    general = CameraIntrinsics(w, h, 50.43, 50.39, 21.7, 12.1)
    rr, cc = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    ident = np.stack([cc, rr], -1)
    rng = np.random.default_rng(3)
    for cam in (exact, general):
        m = ref_map(cam, cam.undistorted())
        assert m.dtype == np.float32 and m.shape == (h, w, 2)
        if cam is exact:
            assert np.array_equal(m, ident)
        else:
            assert np.array_equal(m[1:, 1:], ident[1:, 1:])
            assert np.abs(m[:, 0, 0]).max() <= 2 * np.spacing(cam.cx) and np.abs(m[0, :, 1]).max() <= 2 * np.spacing(cam.cy)
        for C_ in (1, 3):
            img = rng.integers(1, 256, size=(2, h, w, C_), dtype=np.uint8)
            out, cls = U.remap_u8(img, m, "nearest")
            assert np.array_equal(out, img) and cls["sampled"].all()
        dep = rng.integers(1, 65536, size=(2, h, w)).astype(np.uint16)
        out, _ = U.remap_depth(dep, m, "nearest")
        assert np.array_equal(out, dep)
    # bilinear on the exact map: weights (1, 0, 0, 0); the last row and column have a neighbour outside, whatever its weight
    m = ref_map(exact, exact.undistorted())
    img = rng.integers(1, 256, size=(1, h, w, 3), dtype=np.uint8)
    out, cls = U.remap_u8(img, m, "bilinear")
    assert np.array_equal(out[:, :-1, :-1], img[:, :-1, :-1]) and not out[:, -1].any() and not out[:, :, -1].any()
    assert cls["outside_right"][0, :, -1].all() and cls["outside_bottom"][0, -1].all() and cls["sampled"][0, :-1, :-1].all()
    dep = rng.integers(1, 65536, size=(1, h, w)).astype(np.uint16)
    out, _ = U.remap_depth(dep, m, "bilinear", np.inf)
    assert np.array_equal(out[:, :-1, :-1], dep[:, :-1, :-1]) and not out[:, -1].any() and not out[:, :, -1].any()


@pytest.mark.parametrize("i, camera", [(0, "depth"), (3, "depth"), (1, "color")])
def test_map_is_consistent_with_the_inverse_of_ac20(i, camera):
    """AC20's Newton inverse at a map entry (u, v) returns the ray of the target pixel the entry belongs to.  The tolerance is derived:
    the entry is a float32, off the fp64 (u, v) by at most half a float32 ulp at that coordinate, i.e. by (eu, ev) =
    (ulp32(u) / 2 / fx, ulp32(v) / 2 / fy) in distorted normalised coordinates; the inverse stops at a residual of at most 1e-11 there
    (its 1e-22 is the squared length), which adds to both.  Through the inverse of the model's Jacobian [[a, b], [c, d]] (AC20's
    `jacobian` at the ray) that box becomes |dx| <= (|d| eu + |b| ev) / |det|, |dy| <= (|c| eu + |a| ev) / |det|.  The second-order
    term is smaller by the factor curvature * |dx| ~ 1e-6 and the fp64 rounding of the chain by 1e-9; 5 % on top covers both."""
    cam = reduced(i, camera)
    target = cam.undistorted("inside")
    m = ref_map(cam, target)
    assert not np.isnan(m).any()
    c = R.cam_of(cam)
    u, v = m[..., 0].astype(np.float64), m[..., 1].astype(np.float64)
    x, y = R.inverse(c, u, v)
    assert not np.isnan(x).any()
    rr, cc = np.meshgrid(np.arange(target.height, dtype=np.float64), np.arange(target.width, dtype=np.float64), indexing="ij")
    wx, wy = (cc - target.cx) / target.fx, (rr - target.cy) / target.fy
    _, _, t = R.distort(c, wx, wy)
    a, b, cj, d = R.jacobian(c, wx, wy, t)
    det = np.abs(a * d - b * cj)
    assert det.min() > 0.05
    eu = np.spacing(np.abs(m[..., 0])).astype(np.float64) / 2 / abs(cam.fx) + 1e-11
    ev = np.spacing(np.abs(m[..., 1])).astype(np.float64) / 2 / abs(cam.fy) + 1e-11
    tol_x = 1.05 * (np.abs(d) * eu + np.abs(b) * ev) / det
    tol_y = 1.05 * (np.abs(cj) * eu + np.abs(a) * ev) / det
    ex, ey = np.abs(x - wx), np.abs(y - wy)
    print("inverse(map) - pinhole ray: max", ex.max(), ey.max(), "normalised; smallest margin", (tol_x - ex).min(), (tol_y - ey).min())
    assert (ex <= tol_x).all() and (ey <= tol_y).all()
    assert tol_x.max() < 2e-6 and tol_y.max() < 2e-6             # (the bound is tight: about a thousandth of a pixel)


def plane_scene(cam):
    """a tilted plane Z = d0 / (n . (x, y, 1)) seen through the lens: the analytic depth per source pixel (float64, mm) and its u16
    image (0 where the pixel has no ray)"""
    tab = R.xy_table(R.cam_of(cam), cam.width, cam.height).astype(np.float64).reshape(cam.height, cam.width, 2)
    z = 1800.0 / ((0.31 * tab[..., 0] - 0.22 * tab[..., 1]) + 1.0)
    img = np.where(np.isnan(z), 0.0, np.floor(z + 0.5)).astype(np.uint16)
    return z, img


def assert_plane_bracket(out, m, z):
    """every non-zero output lies within [min, max] of the analytic depth over the 2 x 2 source block its map entry falls in, +-1 for
    the roundings to u16 (the source's and, bilinear, the output's: a blend of values each within 0.5 of the plane, rounded once more,
    stays within 1 of the block's range)"""
    h, w = z.shape
    live = out != 0
    x0 = np.floor(m[..., 0].astype(np.float64))[live].astype(np.int64)
    y0 = np.floor(m[..., 1].astype(np.float64))[live].astype(np.int64)
    assert (x0 >= 0).all() and (x0 <= w - 2).all() and (y0 >= 0).all() and (y0 <= h - 2).all()
    block = np.stack([z[y0, x0], z[y0, x0 + 1], z[y0 + 1, x0], z[y0 + 1, x0 + 1]])
    got = out[live].astype(np.float64)
    assert (got >= block.min(0) - 1.0).all() and (got <= block.max(0) + 1.0).all()
    return live.mean()


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_tilted_plane_stays_inside_its_source_block(i):
    cam = reduced(i)
    z, img = plane_scene(cam)
    assert (img != 0).all() and z.max() - z.min() > 500.0
    target = cam.undistorted("inside")
    m = ref_map(cam, target)
    for interpolation, gap in (("nearest", None), ("bilinear", 50.0)):
        out, cls = U.remap_depth(img[None], m, interpolation, gap)
        frac = assert_plane_bracket(out[0], m, z)
        assert frac >= 0.9, (interpolation, frac)
        assert not cls["gap"].any() and not cls["zero_neighbour"].any()
    # fit="same" and fit="all" look beyond the image in places: zeros there, the bracket everywhere else
    for fit in ("same", "all"):
        m = ref_map(cam, cam.undistorted(fit))
        out, cls = U.remap_depth(img[None], m, "bilinear", 50.0)
        assert_plane_bracket(out[0], m, z)
        assert np.array_equal(out[0] != 0, cls["sampled"][0])


# ---- the fits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["depth", "color"])
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_fit_inside_has_every_bilinear_neighbour_and_fit_all_sees_every_border_pixel(i, camera):
    from kinectpy_amd.utils import synth
    cam = getattr(synth.sensor_calibration(i), camera)
    target = cam.undistorted("inside")
    assert (target.width, target.height) == (cam.width, cam.height) and not target.has_distortion()
    m = ref_map(cam, target)
    assert not np.isnan(m).any()
    x0, y0 = np.floor(m[..., 0].astype(np.float64)), np.floor(m[..., 1].astype(np.float64))
    assert x0.min() >= 0 and x0.max() <= cam.width - 2 and y0.min() >= 0 and y0.max() <= cam.height - 2
    wide = cam.undistorted("all")
    r, c = np.arange(cam.height, dtype=np.float64), np.arange(cam.width, dtype=np.float64)
    border = np.concatenate([np.stack([np.zeros_like(r), r], -1), np.stack([np.full_like(r, cam.width - 1.0), r], -1),
                             np.stack([c, np.zeros_like(c)], -1), np.stack([c, np.full_like(c, cam.height - 1.0)], -1)])
    x, y = R.inverse(R.cam_of(cam), border[:, 0], border[:, 1])
    ok = ~np.isnan(x)
    assert ok.all()                                          # (these lenses have a ray at every pixel)
    px, py = np.floor((wide.fx * x + wide.cx) + 0.5), np.floor((wide.fy * y + wide.cy) + 0.5)
    assert px.min() == 0 and px.max() == cam.width - 1 and py.min() == 0 and py.max() == cam.height - 1


def test_fit_all_ignores_rayless_border_pixels_and_fit_inside_refuses_them():
    cam = wide_camera()
    with pytest.raises(ValueError, match="metric radius"):
        cam.undistorted("inside")
    wide = cam.undistorted("all")
    r, c = np.arange(cam.height, dtype=np.float64), np.arange(cam.width, dtype=np.float64)
    border = np.concatenate([np.stack([np.zeros_like(r), r], -1), np.stack([np.full_like(r, cam.width - 1.0), r], -1),
                             np.stack([c, np.zeros_like(c)], -1), np.stack([c, np.full_like(c, cam.height - 1.0)], -1)])
    x, y = R.inverse(R.cam_of(cam), border[:, 0], border[:, 1])
    ok = ~np.isnan(x)
    assert 0 < ok.sum() < ok.size
    px, py = np.floor((wide.fx * x[ok] + wide.cx) + 0.5), np.floor((wide.fy * y[ok] + wide.cy) + 0.5)
    assert px.min() >= 0 and px.max() <= cam.width - 1 and py.min() >= 0 and py.max() <= cam.height - 1
    with pytest.raises(ValueError, match="fit"):
        cam.undistorted("outside")


def test_undistorted_cameras_are_pinhole_and_the_distorted_one_still_refuses():
    from kinectpy_amd.calibration import SensorRig
    from kinectpy_amd.utils import synth
    cal = synth.sensor_calibration(0)
    with pytest.raises(ValueError, match="distortion"):
        cal.depth.to_pinhole()
    same = cal.depth.undistorted()
    assert (same.fx, same.fy, same.cx, same.cy, same.width, same.height) == (cal.depth.fx, cal.depth.fy, cal.depth.cx, cal.depth.cy, 640, 576)
    pin = same.to_pinhole()
    assert (pin.width, pin.height) == (640, 576) and pin.get_focal_length() == (cal.depth.fx, cal.depth.fy)
    small = cal.depth.undistorted("inside", 320, 288)
    assert (small.width, small.height) == (320, 288) and small.to_pinhole().is_valid()
    full = cal.depth.undistorted("inside")
    # the same view on half the pixels: columns 0 and W' - 1 see the same rays
    assert np.isclose(-small.cx / small.fx, -full.cx / full.fx, rtol=0, atol=1e-12) and np.isclose((319 - small.cx) / small.fx, (639 - full.cx) / full.fx, rtol=0, atol=1e-12)
    und = cal.undistorted("inside")
    assert not und.depth.has_distortion() and not und.color.has_distortion() and np.array_equal(und.depth_to_color, cal.depth_to_color)
    assert und.depth == full and und.color.to_pinhole().is_valid()
    rig = SensorRig([synth.sensor_calibration(i) for i in range(4)])
    rects = np.array([c.depth.view_rectangle("inside") for c in rig.calibrations])
    common = rig.common_pinhole()
    assert (common.width, common.height) == (640, 576) and common.to_pinhole().is_valid()
    got = np.array([-common.cx / common.fx, (639 - common.cx) / common.fx, -common.cy / common.fy, (575 - common.cy) / common.fy])
    assert np.allclose(got, [rects[:, 0].max(), rects[:, 1].min(), rects[:, 2].max(), rects[:, 3].min()], rtol=0, atol=1e-12)
    for c in rig.calibrations:                              # the intersection: inside every sensor's image
        m = ref_map(reduced_like(c.depth, 8), reduced_like(common, 8))
        x0, y0 = np.floor(m[..., 0].astype(np.float64)), np.floor(m[..., 1].astype(np.float64))
        assert not np.isnan(m).any() and x0.min() >= 0 and x0.max() <= 80 - 2 and y0.min() >= 0 and y0.max() <= 72 - 2
    union = rig.common_pinhole("color", "all")
    rects = np.array([c.color.view_rectangle("all") for c in rig.calibrations])
    assert np.isclose(-union.cx / union.fx, rects[:, 0].min(), rtol=0, atol=1e-12) and np.isclose((719 - union.cy) / union.fy, rects[:, 3].max(), rtol=0, atol=1e-12)


def reduced_like(cam, scale):
    """`cam` on an image 1 / scale the size with pixel 0 and the last pixel on the same rays (the view rectangle is kept)"""
    from kinectpy_amd.calibration import CameraIntrinsics
    d = cam.to_dict()
    w, h = d["width"] // scale, d["height"] // scale
    sx, sy = (w - 1) / (d["width"] - 1), (h - 1) / (d["height"] - 1)
    return CameraIntrinsics(**dict(d, width=w, height=h, fx=d["fx"] * sx, fy=d["fy"] * sy, cx=d["cx"] * sx, cy=d["cy"] * sy))


# ---- the Python layers, without a device --------------------------------------------------------------------------------------------
def test_python_layers_reject_bad_calls_before_any_device_call():
    from kinectpy_amd import _lib, ops
    from kinectpy_amd.calibration import SensorRig
    from kinectpy_amd.preprocessing import fusion
    from kinectpy_amd.utils import synth
    cals = [synth.sensor_calibration(i) for i in range(2)]
    rig = SensorRig(cals)
    depth = np.zeros((2, 576, 640), np.uint16)
    maps = np.zeros((2, 10, 12, 2), np.float32)
    with pytest.raises(ValueError, match="max_gap_mm"):
        ops.remap_depth(depth, maps, "bilinear")
    with pytest.raises(ValueError, match="interpolation"):
        ops.remap_depth(depth, maps, "cubic")
    with pytest.raises(ValueError, match="interpolation"):
        ops.remap(np.zeros((2, 4, 4, 3), np.uint8), maps, "cubic")
    with pytest.raises(_lib.KinectPxError, match="do not divide"):
        ops.remap_depth(depth[:1], maps, "nearest")
    with pytest.raises(_lib.KinectPxError, match="maps must be"):
        ops.remap(np.zeros((2, 4, 4, 3), np.uint8), maps[..., :1], "nearest")
    with pytest.raises(_lib.KinectPxError, match="dimensions"):
        ops.remap_depth(depth[0, 0], maps, "nearest")
    with pytest.raises(ValueError, match="distortion"):
        ops.undistort_map(cals[0].depth, cals[0].depth)                  # the target must be distortion-free
    with pytest.raises(ValueError, match="max_gap_mm"):
        cals[0].undistort_depth(depth[0], "bilinear")
    with pytest.raises(ValueError, match="max_gap_mm"):
        rig.undistort_depths(depth, "bilinear")
    with pytest.raises(ValueError, match="expected"):
        cals[0].undistort_depth(depth[0, :-1])                           # 575 rows
    with pytest.raises(ValueError, match="expected"):
        cals[0].undistort_color(np.zeros((720, 1280), np.uint8))         # no channel axis
    with pytest.raises(ValueError, match="expected"):
        cals[0].undistort_mask(np.zeros((576, 640), np.uint8))           # a depth-sized mask for the colour camera
    with pytest.raises(ValueError, match="expected"):
        rig.undistort_colors(np.zeros((2, 576, 640, 3), np.uint8))
    with pytest.raises(ValueError, match="do not divide"):
        rig.undistort_depths(np.zeros((3, 576 * 640), np.uint16))
    with pytest.raises(ValueError, match="camera must be"):
        rig.undistort_masks(np.zeros((2, 576, 640), np.uint8), camera="ir")
    pin = cals[0].depth.undistorted().to_pinhole()
    with pytest.raises(ValueError, match="not both"):
        fusion.fuse_depth_tsdf(depth.reshape(2, -1), None, pin, [np.eye(4)], 2000.0, 32, (0, 0, 0), rig=rig)
    with pytest.raises(ValueError, match="not both"):
        fusion.remove_free_space_points(None, depth.reshape(2, -1), pin, [np.eye(4)], 20.0, rig=rig)

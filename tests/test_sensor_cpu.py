"""CPU suite of the sensor calibration (AC20): the restatement tests/sensor_ref.py judged against itself and against
SciPy, the host helpers of kinectpy_amd.calibration against the restatement, the C entries' argument checks, the JSON round trip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import sensor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("kpx_xy_table", "kpx_color_to_depth")
PX_TOL = 1e-7          # the stop rule leaves ~1e-11 normalised = ~6e-9 px at f ~ 600: two orders of margin


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.int64)[~np.isnan(a)], b.view(np.int64)[~np.isnan(b)])


def wide_camera():
    """a 64 x 48 camera so wide that the metric radius ends inside the image (radius ~22 px around the principal point)"""
    from kinectpy_amd.calibration import CameraIntrinsics
    return CameraIntrinsics(64, 48, 22.0, 22.5, 30.7, 22.9, k1=4.9, k2=3.1, k3=0.17, k4=5.23, k5=4.7, k6=0.88, p1=7e-5, p2=-4e-5)


@pytest.fixture(scope="module")
def synth0():
    from kinectpy_amd.utils import synth
    return synth.sensor_calibration(0)


@pytest.fixture(scope="module")
def depth_table64(synth0):
    """the float64 inverse at every pixel of the synthetic depth camera, computed once"""
    cam = R.cam_of(synth0.depth)
    v, u = np.meshgrid(np.arange(synth0.depth.height, dtype=np.float64), np.arange(synth0.depth.width, dtype=np.float64), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    x, y = R.inverse(cam, u, v)
    return cam, u, v, x, y


def test_restatement_forward_of_inverse_is_the_pixel(depth_table64):
    cam, u, v, x, y = depth_table64
    ok = ~np.isnan(x)
    assert ok.sum() > 0.9 * ok.size                       # f ~ 504 on 640 x 576: the whole image lies inside the metric radius
    uu, vv, inside = R.forward_normalised(cam, x[ok], y[ok])
    assert inside.all()
    err = max(np.abs(uu - u[ok]).max(), np.abs(vv - v[ok]).max())
    print("forward(inverse(pixel)) - pixel: max", err, "px over", int(ok.sum()), "pixels")
    assert err <= PX_TOL


def test_restatement_agrees_with_scipy_root(depth_table64):
    from scipy.optimize import root
    cam, u, v, x, y = depth_table64
    rng = np.random.default_rng(5)
    pick = rng.choice(np.nonzero(~np.isnan(x))[0], 200, replace=False)
    fx, fy, cx, cy = cam[:4]
    worst = 0.0
    for i in pick:
        def residual(p, i=i):
            uu, vv, _ = R.forward_normalised(cam, np.float64(p[0]), np.float64(p[1]))
            return [float(uu - u[i]), float(vv - v[i])]
        sol = root(residual, [(u[i] - cx) / fx, (v[i] - cy) / fy], method="hybr", tol=1e-15)
        assert np.abs(sol.fun).max() <= 1e-9, (i, sol.message)          # SciPy's own residual, in pixels
        worst = max(worst, abs(sol.x[0] - x[i]) * fx, abs(sol.x[1] - y[i]) * fy)
    print("restatement - scipy.optimize.root: max", worst, "px")
    assert worst <= PX_TOL


def test_table_is_nan_beyond_the_metric_radius_and_valid_pixels_are_connected():
    from scipy import ndimage
    w = wide_camera()
    cam = R.cam_of(w)
    t = R.xy_table(cam, w.width, w.height)
    assert t.dtype == np.float32 and t.shape == (w.width * w.height, 2)
    nan = np.isnan(t[:, 0])
    assert np.array_equal(nan, np.isnan(t[:, 1]))
    valid = ~nan.reshape(w.height, w.width)
    assert 0.2 * valid.size < valid.sum() < 0.8 * valid.size
    assert ndimage.label(valid)[1] == 1
    r2 = t[~nan].astype(np.float64) ** 2
    assert (r2.sum(1) <= w.metric_radius ** 2 * (1 + 1e-6)).all()
    # the distorted radius of the metric radius: pixels clearly beyond it have no ray, pixels clearly inside have one
    edge = R.distort(cam, np.float64(w.metric_radius), np.float64(0.0))[0]
    v, u = np.meshgrid(np.arange(w.height, dtype=np.float64), np.arange(w.width, dtype=np.float64), indexing="ij")
    rd = np.hypot((u - w.cx) / w.fx, (v - w.cy) / w.fy)
    assert not valid[rd > 1.02 * edge].any() and valid[rd < 0.98 * edge].all()
    assert (rd > 1.02 * edge).any() and (rd < 0.98 * edge).any()


def test_host_project_and_unproject_are_the_restatement_bit_for_bit(synth0):
    rng = np.random.default_rng(11)
    for intr in (synth0.depth, synth0.color, wide_camera()):
        cam = R.cam_of(intr)
        px = np.stack([rng.uniform(-40, intr.width + 40, 3000), rng.uniform(-40, intr.height + 40, 3000)], -1)
        px[:50] = np.floor(px[:50])
        got = intr.unproject(px)
        x, y = R.inverse(cam, px[:, 0], px[:, 1])
        assert _bits_equal(got, np.stack([x, y], -1))
        assert intr.unproject(px.reshape(30, 100, 2)).shape == (30, 100, 2)
        pts = rng.normal(size=(3000, 3)) * [900.0, 900.0, 1500.0] + [0.0, 0.0, 800.0]          # some behind the camera, some beyond the radius
        pts[0] = [1.0, 2.0, 0.0]
        got = intr.project(pts)
        u, v, inside = R.forward(cam, pts[:, 0], pts[:, 1], pts[:, 2])
        ok = inside & (pts[:, 2] > 0.0)
        assert 0 < ok.sum() < len(ok)
        assert _bits_equal(got, np.where(ok[:, None], np.stack([u, v], -1), np.nan))


def test_pinhole_unproject_is_the_pinhole_guess_exactly():
    from kinectpy_amd.calibration import CameraIntrinsics
    p = CameraIntrinsics(640, 576, 504.3, 503.9, 321.7, 287.1)
    assert not p.has_distortion()
    rng = np.random.default_rng(2)
    px = np.stack([rng.uniform(0, 640, 500), rng.uniform(0, 576, 500)], -1)
    want = np.stack([(px[:, 0] - p.cx) / p.fx, (px[:, 1] - p.cy) / p.fy], -1)
    assert _bits_equal(p.unproject(px), want)
    x, y = R.inverse(R.cam_of(p), px[:, 0], px[:, 1])
    assert _bits_equal(np.stack([x, y], -1), want)
    pin = p.to_pinhole()
    assert (pin.width, pin.height) == (640, 576) and pin.get_focal_length() == (504.3, 503.9) and pin.get_principal_point() == (321.7, 287.1)


def test_synthetic_calibration_is_what_the_docstring_says():
    from kinectpy_amd.utils import synth
    a, b = synth.sensor_calibration(0), synth.sensor_calibration(1)
    assert (a.depth.width, a.depth.height, a.color.width, a.color.height) == (640, 576, 1280, 720)
    assert abs(a.depth.fx - 504) < 2 and abs(a.color.fx - 605) < 2
    for cam in (a.depth, a.color):
        assert all(getattr(cam, k) != 0.0 for k in ("k1", "k2", "k3", "k4", "k5", "k6")) and cam.has_distortion()
    T = a.depth_to_color
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12) and 30 < np.linalg.norm(T[:3, 3]) < 34
    assert 5.5 < np.degrees(np.arccos((np.trace(T[:3, :3]) - 1) / 2)) < 6.5
    assert a != b and a == synth.sensor_calibration(0)


def test_abi_symbols_in_header_and_signatures():
    from kinectpy_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "kinectpx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    for name, value in (("KPX_CAMERA_DOUBLES", 13), ("KPX_CALIBRATION_DOUBLES", 29), ("KPX_SENSOR_MAX_CALIBRATIONS", 16), ("KPX_SAMPLE_NEAREST", 0),
                        ("KPX_SAMPLE_BILINEAR", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    assert ops.SAMPLE_MODES == {"nearest": 0, "bilinear": 1}
    assert (ops.CAMERA_DOUBLES, ops.CALIBRATION_DOUBLES, ops.SENSOR_MAX_CALIBRATIONS) == (13, 29, 16)
    assert callable(ops.xy_table) and callable(ops.color_to_depth)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.load()


def test_c_entries_reject_bad_arguments_on_the_host(lib, synth0):
    """nothing here reaches a device: this suite runs without one"""
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    err = lambda: lib.kpx_last_error()
    dummy = C.c_void_p(4096)
    cam = synth0.depth.packed()
    hcam = cam.ctypes.data_as(C.c_void_p)
    t = lib.kpx_xy_table
    assert t(None, 4, 4, dummy, None) == -1 and b"null camera" in err()
    assert t(hcam, 4, 4, None, None) == -1 and b"null pointer" in err()
    assert t(hcam, -1, 4, dummy, None) == -1 and b"negative" in err()
    assert t(hcam, 4, -1, dummy, None) == -1
    for i, bad in ((0, 0.0), (1, 0.0), (12, 0.0), (12, -1.0), (5, np.nan), (3, np.inf)):
        c = cam.copy()
        c[i] = bad
        assert t(c.ctypes.data_as(C.c_void_p), 4, 4, dummy, None) == -1 and b"metric radius" in err(), (i, bad)
    assert t(hcam, 0, 4, None, None) == 0 and t(hcam, 4, 0, None, None) == 0             # an empty image is a no-op

    cal = np.concatenate([synth0.color.packed(), synth0.depth_to_color.reshape(16)])
    assert cal.size == 29
    cals = np.tile(cal, 17)
    hc = cals.ctypes.data_as(C.c_void_p)
    f = lib.kpx_color_to_depth
    good = dict(depth=dummy, xy=dummy, color=dummy, n_px=100, frames=4, wc=8, hc_=6, ch=3, cal=hc, s=2, interp=1, out=dummy)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["depth"], a["xy"], a["color"], a["n_px"], a["frames"], a["wc"], a["hc_"], a["ch"], a["cal"], a["s"], a["interp"], a["out"], None)

    for name in ("depth", "xy", "color", "out"):
        assert call(**{name: None}) == -1 and b"null pointer" in err(), name
    assert call(cal=None) == -1 and b"null calibrations" in err()
    assert call(n_px=-1) == -1 and b"negative" in err()
    assert call(frames=-2) == -1
    assert call(frames=65536, s=1) == -1 and b"65535" in err()
    assert call(wc=0) == -1 and b"colour image size" in err()
    assert call(hc_=-3) == -1
    for ch in (0, 2, 4):
        assert call(ch=ch) == -1 and b"channels" in err()
    for interp in (-1, 2):
        assert call(interp=interp) == -1 and b"interpolation" in err()
    for s in (0, -1, 17):
        assert call(s=s) == -1 and b"calibrations" in err()
    assert call(s=3) == -1 and b"do not divide" in err()
    badcal = cals.copy()
    badcal[29 + 13 + 5] = np.nan                                                          # the second calibration's transform
    assert call(cal=badcal.ctypes.data_as(C.c_void_p)) == -1 and b"calibration 1" in err()
    # zero sizes: KPX_OK without a launch, null pointers and all
    assert call(frames=0, depth=None, xy=None, color=None, out=None) == 0
    assert call(n_px=0, depth=None, xy=None, color=None, out=None) == 0
    assert call(frames=0, s=3) == 0                                                       # 3 divides 0


def test_json_round_trip_is_exact(tmp_path, synth0):
    from kinectpy_amd.calibration import CameraIntrinsics, SensorCalibration, SensorRig
    from kinectpy_amd.utils import synth
    odd = SensorCalibration(CameraIntrinsics(7, 5, 0.1 + 0.2, 1 / 3, np.pi, np.e, k1=1e-300, k2=-5e-324, k6=2.0 ** 0.5, p2=1e17 / 3, metric_radius=1.7000000000000002),
                            synth0.color, synth0.depth_to_color)
    for i, cal in enumerate((synth0, synth.sensor_calibration(3), odd)):
        path = tmp_path / f"cal{i}.json"
        cal.save(str(path))
        back = SensorCalibration.load(str(path))
        assert back == cal
        assert np.array_equal(back.depth.packed().view(np.int64), cal.depth.packed().view(np.int64))
        assert np.array_equal(back.color.packed().view(np.int64), cal.color.packed().view(np.int64))
        assert np.array_equal(back.depth_to_color.view(np.int64), cal.depth_to_color.view(np.int64))
        assert (back.depth.width, back.depth.height) == (cal.depth.width, cal.depth.height)
    with pytest.raises(ValueError, match="distortion"):
        synth0.depth.to_pinhole()
    assert len(SensorRig([synth0, synth.sensor_calibration(1)])) == 2
    with pytest.raises(ValueError):
        SensorRig([synth0, odd])
    cv = CameraIntrinsics.from_opencv(640, 576, [[504.0, 0, 320.5], [0, 504.5, 330.0], [0, 0, 1]], [1, 2, 3, 4, 5, 6, 7, 8])
    assert (cv.k1, cv.k2, cv.p1, cv.p2, cv.k3, cv.k4, cv.k5, cv.k6) == (1, 2, 3, 4, 5, 6, 7, 8) and (cv.fx, cv.fy, cv.cx, cv.cy) == (504.0, 504.5, 320.5, 330.0)


def test_frame_source_with_an_array_is_unchanged_and_a_calibration_becomes_its_table(tmp_path, monkeypatch, synth0):
    """extract(pointcloud=True) hands ops.unproject_u16 the array a frame_source returned, untouched, and the calibration's table when
    it returned a SensorCalibration; color=True / depth=True keep raising.  (The device calls are replaced: no GPU here.)"""
    from kinectpy_amd import ops
    from kinectpy_amd.preprocessing.extractor import MKVFilesProcessing
    seen = []

    class FakeXYZ:
        def __init__(self, n, px):
            self.a = np.zeros((n, px, 3), np.int16)

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    def fake_unproject(depth, xy, frames=1):
        seen.append((xy, frames))
        return FakeXYZ(frames, 6)

    monkeypatch.setattr(ops, "unproject_u16", fake_unproject)
    table = np.arange(12, dtype=np.float32).reshape(6, 2)
    frames = [(10, np.arange(6, dtype=np.uint16)), (0, np.zeros(6, np.uint16)), (20, np.arange(6, dtype=np.uint16))]
    out = tmp_path / "a"
    MKVFilesProcessing(["a.mkv"], [str(out)], frame_source=lambda fp: (table, iter(frames))).extract(pointcloud=True)
    assert len(seen) == 1 and seen[0][0] is table and seen[0][1] == 3
    assert sorted(os.listdir(out / "depths")) == ["10_depth.dat", "20_depth.dat"]
    sentinel = object()
    monkeypatch.setattr(type(synth0), "xy_table", lambda self: sentinel)
    out = tmp_path / "b"
    p = MKVFilesProcessing(["b.mkv"], [str(out)], frame_source=lambda fp: (synth0, iter(frames)))
    p.extract(pointcloud=True)
    assert len(seen) == 2 and seen[1][0] is sentinel
    with pytest.raises(NotImplementedError):
        p.extract(color=True)
    with pytest.raises(NotImplementedError):
        p.extract(depth=True)

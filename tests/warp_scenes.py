"""Sensors and scenes of the AC21 suites (tests/test_warp_cpu.py, tests/test_warp_gpu.py) -- TEST INFRASTRUCTURE ONLY.

Everything is computed once per argument set and handed out read-only: the restatement's table of a sensor, a scene's depth image,
the restatement's warp of it.
"""
import functools

import numpy as np

from tests import sensor_ref as R
from tests import warp_ref as WR

MAX_GAP_MM = 100.0          # the scenes below put 1 m between person and wall, and less than 20 mm between neighbours on either
OCCLUSION_MM = 100.0


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


@functools.lru_cache(maxsize=None)
def sensor(i, w, h, wc, hc, long_focal=False):
    """SensorCalibration i of a w x h depth camera (f = 0.8 w) and a wc x hc colour camera (f = 0.62 wc) ~120 mm beside it, both with
    the rational lens model's six radial terms.  long_focal: a colour camera so long that neighbouring depth pixels land ~16.3
    columns and ~12 rows apart: the bounding boxes of the triangles are 15 or 16 columns wide, and the image holds a few of them."""
    from kinectpy_amd.calibration import CameraIntrinsics, SensorCalibration
    s = float(i)
    fd = 0.8 * w + 0.3 * s
    depth = CameraIntrinsics(w, h, fd, fd + 0.2, 0.5 * w - 0.4 + 0.3 * s, 0.5 * h + 0.3 - 0.2 * s, k1=4.9 + 0.1 * s, k2=3.1, k3=0.17, k4=5.23 + 0.1 * s, k5=4.7,
                             k6=0.88, p1=7e-4, p2=-4e-4)
    fx, fy = (16.3 * fd, 12.0 * fd) if long_focal else (0.62 * wc + 0.5 * s, 0.62 * wc + 0.4 * s)
    color = CameraIntrinsics(wc, hc, fx, fy, 0.5 * wc + 0.7 - 0.3 * s, 0.5 * hc - 0.4 + 0.2 * s, k1=0.61, k2=-2.7, k3=1.5, k4=0.49, k5=-2.5, k6=1.44 + 0.02 * s,
                             p1=5e-4, p2=-2e-4)
    T = np.eye(4)
    T[:3, :3] = _rot("z", 0.3 - 0.1 * s) @ _rot("x", 2.0 + 0.5 * s)
    T[:3, 3] = [-120.0 - 5.0 * s, -3.0 + 2.0 * s, 4.0 - s]
    if long_focal:                                        # (a tenth of the baseline and no tilt: the scene stays in the narrow view)
        T[:3, :3] = _rot("z", 0.3 - 0.1 * s)
        T[:3, 3] *= 0.1
    return SensorCalibration(depth, color, T)


@functools.lru_cache(maxsize=None)
def table(i, w, h, wc, hc, long_focal=False):
    """float32 (h * w, 2): the restatement's ray table of the sensor's depth camera"""
    t = R.xy_table(R.cam_of(sensor(i, w, h, wc, hc, long_focal).depth), w, h)
    t.setflags(write=False)
    return t


def person_wall(xy, seed):
    """a person (an ellipsoid cap around z = 1 m on the optical axis) before a slanted wall (z = 2 m on the axis), 3 % of the pixels
    without depth -> depth u16 (n_px,), wall bool (n_px,)"""
    rng = np.random.default_rng(seed)
    xt, yt = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        e = (xt / 0.22) ** 2 + (yt / 0.3) ** 2
        person = e < 1.0
        z = np.where(person, 1000.0 - 80.0 * (1.0 - e), 2000.0 / (1.0 - 0.3 * xt - 0.1 * yt))
    depth = np.where(np.isnan(z), 0.0, np.rint(z)).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.03] = 0
    return depth, ~person & (depth != 0)


@functools.lru_cache(maxsize=None)
def scene(F, S, w, h, wc, hc, long_focal=False, seed=0):
    """-> depth u16 (F, h * w), xy f32 (S, h * w, 2), wall bool (F, h * w), the S sensors"""
    cals = tuple(sensor(i, w, h, wc, hc, long_focal) for i in range(S))
    xy = np.stack([table(i, w, h, wc, hc, long_focal) for i in range(S)])
    if w < 8:                                             # too few columns for a person: a plane at 1.5 m, every pixel "wall"
        frames = [(np.full(w * h, 1500, np.uint16), np.ones(w * h, bool))] * F
    else:
        frames = [person_wall(xy[f % S], 100 * seed + 10 * f + S) for f in range(F)]
    depth, wall = np.stack([d for d, _ in frames]), np.stack([m for _, m in frames])
    for a in (depth, xy, wall):
        a.setflags(write=False)
    return depth, xy, wall, cals


@functools.lru_cache(maxsize=None)
def reference(F, S, w, h, wc, hc, long_focal=False, seed=0, max_gap_mm=MAX_GAP_MM):
    """the restatement's warp of scene(...): warped u16 (F, hc, wc), classes, hits, spread"""
    depth, xy, _, cals = scene(F, S, w, h, wc, hc, long_focal, seed)
    res = WR.depth_to_color(depth, xy, w, h, WR.calibrations_of(cals), wc, hc, max_gap_mm, want_classes=True)
    res[0].setflags(write=False)
    return res


def assert_every_class(cls, warped, hits, spread, want=("invalid_vertex", "gap", "drawn")):
    for k in want:
        assert cls[k].any(), f"no triangle of class {k} in the test data"
    assert (warped == 0).any() and (warped != 0).any(), "no empty / no covered colour pixel in the test data"
    assert (hits > 1).any() and spread.any(), "no colour pixel reached more than once with different depths"

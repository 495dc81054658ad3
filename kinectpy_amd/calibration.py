"""Sensor calibration (arithmetic contract AC20): the lens model of a camera, the depth -> colour transform of one
sensor, and a rig of sensors.

The reference pairs `<ts>_rgb.png` with `<ts>_depth.dat` row for row (preprocessing/data.py:165-178) because the sensor SDK's
offline processor has already un-projected the depth image through the lens model and warped the colour image into the depth
camera.  Both steps are open geometry (OpenCV's rational model); here they are `SensorCalibration.xy_table()` -- the table every
entry point at the front of the hot path takes -- and `register_color` / `register_mask`, on the device.  Contract AC21 (DESIGN.md
5.22) adds `warp_depth` -- the depth image rendered into the colour camera through a z-buffer -- and with it the occlusion test of
the `register_*` methods (`occlusion_mm`, `max_gap_mm`): the strip of background the depth camera sees beside a silhouette, where the
colour camera sees the subject, no longer takes the subject's colour and mask label.  Contract AC22 adds lens
undistortion for the pinhole-only consumers (TSDF volumes, odometry, VoxelGrid carving): `undistorted()` gives the distortion-free
camera with the same centre and axis, `undistort_map()` the device map from its pixels to the lens's, and `undistort_depth` /
`undistort_color` / `undistort_mask` (`SensorRig.undistort_*s` for a batch) the images resampled through it.

`CameraIntrinsics.project` / `unproject` are host NumPy float64 that follow AC20 operation for operation: they are meant for a
handful of skeleton joints, not for images.
"""
import json

import numpy as np

from . import ops

_FIELDS = ("width", "height", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2", "metric_radius")
MAX_ROUNDS = 21             # 20 Newton steps and one last test
RESIDUAL2 = 1e-22


class CameraIntrinsics:
    """Pixel units; integer pixel coordinates are pixel centres; k1..k6, p1, p2 have OpenCV's meaning (pyk4a's
    get_camera_matrix / get_distortion_coefficients: `from_opencv`)."""

    def __init__(self, width, height, fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, k4=0.0, k5=0.0, k6=0.0, p1=0.0, p2=0.0, metric_radius=1.7):
        self.width, self.height = int(width), int(height)
        for name, v in zip(_FIELDS[2:], (fx, fy, cx, cy, k1, k2, k3, k4, k5, k6, p1, p2, metric_radius)):
            setattr(self, name, float(v))
        if self.width < 0 or self.height < 0:
            raise ValueError(f"CameraIntrinsics: image size {self.width} x {self.height}")
        if not np.all(np.isfinite(self.packed())) or self.fx == 0.0 or self.fy == 0.0 or not self.metric_radius > 0.0:
            raise ValueError("CameraIntrinsics: finite numbers, non-zero focal lengths and a positive metric radius")

    @classmethod
    def from_opencv(cls, width, height, camera_matrix, dist_coeffs, metric_radius=1.7):
        """camera_matrix 3x3, dist_coeffs in OpenCV's storage order (k1, k2, p1, p2, k3, k4, k5, k6), shorter vectors padded with 0"""
        K = np.asarray(camera_matrix, dtype=np.float64).reshape(3, 3)
        d = np.zeros(8)
        dc = np.asarray(dist_coeffs, dtype=np.float64).reshape(-1)[:8]
        d[:dc.size] = dc
        return cls(width, height, K[0, 0], K[1, 1], K[0, 2], K[1, 2], d[0], d[1], d[4], d[5], d[6], d[7], d[2], d[3], metric_radius)

    def packed(self):
        """float64[13]: fx fy cx cy k1..k6 p1 p2 metric_radius (KPX_CAMERA_DOUBLES of include/kinectpx.h)"""
        return np.array([getattr(self, n) for n in _FIELDS[2:]], dtype=np.float64)

    def to_dict(self):
        return {n: getattr(self, n) for n in _FIELDS}

    @classmethod
    def from_dict(cls, d):
        return cls(**{n: d[n] for n in _FIELDS})

    def __eq__(self, other):
        return isinstance(other, CameraIntrinsics) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return "CameraIntrinsics(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in _FIELDS) + ")"

    def has_distortion(self):
        return any(getattr(self, n) != 0.0 for n in _FIELDS[6:14])

    def to_pinhole(self):
        """o3d.camera.PinholeCameraIntrinsic for the pinhole-only consumers (TSDF, odometry, VoxelGrid carving); refuses a distorted
        camera: those consumers would silently use the wrong rays."""
        if self.has_distortion():
            raise ValueError("to_pinhole: this camera has lens distortion; undistort the images first (undistorted() is the camera "
                             "they are then taken with, SensorCalibration.undistort_depth / undistort_color resample them)")
        from . import o3d
        return o3d.camera.PinholeCameraIntrinsic(self.width, self.height, self.fx, self.fy, self.cx, self.cy)

    # ---- AC22: the distortion-free camera with this one's centre and axis -----------------------------------------------------
    def _border_rays(self):
        """the rays of the border pixel centres of the image as four (n, 2) arrays of normalised (x, y): left, right, top, bottom edge
        (NaN pairs where a pixel has no ray)"""
        if self.width < 1 or self.height < 1:
            raise ValueError("undistorted: the camera has no image size to fit a rectangle to")
        r = np.arange(self.height, dtype=np.float64)
        c = np.arange(self.width, dtype=np.float64)
        edges = (np.stack([np.zeros_like(r), r], -1), np.stack([np.full_like(r, self.width - 1.0), r], -1),
                 np.stack([c, np.zeros_like(c)], -1), np.stack([c, np.full_like(c, self.height - 1.0)], -1))
        return tuple(self.unproject(e) for e in edges)

    def view_rectangle(self, fit):
        """(x_left, x_right, y_top, y_bottom) in normalised coordinates.  fit="inside": the rectangle inside the image's outline --
        the largest x on the left edge, the smallest on the right, the same for y -- shrunk by one source pixel (1 / fx, 1 / fy) on
        each side, so that every pixel of a target fitted to it has all four bilinear neighbours; a border pixel without a ray
        raises ValueError.  fit="all": the rectangle around every border pixel that has a ray."""
        left, right, top, bottom = self._border_rays()
        if fit == "inside":
            if any(np.isnan(e).any() for e in (left, right, top, bottom)):
                raise ValueError('undistorted: fit="inside" needs a ray at every border pixel, and some lie beyond the metric radius (fit="all" ignores them)')
            px, py = abs(1.0 / self.fx), abs(1.0 / self.fy)
            rect = (left[:, 0].max() + px, right[:, 0].min() - px, top[:, 1].max() + py, bottom[:, 1].min() - py)
        elif fit == "all":
            rays = np.concatenate([left, right, top, bottom])
            rays = rays[~np.isnan(rays[:, 0])]
            if rays.size == 0:
                raise ValueError("undistorted: no border pixel has a ray")
            rect = (rays[:, 0].min(), rays[:, 0].max(), rays[:, 1].min(), rays[:, 1].max())
        else:
            raise ValueError(f'undistorted: fit must be "same", "inside" or "all", got {fit!r}')
        return tuple(float(v) for v in rect)

    @classmethod
    def from_view_rectangle(cls, rect, width, height, metric_radius=1.7):
        """the distortion-free camera whose pixel columns 0 .. width - 1 span x_left .. x_right and rows 0 .. height - 1 span
        y_top .. y_bottom: fx' = (width - 1) / (x_right - x_left), cx' = -fx' x_left, the same for y"""
        xl, xr, yt, yb = rect
        if not (xr > xl and yb > yt) or width < 2 or height < 2:
            raise ValueError(f"undistorted: empty view rectangle x {xl} .. {xr}, y {yt} .. {yb} for a {width} x {height} image")
        fx = (width - 1) / (xr - xl)
        fy = (height - 1) / (yb - yt)
        return cls(width, height, fx, fy, -fx * xl, -fy * yt, metric_radius=metric_radius)

    def undistorted(self, fit="same", width=None, height=None):
        """the distortion-free CameraIntrinsics (to_pinhole() works on it) of width x height pixels (default: this camera's) that the
        undistorted images are taken with.  fit="same" keeps fx, fy, cx, cy; "inside" / "all" fit the view to view_rectangle(fit):
        "inside" sees only what the lens saw (no empty border), "all" everything it saw."""
        w = self.width if width is None else int(width)
        h = self.height if height is None else int(height)
        if fit == "same":
            return CameraIntrinsics(w, h, self.fx, self.fy, self.cx, self.cy, metric_radius=self.metric_radius)
        return CameraIntrinsics.from_view_rectangle(self.view_rectangle(fit), w, h, self.metric_radius)

    def undistort_map(self, pinhole=None):
        """AC22's map for the target camera `pinhole` (default: undistorted()): float32 (H', W', 2) on the device (ops.undistort_map),
        computed once per target"""
        target = self.undistorted() if pinhole is None else pinhole
        key = (tuple(self.packed()), _target_key(target))
        cache = self.__dict__.setdefault("_maps", {})
        if key not in cache:
            cache[key] = ops.undistort_map(self, target)
        return cache[key]

    # ---- AC20 on the host ------------------------------------------------------------------------------------------------------
    def _distort(self, x, y):
        xx = x * x
        yy = y * y
        r2 = xx + yy
        r4 = r2 * r2
        r6 = r4 * r2
        num = ((1.0 + self.k1 * r2) + self.k2 * r4) + self.k3 * r6
        den = ((1.0 + self.k4 * r2) + self.k5 * r4) + self.k6 * r6
        radial = num / den
        xy2 = 2.0 * (x * y)
        xd = (x * radial + self.p1 * xy2) + self.p2 * (r2 + 2.0 * xx)
        yd = (y * radial + self.p1 * (r2 + 2.0 * yy)) + self.p2 * xy2
        return xd, yd, r2, r4, num, den, radial

    def project(self, points):
        """(..., 3) points in the camera frame -> (..., 2) pixel coordinates, NaN pairs where Z <= 0 or beyond the metric radius"""
        p = np.asarray(points, dtype=np.float64)
        X, Y, Z = p[..., 0], p[..., 1], p[..., 2]
        with np.errstate(all="ignore"):
            x = X / Z
            y = Y / Z
            xd, yd, r2 = self._distort(x, y)[:3]
            u = self.fx * xd + self.cx
            v = self.fy * yd + self.cy
            ok = (Z > 0.0) & (r2 <= self.metric_radius * self.metric_radius)
        return np.where(ok[..., None], np.stack([u, v], -1), np.nan)

    def unproject(self, pixels):
        """(..., 2) pixel coordinates -> (..., 2) normalised (x, y) = (X / Z, Y / Z) of the ray, NaN pairs where there is none"""
        uv = np.asarray(pixels, dtype=np.float64)
        shape = uv.shape[:-1]
        u, v = uv[..., 0].reshape(-1), uv[..., 1].reshape(-1)
        xn = (u - self.cx) / self.fx
        yn = (v - self.cy) / self.fy
        x, y = xn.copy(), yn.copy()
        live = np.ones(x.shape, dtype=bool)             # still iterating
        done = np.zeros(x.shape, dtype=bool)            # converged
        p1x2, p2x2, p1x6, p2x6 = 2.0 * self.p1, 2.0 * self.p2, 6.0 * self.p1, 6.0 * self.p2
        with np.errstate(all="ignore"):
            for rnd in range(MAX_ROUNDS):
                i = np.nonzero(live)[0]
                if i.size == 0:
                    break
                xi, yi = x[i], y[i]
                xd, yd, r2, r4, num, den, radial = self._distort(xi, yi)
                ex = xd - xn[i]
                ey = yd - yn[i]
                conv = ex * ex + ey * ey <= RESIDUAL2
                done[i[conv]] = True
                if rnd == MAX_ROUNDS - 1:
                    break
                nd = (self.k1 + (2.0 * self.k2) * r2) + (3.0 * self.k3) * r4
                dd = (self.k4 + (2.0 * self.k5) * r2) + (3.0 * self.k6) * r4
                dr = (nd * den - num * dd) / (den * den)
                gx = (2.0 * xi) * dr
                gy = (2.0 * yi) * dr
                a = ((radial + xi * gx) + p1x2 * yi) + p2x6 * xi
                b = (xi * gy + p1x2 * xi) + p2x2 * yi
                c = (yi * gx + p1x2 * xi) + p2x2 * yi
                d = ((radial + yi * gy) + p1x6 * yi) + p2x2 * xi
                det = a * d - b * c
                step = ~conv & np.isfinite(det) & (det != 0.0)
                live[i[~step]] = False
                j = i[step]
                x[j] = xi[step] - ((d * ex - b * ey) / det)[step]
                y[j] = yi[step] - ((a * ey - c * ex) / det)[step]
            ok = done & np.isfinite(x) & np.isfinite(y) & (x * x + y * y <= self.metric_radius * self.metric_radius)
        out = np.where(ok[:, None], np.stack([x, y], -1), np.nan)
        return out.reshape(shape + (2,))


class SensorCalibration:
    """One sensor: its depth camera, its colour camera and the 4x4 depth -> colour transform in millimetres."""

    def __init__(self, depth, color, depth_to_color):
        if not isinstance(depth, CameraIntrinsics) or not isinstance(color, CameraIntrinsics):
            raise TypeError("SensorCalibration: depth and color are CameraIntrinsics")
        T = np.array(depth_to_color, dtype=np.float64)
        if T.shape != (4, 4) or not np.all(np.isfinite(T)):
            raise ValueError("SensorCalibration: depth_to_color is a finite 4x4 matrix")
        self.depth, self.color, self.depth_to_color = depth, color, T
        self._table = None
        self._color_table = None

    def xy_table(self):
        """the depth camera's ray table, float32 (H * W, 2) on the device (ops.xy_table), computed once"""
        if self._table is None:
            self._table = ops.xy_table(self.depth)
        return self._table

    def color_xy_table(self):
        """the colour camera's ray table, float32 (Hc * Wc, 2) on the device, computed once: with it warp_depth's image goes into
        ops.unproject_u16 / ops.depth_to_cloud beside the raw colour image"""
        if self._color_table is None:
            self._color_table = ops.xy_table(self.color)
        return self._color_table

    def warp_depth(self, depth, max_gap_mm):
        """depth uint16 (H * W,) -> uint16 (Hc, Wc): the depth image seen from the colour camera, 0 where the depth camera saw nothing
        (AC21, ops.depth_to_color).  max_gap_mm: triangles of the depth mesh whose vertices differ by more than this in depth are not
        drawn.  No default: it depends on the scene and the rig, and nothing in this project measures it."""
        return _warp([self], depth, max_gap_mm)[0]

    def register_color(self, depth, color, occlusion_mm=None, max_gap_mm=None):
        """depth uint16 (n_px,), color uint8 (Hc, Wc, 3) -> uint8 (n_px, 3) in the depth camera's pixel grid, bilinear.  By default
        without an occlusion test (ops.color_to_depth).  occlusion_mm (with max_gap_mm, see warp_depth): the depth image is warped
        into the colour camera first, and a depth pixel that lies more than occlusion_mm behind what the colour camera sees at its
        place is zero.  Neither has a default value: both depend on the scene and the rig, and nothing in this project measures them."""
        return _register([self], depth, color, "bilinear", 1, None, occlusion_mm, max_gap_mm)[0]

    def register_mask(self, depth, mask, occlusion_mm=None, max_gap_mm=None):
        """depth uint16 (n_px,), mask uint8 (Hc, Wc) taken on the colour image -> uint8 (n_px,), nearest pixel; occlusion_mm and
        max_gap_mm as in register_color"""
        return _register([self], depth, mask, "nearest", 1, None, occlusion_mm, max_gap_mm)[0]

    def undistorted(self, fit="same"):
        """the SensorCalibration of the undistorted images: both cameras distortion-free (CameraIntrinsics.undistorted(fit)), the same
        depth_to_color -- undistortion moves neither camera"""
        return SensorCalibration(self.depth.undistorted(fit), self.color.undistorted(fit), self.depth_to_color)

    def undistort_depth(self, depth, interpolation="nearest", max_gap_mm=None, pinhole=None):
        """depth uint16 (H * W,) or (H, W) -> uint16 (H', W') as the camera `pinhole` (default: depth.undistorted()) sees it (AC22,
        ops.remap_depth).  "nearest" copies depth values; "bilinear" blends the four neighbours unless one is 0 or they differ by more
        than max_gap_mm, which it then needs (no default, as in warp_depth)."""
        return _undistort([self], "depth", depth, interpolation, pinhole, True, depth=True, max_gap_mm=max_gap_mm)[0]

    def undistort_color(self, color, pinhole=None):
        """color uint8 (Hc, Wc, 3) -> uint8 (H', W', 3) as the camera `pinhole` (default: color.undistorted()) sees it, bilinear"""
        return _undistort([self], "color", color, "bilinear", pinhole, True, channels=3)[0]

    def undistort_mask(self, mask, camera="color", pinhole=None):
        """mask uint8 (H, W) taken on the image of `camera` ("color" or "depth") -> uint8 (H', W'), nearest pixel"""
        return _undistort([self], camera, mask, "nearest", pinhole, True)[0]

    def to_dict(self):
        return {"depth": self.depth.to_dict(), "color": self.color.to_dict(), "depth_to_color": self.depth_to_color.tolist()}

    @classmethod
    def from_dict(cls, d):
        return cls(CameraIntrinsics.from_dict(d["depth"]), CameraIntrinsics.from_dict(d["color"]), d["depth_to_color"])

    def save(self, path):
        """plain JSON of the fields (Python writes the shortest decimal that reads back as the same double: the round trip is exact)"""
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=1)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls.from_dict(json.load(f))

    def __eq__(self, other):
        return isinstance(other, SensorCalibration) and self.to_dict() == other.to_dict()


class SensorRig:
    """The sensors of a rig, in the order of the frames' sensor axis."""

    def __init__(self, calibrations):
        self.calibrations = list(calibrations)
        if not self.calibrations or not all(isinstance(c, SensorCalibration) for c in self.calibrations):
            raise TypeError("SensorRig: a non-empty list of SensorCalibration")
        n = {(c.depth.width, c.depth.height) for c in self.calibrations}
        if len(n) != 1:
            raise ValueError(f"SensorRig: the depth cameras differ in size: {sorted(n)}")
        self._tables = None
        self._maps = {}

    def __len__(self):
        return len(self.calibrations)

    def xy_tables(self):
        """float32 (S, n_px, 2) on the device: one table per sensor (the batched kpx_depth_to_cloud / frame step take ONE table: a
        rig of distinct lenses calls them once per sensor)"""
        if self._tables is None:
            import torch
            self._tables = torch.stack([c.xy_table() for c in self.calibrations])
        return self._tables

    def warp_depths(self, depth, max_gap_mm):
        """depth uint16 (F, H * W), frame f of sensor f % S -> uint16 (F, Hc, Wc): every frame's depth image seen from its colour camera
        (SensorCalibration.warp_depth, one call for the batch).  The colour cameras must be of one size: ValueError otherwise."""
        return _warp(self.calibrations, depth, max_gap_mm, self)

    def register_colors(self, depth, colors, occlusion_mm=None, max_gap_mm=None):
        """depth uint16 (S, n_px) -- or (F, n_px) with S dividing F, frame f of sensor f % S --, colors uint8 (F, Hc, Wc, 3) ->
        uint8 (F, n_px, 3): every sensor's colour image in its depth camera's grid, one launch; occlusion_mm and max_gap_mm as in
        SensorCalibration.register_color (the warp and the registration are two calls with no host synchronisation between them)"""
        return _register(self.calibrations, depth, colors, "bilinear", None, self, occlusion_mm, max_gap_mm)

    def register_masks(self, depth, masks, occlusion_mm=None, max_gap_mm=None):
        """as register_colors for uint8 (F, Hc, Wc) masks / label images, nearest pixel -> uint8 (F, n_px)"""
        return _register(self.calibrations, depth, masks, "nearest", None, self, occlusion_mm, max_gap_mm)

    def common_pinhole(self, camera="depth", fit="inside"):
        """one distortion-free CameraIntrinsics for `camera` ("depth" or "color") of every sensor, of the cameras' size: fitted to the
        intersection (fit="inside") or the union ("all") of the sensors' view rectangles (CameraIntrinsics.view_rectangle) -- the one
        PinholeCameraIntrinsic the batched consumers (integrate_frames, carve_depth_maps) take"""
        cams = _cameras(self.calibrations, camera)
        rects = np.array([c.view_rectangle(fit) for c in cams])
        lo, hi = (rects.max(0), rects.min(0)) if fit == "inside" else (rects.min(0), rects.max(0))
        return CameraIntrinsics.from_view_rectangle((lo[0], hi[1], lo[2], hi[3]), cams[0].width, cams[0].height, min(c.metric_radius for c in cams))

    def undistort_maps(self, camera="depth", pinhole=None):
        """float32 (S, H', W', 2) on the device: every sensor's map to the one target `pinhole` (default: common_pinhole(camera)),
        stacked once per target"""
        target = self.common_pinhole(camera) if pinhole is None else pinhole
        key = (camera, tuple(tuple(c.packed()) for c in _cameras(self.calibrations, camera)), _target_key(target))
        if key not in self._maps:
            import torch
            self._maps[key] = torch.stack([c.undistort_map(target) for c in _cameras(self.calibrations, camera)])
        return self._maps[key]

    def undistort_depths(self, depth, interpolation="nearest", max_gap_mm=None, pinhole=None):
        """depth uint16 (F, H * W) or (F, H, W), frame f of sensor f % S -> uint16 (F, H', W') as the one camera `pinhole` (default:
        common_pinhole("depth")) sees them; one launch for the batch (SensorCalibration.undistort_depth)"""
        return _undistort(self.calibrations, "depth", depth, interpolation, pinhole, False, self, depth=True, max_gap_mm=max_gap_mm)

    def undistort_colors(self, colors, pinhole=None, camera="color", interpolation="bilinear"):
        """colors uint8 (F, H, W, 3) taken on `camera`'s image -> uint8 (F, H', W', 3) as `pinhole` (default: common_pinhole(camera))
        sees them.  Colours already registered into the depth grid (register_colors) are (F, H * W, 3) with camera="depth"; their
        zero holes want interpolation="nearest" (bilinear would blend them in)."""
        return _undistort(self.calibrations, camera, colors, interpolation, pinhole, False, self, channels=3)

    def undistort_masks(self, masks, camera="color", pinhole=None):
        """masks uint8 (F, H, W) taken on `camera`'s image -> uint8 (F, H', W'), nearest pixel"""
        return _undistort(self.calibrations, camera, masks, "nearest", pinhole, False, self)


def _target_key(target):
    if hasattr(target, "packed"):
        return (int(target.width), int(target.height)) + tuple(target.packed())
    return (int(target.width), int(target.height)) + tuple(np.asarray(target.intrinsic_matrix, dtype=np.float64).reshape(-1))


def _cameras(cals, camera):
    if camera not in ("depth", "color"):
        raise ValueError(f'camera must be "depth" or "color", got {camera!r}')
    cams = [getattr(c, camera) for c in cals]
    sizes = {(c.width, c.height) for c in cams}
    if len(sizes) != 1:
        raise ValueError(f"undistort: the {camera} cameras differ in size: {sorted(sizes)}")
    return cams


def _undistort(cals, camera, image, interpolation, pinhole, single, rig=None, channels=None, depth=False, max_gap_mm=None):
    """the images of `camera` resampled to `pinhole`: uint16 depth images (depth=True) or uint8 images of `channels` channels (None: no
    channel axis).  Everything is checked before the maps are asked for (the first device call)."""
    import torch
    cams = _cameras(cals, camera)
    w, h = cams[0].width, cams[0].height
    img = image if isinstance(image, torch.Tensor) else np.asarray(image)
    if depth and interpolation == "bilinear" and max_gap_mm is None:
        raise ValueError("undistort: the bilinear depth mode needs max_gap_mm (no default: it depends on the scene and the rig)")
    tail = () if channels is None else (channels,)
    shape = tuple(int(n) for n in img.shape)
    lead = shape[:1] if not single else ()
    if shape not in (lead + (h, w) + tail, lead + (h * w,) + tail):
        raise ValueError(f"undistort: the image is {shape}, expected {lead + (h, w) + tail} for the {w} x {h} {camera} camera"
                         + ("" if single else f" (F frames first, frame f of sensor f % {len(cals)})"))
    if not single and shape[0] % len(cals) != 0:
        raise ValueError(f"undistort: {len(cals)} sensors do not divide {shape[0]} frames")
    img = img.reshape(((1,) if single else lead) + (h, w) + tail)
    if rig is not None:
        maps = rig.undistort_maps(camera, pinhole)
    else:
        maps = cams[0].undistort_map(pinhole)
    if depth:
        return ops.remap_depth(img, maps, interpolation, max_gap_mm)
    return ops.remap(img, maps, interpolation)


def _tables(cals, rig):
    """the depth cameras' tables (a rig keeps its stack), asked for only once the arguments have been checked"""
    if rig is not None:
        return rig.xy_tables()
    import torch
    return torch.stack([c.xy_table() for c in cals]) if len(cals) > 1 else cals[0].xy_table()


def _warp(cals, depth, max_gap_mm, rig=None, tables=None):
    sizes = {(c.color.width, c.color.height) for c in cals}
    if len(sizes) != 1:
        raise ValueError(f"warp: the colour cameras differ in size: {sorted(sizes)}")
    if max_gap_mm is None:
        raise ValueError("warp: max_gap_mm is required (no default: it depends on the scene and the rig)")
    d = cals[0].depth
    return ops.depth_to_color(depth, _tables(cals, rig) if tables is None else tables, d.width, d.height, cals, max_gap_mm)


def _register(cals, depth, image, interpolation, frames, rig=None, occlusion_mm=None, max_gap_mm=None):
    import torch
    if occlusion_mm is None and max_gap_mm is not None:
        raise ValueError("register: max_gap_mm belongs to the occlusion test: give occlusion_mm too")
    if occlusion_mm is not None and max_gap_mm is None:
        raise ValueError("register: occlusion_mm needs max_gap_mm (the depth image is warped into the colour camera first)")
    img = image if isinstance(image, torch.Tensor) else np.asarray(image)
    want = 3 if interpolation == "nearest" else 4         # dimensions of a batch
    if frames == 1 and img.ndim == want - 1:
        img = img[None]
    if img.ndim != want:
        raise ValueError(f"register: the image batch has {img.ndim} dimensions, expected {want}")
    tables = _tables(cals, rig)
    if occlusion_mm is None:
        return ops.color_to_depth(depth, tables, img, cals, interpolation)
    depth = ops._dev(depth, torch.uint16)                 # (both calls read it: a host array goes to the device once)
    warped = _warp(cals, depth, max_gap_mm, rig, tables)
    return ops.color_to_depth(depth, tables, img, cals, interpolation, warped=warped, occlusion_mm=occlusion_mm)

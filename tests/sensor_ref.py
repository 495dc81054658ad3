"""Float64 NumPy restatement of arithmetic contract AC20 (include/kinectpx.h) -- TEST INFRASTRUCTURE ONLY.

Written from the contract's text, not from the product: the forward map, the Newton inverse, the ray table and the two samplers,
elementwise on arrays.  NumPy evaluates every multiply, add and divide as one IEEE operation and fuses nothing, so an implementation
that keeps the contract's order of operations agrees with this file bit for bit.

A camera here is a plain tuple cam = (fx, fy, cx, cy, k1, k2, k3, k4, k5, k6, p1, p2, metric_radius) of Python floats.
"""
import numpy as np

ROUNDS = 21
STOP = 1e-22


def cam_of(intr):
    """anything with the fifteen AC20 attributes -> the tuple"""
    return tuple(float(getattr(intr, n)) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2", "metric_radius"))


def distort(cam, x, y):
    _, _, _, _, k1, k2, k3, k4, k5, k6, p1, p2, _ = cam
    xx = x * x
    yy = y * y
    r2 = xx + yy
    r4 = r2 * r2
    r6 = r4 * r2
    num = 1.0 + k1 * r2
    num = num + k2 * r4
    num = num + k3 * r6
    den = 1.0 + k4 * r2
    den = den + k5 * r4
    den = den + k6 * r6
    radial = num / den
    xy2 = 2.0 * (x * y)
    xd = x * radial + p1 * xy2
    xd = xd + p2 * (r2 + 2.0 * xx)
    yd = y * radial + p1 * (r2 + 2.0 * yy)
    yd = yd + p2 * xy2
    return xd, yd, dict(r2=r2, r4=r4, num=num, den=den, radial=radial)


def forward_normalised(cam, x, y):
    """(x, y) = (X / Z, Y / Z) -> u, v, valid"""
    fx, fy, cx, cy = cam[:4]
    mr = cam[12]
    with np.errstate(all="ignore"):
        xd, yd, t = distort(cam, x, y)
        u = fx * xd + cx
        v = fy * yd + cy
        return u, v, t["r2"] <= mr * mr


def forward(cam, X, Y, Z):
    with np.errstate(all="ignore"):
        return forward_normalised(cam, X / Z, Y / Z)


def jacobian(cam, x, y, t):
    _, _, _, _, k1, k2, k3, k4, k5, k6, p1, p2, _ = cam
    r2, r4, num, den, radial = t["r2"], t["r4"], t["num"], t["den"], t["radial"]
    nd = k1 + (2.0 * k2) * r2
    nd = nd + (3.0 * k3) * r4
    dd = k4 + (2.0 * k5) * r2
    dd = dd + (3.0 * k6) * r4
    dr = (nd * den - num * dd) / (den * den)
    gx = (2.0 * x) * dr
    gy = (2.0 * y) * dr
    a = radial + x * gx
    a = a + (2.0 * p1) * y
    a = a + (6.0 * p2) * x
    b = x * gy + (2.0 * p1) * x
    b = b + (2.0 * p2) * y
    c = y * gx + (2.0 * p1) * x
    c = c + (2.0 * p2) * y
    d = radial + y * gy
    d = d + (6.0 * p1) * y
    d = d + (2.0 * p2) * x
    return a, b, c, d


def inverse(cam, u, v):
    """pixel coordinates (float64 arrays of one shape) -> x, y (NaN where there is no ray).  Every element runs its own Newton
    iteration: an element that has converged or stopped is left alone from then on."""
    fx, fy, cx, cy = cam[:4]
    mr = cam[12]
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        xn = (u - cx) / fx
        yn = (v - cy) / fy
        x = xn.copy()
        y = yn.copy()
        running = np.ones(u.shape, dtype=bool)
        converged = np.zeros(u.shape, dtype=bool)
        for rnd in range(ROUNDS):
            xd, yd, t = distort(cam, x, y)
            ex = xd - xn
            ey = yd - yn
            hit = running & (ex * ex + ey * ey <= STOP)
            converged |= hit
            running &= ~hit
            if rnd == ROUNDS - 1 or not running.any():
                break
            a, b, c, d = jacobian(cam, x, y, t)
            det = a * d - b * c
            running &= np.isfinite(det) & (det != 0.0)
            nx = x - (d * ex - b * ey) / det
            ny = y - (a * ey - c * ex) / det
            x = np.where(running, nx, x)
            y = np.where(running, ny, y)
        ok = converged & np.isfinite(x) & np.isfinite(y) & (x * x + y * y <= mr * mr)
    return np.where(ok, x, np.nan), np.where(ok, y, np.nan)


def xy_table(cam, width, height):
    """float32 (height * width, 2): the inverse at every pixel centre, rounded once"""
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    x, y = inverse(cam, u.reshape(-1), v.reshape(-1))
    return np.stack([x, y], -1).astype(np.float32)


def color_to_depth(depth, xy, color, calibrations, interpolation, want_classes=False):
    """depth u16 (F, n_px), xy f32 (S, n_px, 2), color u8 (F, Hc, Wc, C), calibrations S pairs (cam tuple, 4x4) -> u8 (F, n_px, C).
    want_classes: also a dict of boolean (F, n_px) masks naming why a pixel is zero / what its sample touched."""
    depth = np.asarray(depth)
    F, n_px = depth.shape
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, n_px, 2)
    S = len(calibrations)
    assert xy.shape[0] == S and F % S == 0
    color = np.asarray(color)
    _, hc, wc, C = color.shape
    out = np.zeros((F, n_px, C), np.uint8)
    names = ("zero_depth", "nan_table", "behind", "beyond_radius", "outside", "left", "right", "top", "bottom", "sampled")
    cls = {k: np.zeros((F, n_px), bool) for k in names}
    for f in range(F):
        cam, T = calibrations[f % S]
        T = np.asarray(T, dtype=np.float64)
        d = depth[f].astype(np.float64)
        xt = xy[f % S, :, 0].astype(np.float64)
        yt = xy[f % S, :, 1].astype(np.float64)
        with np.errstate(all="ignore"):
            px = xt * d
            py = yt * d
            pz = d
            q = [((T[i, 0] * px + T[i, 1] * py) + T[i, 2] * pz) + T[i, 3] for i in range(3)]
            uc, vc, inside_radius = forward(cam, q[0], q[1], q[2])
            zero = depth[f] == 0
            nan = ~zero & (np.isnan(xt) | np.isnan(yt))
            behind = ~zero & ~nan & ~(q[2] > 0.0)
            beyond = ~zero & ~nan & ~behind & ~inside_radius
            live = ~(zero | nan | behind | beyond)
            if interpolation == "nearest":
                ix = np.floor(uc + 0.5)
                iy = np.floor(vc + 0.5)
                inside = (ix >= 0.0) & (ix <= wc - 1.0) & (iy >= 0.0) & (iy <= hc - 1.0)
                take = live & inside
                jx = ix[take].astype(np.int64)
                jy = iy[take].astype(np.int64)
                out[f, take] = color[f, jy, jx]
                touched = {"left": ix == 0.0, "right": ix == wc - 1.0, "top": iy == 0.0, "bottom": iy == hc - 1.0}
            else:
                x0 = np.floor(uc)
                y0 = np.floor(vc)
                inside = (x0 >= 0.0) & (x0 <= wc - 2.0) & (y0 >= 0.0) & (y0 <= hc - 2.0)
                take = live & inside
                jx = x0[take].astype(np.int64)
                jy = y0[take].astype(np.int64)
                ax = (uc - x0)[take][:, None]
                ay = (vc - y0)[take][:, None]
                bx = 1.0 - ax
                by = 1.0 - ay
                c00 = color[f, jy, jx].astype(np.float64)
                c10 = color[f, jy, jx + 1].astype(np.float64)
                c01 = color[f, jy + 1, jx].astype(np.float64)
                c11 = color[f, jy + 1, jx + 1].astype(np.float64)
                val = (bx * by) * c00 + (ax * by) * c10
                val = val + (bx * ay) * c01
                val = val + (ax * ay) * c11
                out[f, take] = np.floor(val + 0.5).astype(np.uint8)
                # neighbours straddling a border: one column / row of the 2 x 2 block inside the image, the other outside
                touched = {"left": x0 == -1.0, "right": x0 == wc - 1.0, "top": y0 == -1.0, "bottom": y0 == hc - 1.0}
            cls["zero_depth"][f], cls["nan_table"][f], cls["behind"][f], cls["beyond_radius"][f] = zero, nan, behind, beyond
            cls["outside"][f] = live & ~inside
            cls["sampled"][f] = take
            for k, m in touched.items():
                cls[k][f] = live & m
    return (out, cls) if want_classes else out

"""Float64 NumPy restatement of arithmetic contract AC21 (include/kinectpx.h) -- TEST INFRASTRUCTURE ONLY.

Written from the contract's text, not from the product: the vertices (AC20's "colour -> depth" chain through tests/sensor_ref.py's
`forward`), the two triangles of every 2 x 2 block, the tests that skip a triangle, the pixel walk over the bounding box -- vectorised
over triangles, a 16 x 16 loop over the offsets inside the box -- and the minimum per colour pixel (np.minimum.at: a minimum does
not depend on the order of the triangles, which `reverse` lets a test see).  NumPy evaluates every multiply, add and divide as one
IEEE operation and fuses nothing.

A calibration here is a pair (cam, T): sensor_ref's camera tuple of the colour camera and the 4x4 depth -> colour transform.
"""
import numpy as np

from tests import sensor_ref as R

MAX_SPAN = 16                     # KPX_WARP_MAX_SPAN
TRIANGLE_CLASSES = ("invalid_vertex", "gap", "span", "flat", "drawn")


def calibrations_of(cals):
    """objects with .color and .depth_to_color -> the pairs"""
    return [(R.cam_of(c.color), np.asarray(c.depth_to_color, dtype=np.float64)) for c in cals]


def vertices(depth, xy, cal):
    """depth u16 (n,), xy f32 (n, 2) -> u, v, z (float64 (n,)) and valid (bool (n,))"""
    cam, T = cal
    T = np.asarray(T, dtype=np.float64)
    d = depth.astype(np.float64)
    xt = xy[:, 0].astype(np.float64)
    yt = xy[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        px = xt * d
        py = yt * d
        pz = d
        q = [((T[i, 0] * px + T[i, 1] * py) + T[i, 2] * pz) + T[i, 3] for i in range(3)]
        u, v, inside_radius = R.forward(cam, q[0], q[1], q[2])
        valid = (depth != 0) & ~np.isnan(xt) & ~np.isnan(yt) & (q[2] > 0.0) & inside_radius
    return u, v, q[2], valid


def edge(au, av, bu, bv, pu, pv):
    return (bu - au) * (pv - av) - (bv - av) * (pu - au)


def triangle_indices(width, height):
    """(3, n_triangles) pixel indices: for every quad in row-major order its triangle A, then its triangle B"""
    r, c = np.meshgrid(np.arange(height - 1), np.arange(width - 1), indexing="ij")
    p = (r * width + c).reshape(-1)
    a = np.stack([p, p + 1, p + width])
    b = np.stack([p + width + 1, p + width, p + 1])
    return np.stack([a, b], -1).reshape(3, -1)


def warp_frame(depth, xy, width, height, cal, wc, hc, max_gap_mm, reverse=False):
    """one frame -> warped u16 (hc, wc), classes {name: bool (n_triangles,)}, hits int (hc, wc), spread bool (hc, wc): the pixel was
    reached with different zi"""
    zbuf = np.full((hc, wc), 0xFFFFFFFF, np.uint32)
    zmax = np.zeros((hc, wc), np.uint32)
    hits = np.zeros((hc, wc), np.int64)
    if width < 2 or height < 2:
        none = np.zeros(0, bool)
        return np.zeros((hc, wc), np.uint16), {k: none for k in TRIANGLE_CLASSES}, hits, zmax != 0
    u, v, z, valid = vertices(depth, xy, cal)
    tri = triangle_indices(width, height)
    if reverse:
        tri = tri[:, ::-1]
    with np.errstate(all="ignore"):
        (u0, u1, u2), (v0, v1, v2), (z0, z1, z2) = u[tri], v[tri], z[tri]
        invalid = ~(valid[tri[0]] & valid[tri[1]] & valid[tri[2]])
        zhi = np.maximum(np.maximum(z0, z1), z2)
        zlo = np.minimum(np.minimum(z0, z1), z2)
        gap = ~invalid & (zhi - zlo > max_gap_mm)
        bx0 = np.ceil(np.minimum(np.minimum(u0, u1), u2))
        bx1 = np.floor(np.maximum(np.maximum(u0, u1), u2))
        by0 = np.ceil(np.minimum(np.minimum(v0, v1), v2))
        by1 = np.floor(np.maximum(np.maximum(v0, v1), v2))
        span = ~invalid & ~gap & ((bx1 - bx0 >= MAX_SPAN) | (by1 - by0 >= MAX_SPAN))
        area = edge(u0, v0, u1, v1, u2, v2)
        flat = ~invalid & ~gap & ~span & ((area == 0.0) | ~np.isfinite(area))
        drawn = ~(invalid | gap | span | flat)
        k = np.nonzero(drawn)[0]
        u0, u1, u2, v0, v1, v2, z0, z1, z2 = (a[k] for a in (u0, u1, u2, v0, v1, v2, z0, z1, z2))
        bx0, bx1, by0, by1, area = bx0[k], bx1[k], by0[k], by1[k], area[k]
        for dy in range(MAX_SPAN):
            y = by0 + dy
            for dx in range(MAX_SPAN):
                x = bx0 + dx
                inbox = (x <= bx1) & (y <= by1) & (x >= 0.0) & (x <= wc - 1.0) & (y >= 0.0) & (y <= hc - 1.0)
                if not inbox.any():
                    continue
                w0 = edge(u1, v1, u2, v2, x, y)
                w1 = edge(u2, v2, u0, v0, x, y)
                w2 = edge(u0, v0, u1, v1, x, y)
                inside = np.where(area > 0.0, (w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0), (w0 <= 0.0) & (w1 <= 0.0) & (w2 <= 0.0))
                s = (w0 + w1) + w2
                zz = ((w0 * z0 + w1 * z1) + w2 * z2) / s
                zi = np.floor(zz + 0.5)
                ok = inbox & inside & (s != 0.0) & (zi >= 1.0) & (zi <= 65535.0)
                jy, jx, val = y[ok].astype(np.int64), x[ok].astype(np.int64), zi[ok].astype(np.uint32)
                np.minimum.at(zbuf, (jy, jx), val)
                np.maximum.at(zmax, (jy, jx), val)
                np.add.at(hits, (jy, jx), 1)
    out = np.where(zbuf == 0xFFFFFFFF, 0, zbuf).astype(np.uint16)
    classes = dict(invalid_vertex=invalid, gap=gap, span=span, flat=flat, drawn=drawn)
    return out, classes, hits, (hits > 1) & (zmax != zbuf)


def depth_to_color(depth, xy, width, height, calibrations, wc, hc, max_gap_mm, want_classes=False, reverse=False):
    """depth u16 (F, height * width), xy f32 (S, height * width, 2), calibrations S pairs -> u16 (F, hc, wc); want_classes: also
    {name: bool (F, n_triangles)}, hits (F, hc, wc), spread (F, hc, wc)"""
    depth = np.asarray(depth).reshape(-1, width * height)
    F, S = depth.shape[0], len(calibrations)
    xy = np.asarray(xy, dtype=np.float32).reshape(S, width * height, 2)
    assert F % S == 0
    res = [warp_frame(depth[f], xy[f % S], width, height, calibrations[f % S], wc, hc, max_gap_mm, reverse) for f in range(F)]
    out = np.stack([r[0] for r in res]) if F else np.zeros((0, hc, wc), np.uint16)
    if not want_classes:
        return out
    cls = {k: np.stack([r[1][k] for r in res]) for k in TRIANGLE_CLASSES}
    return out, cls, np.stack([r[2] for r in res]), np.stack([r[3] for r in res])


def visible(depth, xy, color, calibrations, interpolation, warped, occlusion_mm):
    """AC20's registration (sensor_ref.color_to_depth) with AC21's occlusion test -> u8 (F, n_px, C), occluded bool (F, n_px)"""
    depth = np.asarray(depth)
    F, n_px = depth.shape
    S = len(calibrations)
    xy = np.asarray(xy, dtype=np.float32).reshape(S, n_px, 2)
    out, cls = R.color_to_depth(depth, xy, color, calibrations, interpolation, want_classes=True)
    out = out.copy()
    warped = np.asarray(warped).reshape(F, color.shape[1], color.shape[2])
    occluded = np.zeros((F, n_px), bool)
    for f in range(F):
        u, v, z, _ = vertices(depth[f], xy[f % S], calibrations[f % S])
        take = cls["sampled"][f]
        ix = np.floor(u[take] + 0.5).astype(np.int64)
        iy = np.floor(v[take] + 0.5).astype(np.int64)
        w = warped[f, iy, ix]
        occluded[f, take] = (w != 0) & (z[take] - w.astype(np.float64) > occlusion_mm)
    out[occluded] = 0
    return out, occluded

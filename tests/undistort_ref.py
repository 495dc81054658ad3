"""Float64 NumPy restatement of arithmetic contract AC22 (include/kinectpx.h) -- TEST INFRASTRUCTURE ONLY.

Written from the contract's text on top of tests/sensor_ref.py (AC20's `distort` and sampling rules): the map of a distortion-free
target camera into a lens's image, and the u8 and depth images resampled through stored maps.  NumPy evaluates every multiply, add
and divide as one IEEE operation and fuses nothing, so an implementation that keeps the contract's order agrees with this file bit
for bit.

A camera is sensor_ref's tuple; a pinhole target is (fx', fy', cx', cy').  Every remap also returns a dict of boolean masks, one
class per output pixel: `nan_map`, `outside` (the sample has no place in the source image), `sampled`; the four borders
`outside_left` / `_right` / `_top` / `_bottom` name the outside pixels whose sample straddles that border -- nearest: the pixel just
beyond it; bilinear: one column / row of the 2 x 2 block inside the image, the other beyond it.  Depth bilinear splits `sampled`
further: `zero_neighbour`, `gap`, and `sampled` is what is left.
"""
import numpy as np

from tests import sensor_ref as R


def pinhole_of(intr):
    return tuple(float(getattr(intr, n)) for n in ("fx", "fy", "cx", "cy"))


def undistort_map(cam, pinhole, out_width, out_height):
    """-> float32 (out_height, out_width, 2)"""
    fxp, fyp, cxp, cyp = pinhole
    fx, fy, cx, cy = cam[:4]
    mr = cam[12]
    r, c = np.meshgrid(np.arange(out_height, dtype=np.float64), np.arange(out_width, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        x = (c - cxp) / fxp
        y = (r - cyp) / fyp
        xd, yd, t = R.distort(cam, x, y)
        u = fx * xd + cx
        v = fy * yd + cy
        bad = (t["r2"] > mr * mr) | ~np.isfinite(u) | ~np.isfinite(v)
        out = np.stack([u, v], -1).astype(np.float32)
    out[bad] = np.nan
    return out


def _place(maps, f, ws, hs, interpolation):
    """the sample positions of frame f: uc, vc (float64), the integer corner (x0, y0), the masks nan / inside / borders"""
    m = maps[f % maps.shape[0]]
    uc = m[..., 0].astype(np.float64)
    vc = m[..., 1].astype(np.float64)
    nan = np.isnan(uc) | np.isnan(vc)
    with np.errstate(all="ignore"):
        if interpolation == "nearest":
            x0 = np.floor(uc + 0.5)
            y0 = np.floor(vc + 0.5)
            inside = (x0 >= 0.0) & (x0 <= ws - 1.0) & (y0 >= 0.0) & (y0 <= hs - 1.0)
            borders = {"outside_left": x0 == -1.0, "outside_right": x0 == ws, "outside_top": y0 == -1.0, "outside_bottom": y0 == hs}
        else:
            x0 = np.floor(uc)
            y0 = np.floor(vc)
            inside = (x0 >= 0.0) & (x0 <= ws - 2.0) & (y0 >= 0.0) & (y0 <= hs - 2.0)
            borders = {"outside_left": x0 == -1.0, "outside_right": x0 == ws - 1.0, "outside_top": y0 == -1.0, "outside_bottom": y0 == hs - 1.0}
    return uc, vc, x0, y0, nan, inside & ~nan, {k: b & ~nan for k, b in borders.items()}


def _bilinear(img, jy, jx, ax, ay):
    """AC20's val for the 2 x 2 blocks at (jy, jx): img (H, W) or (H, W, C), ax / ay broadcast against the channel axis"""
    bx = 1.0 - ax
    by = 1.0 - ay
    c00 = img[jy, jx].astype(np.float64)
    c10 = img[jy, jx + 1].astype(np.float64)
    c01 = img[jy + 1, jx].astype(np.float64)
    c11 = img[jy + 1, jx + 1].astype(np.float64)
    val = (bx * by) * c00 + (ax * by) * c10
    val = val + (bx * ay) * c01
    val = val + (ax * ay) * c11
    return np.floor(val + 0.5), (c00, c10, c01, c11)


def _maps4(maps):
    maps = np.asarray(maps, dtype=np.float32)
    return maps[None] if maps.ndim == 3 else maps


def remap_u8(src, maps, interpolation):
    """src u8 (F, Hs, Ws, C), maps f32 (M, Ho, Wo, 2) or (Ho, Wo, 2) -> u8 (F, Ho, Wo, C), classes (F, Ho, Wo)"""
    src = np.asarray(src)
    maps = _maps4(maps)
    F, hs, ws, C = src.shape
    M, ho, wo, _ = maps.shape
    assert F % M == 0 and interpolation in ("nearest", "bilinear")
    out = np.zeros((F, ho, wo, C), np.uint8)
    names = ("nan_map", "outside", "outside_left", "outside_right", "outside_top", "outside_bottom", "sampled")
    cls = {k: np.zeros((F, ho, wo), bool) for k in names}
    for f in range(F):
        uc, vc, x0, y0, nan, take, borders = _place(maps, f, ws, hs, interpolation)
        jx = x0[take].astype(np.int64)
        jy = y0[take].astype(np.int64)
        if interpolation == "nearest":
            out[f][take] = src[f, jy, jx]
        else:
            val, _ = _bilinear(src[f], jy, jx, (uc - x0)[take][:, None], (vc - y0)[take][:, None])
            out[f][take] = val.astype(np.uint8)
        cls["nan_map"][f], cls["sampled"][f], cls["outside"][f] = nan, take, ~nan & ~take
        for k, b in borders.items():
            cls[k][f] = b & ~take
    return out, cls


def remap_depth(src, maps, interpolation, max_gap_mm=None):
    """src u16 (F, Hs, Ws) -> u16 (F, Ho, Wo), classes (F, Ho, Wo); max_gap_mm is read by the bilinear mode only"""
    src = np.asarray(src)
    maps = _maps4(maps)
    F, hs, ws = src.shape
    M, ho, wo, _ = maps.shape
    assert F % M == 0 and interpolation in ("nearest", "bilinear")
    out = np.zeros((F, ho, wo), np.uint16)
    names = ("nan_map", "outside", "outside_left", "outside_right", "outside_top", "outside_bottom", "zero_neighbour", "gap", "sampled")
    cls = {k: np.zeros((F, ho, wo), bool) for k in names}
    for f in range(F):
        uc, vc, x0, y0, nan, take, borders = _place(maps, f, ws, hs, interpolation)
        jx = x0[take].astype(np.int64)
        jy = y0[take].astype(np.int64)
        cls["nan_map"][f], cls["outside"][f] = nan, ~nan & ~take
        for k, b in borders.items():
            cls[k][f] = b & ~take
        if interpolation == "nearest":
            out[f][take] = src[f, jy, jx]
            cls["sampled"][f] = take
            continue
        val, four = _bilinear(src[f], jy, jx, (uc - x0)[take], (vc - y0)[take])
        four = np.stack(four)
        zero = (four == 0.0).any(0)
        gap = ~zero & (four.max(0) - four.min(0) > float(max_gap_mm))
        keep = ~zero & ~gap
        out[f][take] = np.where(keep, val, 0.0).astype(np.uint16)
        for k, m in (("zero_neighbour", zero), ("gap", gap), ("sampled", keep)):
            cls[k][f][take] = m
    return out, cls

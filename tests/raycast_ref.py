"""The pinned statement of arithmetic contract AC14: RaycastingScene's ray casts, occlusion tests,
intersection counts and closest points as a literal brute force over every (query, triangle) pair, vectorised in NumPy.  float64
throughout, every multiply and add a separate NumPy operation (NumPy never fuses them), float32 only where the contract rounds; AC3's
fma chain is tests/tsdf_ref.py's exact fused multiply-add.  There is no hierarchy here: every triangle is tested against every query,
ties go to the lowest global triangle index.

The ray side is staged only to bound the work: a pair whose determinant is 0 or whose u lies outside [0, 1] cannot be a hit (u >= 0 is
a clause; v >= 0 and u + v <= 1 imply u <= 1 in floating point too, because rounding is monotone: fl(u + v) >= fl(u + 0) = u), so v, t
and the box clause are evaluated on the remaining pairs alone, with the same arithmetic."""
import numpy as np

import tsdf_mesh_ref as M
from tsdf_ref import fma

OCCUPANCY_DIRECTION = (1.0, 0.375, 0.3125)
PAIRS_PER_CHUNK = 1 << 19


def _err():
    return np.errstate(all="ignore")


def _f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a).astype(np.float32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def ac3(dx, dy, dz):
    """AC3: fma(dz, dz, fma(dy, dy, dx dx))"""
    with _err():
        return fma(dz, dz, fma(dy, dy, dx * dx))


class Scene:
    """geometries: a list of (vertices (V, 3), triangles (T, 3)); concatenated in order, global index g = position in the concatenation"""

    def __init__(self, geometries):
        cs, gid, pid, nrm = [], [], [], []
        for g, (v, t) in enumerate(geometries):
            v = _f32(np.asarray(v).reshape(-1, 3))
            t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
            cs.append(v.astype(np.float64)[t].reshape(-1, 3, 3))
            gid.append(np.full(len(t), g, dtype=np.int32))
            pid.append(np.arange(len(t), dtype=np.int32))
            nrm.append(M.triangle_normals(v, t, True).reshape(-1, 3))
        self.corners = np.concatenate(cs) if cs else np.zeros((0, 3, 3))
        self.geometry_ids = np.concatenate(gid) if gid else np.zeros(0, np.int32)
        self.primitive_ids = np.concatenate(pid) if pid else np.zeros(0, np.int32)
        self.normals = np.concatenate(nrm) if nrm else np.zeros((0, 3), np.float32)
        lo, hi = self.corners.min(1), self.corners.max(1)
        m = np.maximum(np.abs(lo), np.abs(hi)).max(1) if len(lo) else np.zeros(0)
        r = (m * 2.0 ** -20)[:, None]
        self.lo, self.hi = lo - r, hi + r

    def __len__(self):
        return len(self.corners)


def slab(o, d, lo, hi):
    """paired rows -> (meets, tn, tf)"""
    n = len(o)
    tn, tf, ok = np.zeros(n), np.full(n, np.inf), np.ones(n, dtype=bool)
    with _err():
        for k in range(3):
            z = d[:, k] == 0.0
            ok &= ~z | ((lo[:, k] <= o[:, k]) & (o[:, k] <= hi[:, k]))
            i = 1.0 / d[:, k]
            a, b = (lo[:, k] - o[:, k]) * i, (hi[:, k] - o[:, k]) * i
            tn = np.where(z, tn, np.maximum(tn, np.minimum(a, b)))
            tf = np.where(z, tf, np.minimum(tf, np.maximum(a, b)))
        return ok & (tn <= tf), tn, tf


def _rays(rays):
    r = _f32(np.asarray(rays).reshape(-1, 6)).astype(np.float64)
    valid = np.isfinite(r).all(1) & (r[:, 3:] != 0.0).any(1)
    return r[:, :3], r[:, 3:], valid


def hits(scene, rays):
    """every hit of AC14 -> (ray index, global triangle index, t, u, v) as flat arrays ascending in (ray, triangle), and the number of
    plain Moeller-Trumbore hits (det != 0, u >= 0, v >= 0, u + v <= 1, t >= 0) that the box clause removed"""
    o, d, valid = _rays(rays)
    T = len(scene)
    out = [np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0)]
    removed = 0
    if T == 0 or len(o) == 0:
        return tuple(out), removed
    v0 = scene.corners[:, 0]
    e1, e2 = scene.corners[:, 1] - v0, scene.corners[:, 2] - v0
    step = max(1, PAIRS_PER_CHUNK // T)
    parts = []
    rows = np.flatnonzero(valid)
    for c0 in range(0, len(rows), step):
        rr = rows[c0:c0 + step]
        with _err():
            dd, oo = d[rr][:, None, :], o[rr][:, None, :]
            p = _cross(dd, e2[None])
            det = _dot(e1[None], p)
            inv = 1.0 / det
            s = oo - v0[None]
            u = _dot(s, p) * inv
            ri, ti = np.nonzero((det != 0.0) & (u >= 0.0) & (u <= 1.0))
            u, inv, s = u[ri, ti], inv[ri, ti], s[ri, ti]
            dr = d[rr][ri]
            q = _cross(s, e1[ti])
            v = _dot(dr, q) * inv
            t = _dot(e2[ti], q) * inv
            mt = (v >= 0.0) & (u + v <= 1.0)
            meets, tn, tf = slab(o[rr][ri], dr, scene.lo[ti], scene.hi[ti])
            hit = mt & meets & (tn <= t) & (t <= tf)
            removed += int((mt & (t >= 0.0) & ~hit).sum())
        parts.append((rr[ri][hit], ti[hit], t[hit], u[hit], v[hit]))
    if parts:
        out = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    return tuple(out), removed


def cast_rays(scene, rays):
    """-> dict: t float64, t_hit float32, primitive_uvs float32 (R, 2), primitive_normals float32 (R, 3), geometry_ids,
    primitive_ids int32 (-1: miss)"""
    n = len(np.asarray(rays).reshape(-1, 6))
    (ri, ti, t, u, v), _ = hits(scene, rays)
    out = {"t": np.full(n, np.inf), "primitive_uvs": np.zeros((n, 2), np.float32), "primitive_normals": np.zeros((n, 3), np.float32),
           "geometry_ids": np.full(n, -1, np.int32), "primitive_ids": np.full(n, -1, np.int32)}
    order = np.lexsort((ti, t, ri))                               # per ray: ascending t, then ascending global index
    ri, ti, t, u, v = ri[order], ti[order], t[order], u[order], v[order]
    first = np.ones(len(ri), dtype=bool)
    first[1:] = ri[1:] != ri[:-1]
    ri, ti, t, u, v = ri[first], ti[first], t[first], u[first], v[first]
    out["t"][ri] = t
    out["primitive_uvs"][ri] = _f32(np.stack([u, v], 1))
    out["primitive_normals"][ri] = scene.normals[ti]
    out["geometry_ids"][ri] = scene.geometry_ids[ti]
    out["primitive_ids"][ri] = scene.primitive_ids[ti]
    out["t_hit"] = _f32(out["t"])
    return out


def test_occlusions(scene, rays, tnear=0.0, tfar=np.inf):
    n = len(np.asarray(rays).reshape(-1, 6))
    (ri, _, t, _, _), _ = hits(scene, rays)
    out = np.zeros(n, dtype=bool)
    out[ri[(tnear <= t) & (t <= tfar)]] = True
    return out


def count_intersections(scene, rays):
    n = len(np.asarray(rays).reshape(-1, 6))
    (ri, _, _, _, _), _ = hits(scene, rays)
    return np.bincount(ri, minlength=n).astype(np.int32)


def closest_all(scene, queries):
    """-> (D (Q, T) float64 with NaN where the contract's D is NaN, closest points (Q, T, 3), d2 (Q, T), gap2 (Q, T)) for finite queries"""
    q = _f32(np.asarray(queries).reshape(-1, 3)).astype(np.float64)[:, None, :]
    a, b, c = scene.corners[None, :, 0], scene.corners[None, :, 1], scene.corners[None, :, 2]
    with _err():
        ab, ac = b - a, c - a
        qa, qb, qc = q - a, q - b, q - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, qa), _dot(ac, qa), _dot(ab, qb), _dot(ac, qb), _dot(ab, qc), _dot(ac, qc)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        w = 1.0 / ((va + vb) + vc)
        regions = [
            (d1 <= 0.0) & (d2 <= 0.0), a,
            (d3 >= 0.0) & (d4 <= d3), b,
            (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), a + (d1 / (d1 - d3))[..., None] * ab,
            (d6 >= 0.0) & (d5 <= d6), c,
            (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), a + (d2 / (d2 - d6))[..., None] * ac,
            (va <= 0.0) & (d4 - d3 >= 0.0) & (d5 - d6 >= 0.0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b),
        ]
        cp = (a + ab * (vb * w)[..., None]) + ac * (vc * w)[..., None]
        for k in range(len(regions) - 2, -1, -2):
            cp = np.where(regions[k][..., None], np.broadcast_to(regions[k + 1], cp.shape), cp)
        diff = q - cp
        dd = ac3(diff[..., 0], diff[..., 1], diff[..., 2])
        g = np.maximum(0.0, np.maximum(scene.lo[None] - q, q - scene.hi[None]))
        gap = ac3(g[..., 0], g[..., 1], g[..., 2])
        D = np.where(np.isnan(dd), dd, np.maximum(dd, gap))
    return D, cp, dd, gap


def closest_points(scene, queries):
    """-> dict: points float32 (Q, 3), distance float32, d2 float64, geometry_ids, primitive_ids int32; a query with a non-finite
    coordinate has no closest point (NaN and -1)"""
    if len(scene) == 0:
        raise RuntimeError("the scene holds no triangle")
    q = _f32(np.asarray(queries).reshape(-1, 3))
    n = len(q)
    out = {"points": np.full((n, 3), np.nan, np.float32), "d2": np.full(n, np.nan), "geometry_ids": np.full(n, -1, np.int32),
           "primitive_ids": np.full(n, -1, np.int32)}
    rows = np.flatnonzero(np.isfinite(q).all(1))
    step = max(1, (PAIRS_PER_CHUNK // 8) // len(scene))
    for c0 in range(0, len(rows), step):
        rr = rows[c0:c0 + step]
        D, cp, _, _ = closest_all(scene, q[rr])
        best = np.argmin(np.where(np.isnan(D), np.inf, D), 1)      # the first of equal minima: the lowest global index
        Db = D[np.arange(len(rr)), best]
        ok = ~np.isnan(Db)
        rr, best, Db = rr[ok], best[ok], Db[ok]
        out["d2"][rr] = Db
        out["points"][rr] = _f32(cp[np.flatnonzero(ok), best])
        out["geometry_ids"][rr] = scene.geometry_ids[best]
        out["primitive_ids"][rr] = scene.primitive_ids[best]
    with _err():
        out["distance"] = _f32(np.sqrt(out["d2"]))
    return out


def occupancy(scene, queries):
    """-> bool (Q,): count_intersections of the ray (q, OCCUPANCY_DIRECTION) is odd"""
    q = _f32(np.asarray(queries).reshape(-1, 3))
    rays = np.concatenate([q, np.broadcast_to(np.asarray(OCCUPANCY_DIRECTION, np.float32), q.shape)], 1)
    return (count_intersections(scene, rays) & 1).astype(bool)


def signed_distance(scene, queries):
    d = closest_points(scene, queries)["distance"]
    return np.where(occupancy(scene, queries), -d, d).astype(np.float32)


def create_rays_pinhole(K, E, W, H, pixel_center=0.5):
    """origin -(R^T t), direction R^T ((x + c - cx) / fx, (y + c - cy) / fy, 1), fp64 scalars, -> float32 (H, W, 6)"""
    K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
    R, t = E[:3, :3], E[:3, 3]
    out = np.empty((H, W, 6), np.float64)
    for y in range(H):
        for x in range(W):
            a, b = ((x + pixel_center) - K[0, 2]) / K[0, 0], ((y + pixel_center) - K[1, 2]) / K[1, 1]
            for k in range(3):
                out[y, x, k] = -((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2])
                out[y, x, 3 + k] = (R[0, k] * a + R[1, k] * b) + R[2, k]
    return out.astype(np.float32)

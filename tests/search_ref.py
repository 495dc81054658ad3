"""NumPy float64 brute-force reference of the neighbour search: d2 in fp64 from the float32-rounded coordinates,
rows ordered by lexsort on (d2, index).  The plain sum dx^2 + dy^2 + dz^2 equals the library's fma chain bit for bit only where
every product and sum is exact -- quantised coordinates (multiples of 1/16 with |x| <= 4096, or integers): the bitwise tests use
those."""
import numpy as np


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3)).astype(np.float64)


def d2_matrix(pts, queries):
    """(M, N) float64; a query with a non-finite coordinate gets a row of NaN"""
    p, q = _f32(pts), _f32(queries)
    with np.errstate(invalid="ignore", over="ignore"):
        d = q[:, None, :] - p[None, :, :]
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _order(row):
    return np.lexsort((np.arange(len(row)), row))


def knn(pts, queries, k, radius=None):
    """idx i32 (M,k) padded with -1, d2 f64 (M,k) padded with +inf, count i32 (M).  radius: hybrid (d2 < radius*radius, strict)."""
    D = d2_matrix(pts, queries)
    m, n = D.shape
    idx = np.full((m, k), -1, dtype=np.int32)
    d2 = np.full((m, k), np.inf)
    cnt = np.zeros(m, dtype=np.int32)
    r2 = None if radius is None else float(radius) * float(radius)
    for i in range(m):
        row = D[i]
        if not np.all(np.isfinite(row)):
            continue
        o = _order(row)
        if r2 is not None:
            o = o[row[o] < r2]
        o = o[:k]
        cnt[i] = len(o)
        idx[i, :len(o)] = o
        d2[i, :len(o)] = row[o]
    return idx, d2, cnt


def radius(pts, queries, radius):
    """CSR: offsets i64 (M+1), idx i32 (total), d2 f64 (total)"""
    D = d2_matrix(pts, queries)
    r2 = float(radius) * float(radius)
    offsets = [0]
    idx, d2 = [], []
    for row in D:
        if np.all(np.isfinite(row)):
            o = _order(row)
            o = o[row[o] < r2]
        else:
            o = np.zeros(0, dtype=np.int64)
        idx.append(o.astype(np.int32))
        d2.append(row[o])
        offsets.append(offsets[-1] + len(o))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.asarray(offsets, dtype=np.int64), cat(idx, np.int32), cat(d2, np.float64)


def quantised(rng, n, lo, hi):
    """n points with coordinates on the 1/16 grid inside [lo, hi] (per axis or scalar), float32"""
    lo, hi = np.broadcast_to(np.asarray(lo, float), 3), np.broadcast_to(np.asarray(hi, float), 3)
    p = np.stack([rng.integers(int(np.ceil(l * 16)), int(np.floor(h * 16)) + 1, n) for l, h in zip(lo, hi)], -1) / 16.0
    assert np.abs(p).max(initial=0.0) <= 4096
    return p.astype(np.float32)

"""NumPy restatements of Open3D's PointCloud::FarthestPointDownSample loop (the contract of kpx_farthest_point_sample).

    dist[j] = +inf; far = start_index
    for i < k: sel[i] = far; s = p[far]; max_dist = 0
               for j ascending: dist[j] = min(dist[j], |p[j] - s|^2)   (float64)
                                if dist[j] > max_dist: max_dist = dist[j]; far = j

`fps_loop` transcribes it literally (scalar Python, small clouds only); `fps` vectorises the inner loop per sample.  The next index
is the FIRST index of the largest dist (np.argmax) -- unless that largest dist is 0, where the loop keeps the previous index (np.argmax
would return 0).  Both sum the squares left to right, (dx^2 + dy^2) + dz^2, as Open3D does; the library's AC3 distance
fma(dz,dz, fma(dy,dy, dx*dx)) equals that whenever every square is exact, which `squares_exact` checks on an input."""
import numpy as np


def _f64(pts):
    return np.asarray(pts, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def fps_loop(pts, k, start_index=0):
    """literal transcription: sel int32 (k), cover float64 (k) = max_dist of each iteration"""
    p = _f64(pts).tolist()
    n = len(p)
    dist = [float("inf")] * n
    far = start_index
    sel, cover = [], []
    for _ in range(k):
        sel.append(far)
        sx, sy, sz = p[far]
        max_dist = 0.0
        for j in range(n):
            dx, dy, dz = p[j][0] - sx, p[j][1] - sy, p[j][2] - sz
            d = dx * dx + dy * dy + dz * dz
            dist[j] = min(dist[j], d)
            if dist[j] > max_dist:
                max_dist = dist[j]
                far = j
        cover.append(max_dist)
    return np.array(sel, dtype=np.int32), np.array(cover, dtype=np.float64)


def fps(pts, k, start_index=0):
    """the same loop, vectorised over j per sample"""
    p = _f64(pts)
    n = len(p)
    assert 0 <= k <= n and (k == 0 or 0 <= start_index < n)
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    dist = np.full(n, np.inf)
    d = np.empty(n)
    t = np.empty(n)
    far = int(start_index)
    sel = np.empty(k, dtype=np.int32)
    cover = np.empty(k, dtype=np.float64)
    for i in range(k):
        sel[i] = far
        np.subtract(x, x[far], out=d)
        np.multiply(d, d, out=d)
        np.subtract(y, y[far], out=t)
        np.multiply(t, t, out=t)
        np.add(d, t, out=d)
        np.subtract(z, z[far], out=t)
        np.multiply(t, t, out=t)
        np.add(d, t, out=d)
        np.minimum(dist, d, out=dist)
        j = int(np.argmax(dist))
        cover[i] = dist[j]
        if dist[j] > 0.0:           # strict '>' against max_dist = 0: all zero keeps the previous index
            far = j
    return sel, cover


def two_product_err(a, b):
    """Dekker's exact error of the float64 product a*b (0 iff the product is exact, barring overflow)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    split = 134217729.0                     # 2^27 + 1
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return ((ah * bh - p) + ah * bl + al * bh) + al * bl


def squares_exact(pts, max_unique=4096):
    """True if every coordinate difference of the cloud squares exactly in float64 (then the AC3 distance equals Open3D's sum).
    Integer coordinates with a span below 2^26 per axis pass at once (|dx| < 2^26: dx^2 < 2^52 is an exact integer); otherwise
    every difference of distinct values per axis is checked with two_product_err (up to `max_unique` values per axis; beyond,
    the answer is False)."""
    p = _f64(pts)
    if len(p) == 0:
        return True
    if np.all(p == np.round(p)) and np.all(p.max(0) - p.min(0) < 2.0 ** 26):
        return True
    for a in range(3):
        u = np.unique(p[:, a])
        if len(u) > max_unique:
            return False
        dx = (u[:, None] - u[None, :]).ravel()
        if np.any(two_product_err(dx, dx) != 0.0):
            return False
    return True


def assert_squares_exact(pts):
    assert squares_exact(pts), "a coordinate difference of this cloud does not square exactly: AC3 may differ from Open3D's sum"

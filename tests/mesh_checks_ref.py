"""Arithmetic contract AC15, restated: the mesh checks of [O3D] geometry.TriangleMesh -- non-manifold vertices,
orientation, volume, Euler-Poincare characteristic and intersecting triangle pairs -- in plain Python / NumPy, serial and brute
force.  The device matches every output of this file bit for bit.  Floating-point work is fp64 from the float32 vertices, every
multiply and add rounded separately (Python floats: IEEE doubles, no fused multiply-add); a dot product is (x x' + y y') + z z', a
cross-product component a b - c d.  tri_tri is Moeller's 1997 interval-overlap test in its division-free form with the coplanar
fallback, typed from memory; tests/test_mesh_checks_cpu.py judges it against exact integer predicates."""
import numpy as np

EPSILON = 1e-6          # [O3D] / Moeller: absolute, not normalised -- plane distances below it count as 0, whatever the mesh's scale


# ---- links: vertex manifoldness ------------------------------------------------------------------------------------------------
def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def _unite(parent, a, b):
    ra, rb = _find(parent, a), _find(parent, b)
    if ra != rb:
        parent[max(ra, rb)] = min(ra, rb)


def non_manifold_vertices(triangles, n_vertices):
    """-> int32 ascending: the vertices whose link has more than one connected component.  The link of v has one edge {u, w} per
    triangle in which v occurs exactly once (u, w the other two corners, u == w allowed); its nodes are the ends of those edges.  A
    vertex without a link edge is not reported."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    links = {}
    for a, b, c in t.tolist():
        for v, u, w in ((a, b, c), (b, c, a), (c, a, b)):
            if v != u and v != w:
                links.setdefault(v, []).append((u, w))
    out = []
    for v in sorted(links):
        parent = {}
        for u, w in links[v]:
            parent.setdefault(u, u)
            parent.setdefault(w, w)
            _unite(parent, u, w)
        if len({_find(parent, x) for x in parent}) > 1:
            out.append(v)
    assert all(0 <= v < n_vertices for v in out)
    return np.asarray(out, dtype=np.int32)


# ---- orientation -------------------------------------------------------------------------------------------------------------------
def orientation(triangles):
    """-> (orientable, flip bool (T,)).  A triangle with a repeated index takes no part.  Two others are neighbours when they share
    an edge key (min, max) -- ALL pairs of a run of equal keys; they agree on it when one runs it min -> max and the other max -> min.
    Orientable: some flip assignment makes all neighbours agree on all shared edges.  flip: in every connected component the smallest
    triangle keeps its winding (all False when not orientable)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    n = len(t)
    parent = list(range(2 * n))          # 2 i: triangle i as it is, 2 i + 1: flipped
    edges = {}
    for i, (a, b, c) in enumerate(t.tolist()):
        if a == b or b == c or a == c:
            continue
        for p, q in ((a, b), (b, c), (c, a)):
            edges.setdefault((min(p, q), max(p, q)), []).append((i, p < q))
    for run in edges.values():
        for x in range(len(run)):
            for y in range(x + 1, len(run)):
                (i, di), (j, dj) = run[x], run[y]
                if di != dj:
                    _unite(parent, 2 * i, 2 * j)
                    _unite(parent, 2 * i + 1, 2 * j + 1)
                else:
                    _unite(parent, 2 * i, 2 * j + 1)
                    _unite(parent, 2 * i + 1, 2 * j)
    roots = [_find(parent, x) for x in range(2 * n)]
    if any(roots[2 * i] == roots[2 * i + 1] for i in range(n)):
        return False, np.zeros(n, dtype=bool)
    return True, np.asarray([roots[2 * i] % 2 == 1 for i in range(n)], dtype=bool).reshape(n)


def orient_triangles(triangles, triangle_normals=None):
    """-> (orientable, triangles, triangle normals): a flip is (t0, t1, t2) -> (t0, t2, t1) and negates a stored triangle normal; a
    mesh that is not orientable comes back as it was"""
    t = np.array(triangles, dtype=np.int32).reshape(-1, 3)
    tn = None if triangle_normals is None else np.array(triangle_normals, dtype=np.float32).reshape(-1, 3)
    ok, flip = orientation(t)
    if ok:
        t[flip] = t[flip][:, [0, 2, 1]]
        if tn is not None:
            tn[flip] = -tn[flip]
    return ok, t, tn


# ---- volume, edges ---------------------------------------------------------------------------------------------------------------
def signed_volume_terms(vertices, triangles):
    """v0 . (v1 x v2) per triangle, float64 (T,): six times the signed volume of the tetrahedron it spans with the origin"""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    cx = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
    cy = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
    cz = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    return (a[:, 0] * cx + a[:, 1] * cy) + a[:, 2] * cz


def volume(vertices, triangles):
    """|the sum from 0, in ascending triangle index, of the signed terms| / 6.0 -- ONE division, after the sum: on integer corners the
    sum is exact, so the cube [0, 2]^3 is exactly 8.0 ([O3D] divides every term and gets 7.999999999999999)"""
    s = 0.0
    for x in signed_volume_terms(vertices, triangles).tolist():
        s = s + x
    return abs(s) / 6.0


def edge_count(triangles):
    """the number of distinct (min, max) corner pairs over the three edges of every triangle"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return len(np.unique(np.sort(e, 1), axis=0)) if len(e) else 0


def euler_poincare_characteristic(n_vertices, triangles):
    return int(n_vertices) - edge_count(triangles) + len(np.asarray(triangles).reshape(-1, 3))


# ---- triangle against triangle ---------------------------------------------------------------------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _intervals(vv0, vv1, vv2, d0, d1, d2, d0d1, d0d2):
    """-> (A, B, C, X0, X1), or None: the triangle lies in the other's plane"""
    if d0d1 > 0.0:
        return vv2, (vv0 - vv2) * d2, (vv1 - vv2) * d2, d2 - d0, d2 - d1
    if d0d2 > 0.0:
        return vv1, (vv0 - vv1) * d1, (vv2 - vv1) * d1, d1 - d0, d1 - d2
    if d1 * d2 > 0.0 or d0 != 0.0:
        return vv0, (vv1 - vv0) * d0, (vv2 - vv0) * d0, d0 - d1, d0 - d2
    if d1 != 0.0:
        return vv1, (vv0 - vv1) * d1, (vv2 - vv1) * d1, d1 - d0, d1 - d2
    if d2 != 0.0:
        return vv2, (vv0 - vv2) * d2, (vv1 - vv2) * d2, d2 - d0, d2 - d1
    return None


def _edge_edge(ax, ay, v0, u0, u1):
    """closed test of the edge from v0 along (ax, ay) against the edge u0 u1, all in 2D; parallel edges (f == 0) report nothing"""
    bx, by = u0[0] - u1[0], u0[1] - u1[1]
    cx, cy = v0[0] - u0[0], v0[1] - u0[1]
    f = ay * bx - ax * by
    d = by * cx - bx * cy
    if (f > 0.0 and d >= 0.0 and d <= f) or (f < 0.0 and d <= 0.0 and d >= f):
        e = ax * cy - ay * cx
        if f > 0.0:
            return e >= 0.0 and e <= f
        return e <= 0.0 and e >= f
    return False


def _point_in_tri(p, u0, u1, u2):
    """p strictly inside the 2D triangle"""
    a = u1[1] - u0[1]
    b = -(u1[0] - u0[0])
    c = -a * u0[0] - b * u0[1]
    d0 = (a * p[0] + b * p[1]) + c
    a = u2[1] - u1[1]
    b = -(u2[0] - u1[0])
    c = -a * u1[0] - b * u1[1]
    d1 = (a * p[0] + b * p[1]) + c
    a = u0[1] - u2[1]
    b = -(u0[0] - u2[0])
    c = -a * u2[0] - b * u2[1]
    d2 = (a * p[0] + b * p[1]) + c
    return d0 * d1 > 0.0 and d0 * d2 > 0.0


def _coplanar(n, v, u):
    a0, a1, a2 = abs(n[0]), abs(n[1]), abs(n[2])
    if a0 > a1:
        i0, i1 = (1, 2) if a0 > a2 else (0, 1)
    else:
        i0, i1 = (0, 1) if a2 > a1 else (0, 2)
    p = [(x[i0], x[i1]) for x in v]
    q = [(x[i0], x[i1]) for x in u]
    for k in range(3):
        s, e = p[k], p[(k + 1) % 3]
        ax, ay = e[0] - s[0], e[1] - s[1]
        if _edge_edge(ax, ay, s, q[0], q[1]) or _edge_edge(ax, ay, s, q[1], q[2]) or _edge_edge(ax, ay, s, q[2], q[0]):
            return True
    return _point_in_tri(p[0], q[0], q[1], q[2]) or _point_in_tri(q[0], p[0], p[1], p[2])


def tri_tri(v, u):
    """whether triangle v (three corners of three Python floats) meets triangle u; v is the pair's lower index / the query"""
    v0, v1, v2 = v
    u0, u1, u2 = u
    n1 = _cross(_sub(v1, v0), _sub(v2, v0))
    d1 = -_dot(n1, v0)
    du0, du1, du2 = _dot(n1, u0) + d1, _dot(n1, u1) + d1, _dot(n1, u2) + d1
    du0 = 0.0 if abs(du0) < EPSILON else du0
    du1 = 0.0 if abs(du1) < EPSILON else du1
    du2 = 0.0 if abs(du2) < EPSILON else du2
    du0du1, du0du2 = du0 * du1, du0 * du2
    if du0du1 > 0.0 and du0du2 > 0.0:
        return False
    n2 = _cross(_sub(u1, u0), _sub(u2, u0))
    d2 = -_dot(n2, u0)
    dv0, dv1, dv2 = _dot(n2, v0) + d2, _dot(n2, v1) + d2, _dot(n2, v2) + d2
    dv0 = 0.0 if abs(dv0) < EPSILON else dv0
    dv1 = 0.0 if abs(dv1) < EPSILON else dv1
    dv2 = 0.0 if abs(dv2) < EPSILON else dv2
    dv0dv1, dv0dv2 = dv0 * dv1, dv0 * dv2
    if dv0dv1 > 0.0 and dv0dv2 > 0.0:
        return False
    dd = _cross(n1, n2)
    index, big = 0, abs(dd[0])
    if abs(dd[1]) > big:
        index, big = 1, abs(dd[1])
    if abs(dd[2]) > big:
        index = 2
    iv = _intervals(v0[index], v1[index], v2[index], dv0, dv1, dv2, dv0dv1, dv0dv2)
    if iv is None:
        return _coplanar(n1, v, u)
    a, b, c, x0, x1 = iv
    iu = _intervals(u0[index], u1[index], u2[index], du0, du1, du2, du0du1, du0du2)
    if iu is None:
        return _coplanar(n1, v, u)
    d, e, f, y0, y1 = iu
    xx, yy = x0 * x1, y0 * y1
    xxyy = xx * yy
    tmp = a * xxyy
    i1 = (tmp + (b * x1) * yy, tmp + (c * x0) * yy)
    tmp = d * xxyy
    i2 = (tmp + (e * xx) * y1, tmp + (f * xx) * y0)
    lo1, hi1 = (i1[1], i1[0]) if i1[0] > i1[1] else i1
    lo2, hi2 = (i2[1], i2[0]) if i2[0] > i2[1] else i2
    return not (hi1 < lo2 or hi2 < lo1)


def _corners(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return v[t] if len(t) else np.zeros((0, 3, 3))


def _meets(p, q):
    return tri_tri(tuple(map(tuple, p.tolist())), tuple(map(tuple, q.tolist())))


def triangle_pairs(vertices, triangles, other=None):
    """-> int32 (P, 2) ascending in (t0, t1).  Two triangles intersect when their exact boxes (componentwise min / max of the corners
    as doubles, closed comparison) overlap AND tri_tri(lower, higher) says so.  other None: the pairs t0 < t1 of one mesh, a pair that
    shares a vertex INDEX skipped; other = (vertices, triangles): every (t0 of this mesh, t1 of the other), nothing skipped, tri_tri(
    this, other)."""
    c = _corners(vertices, triangles)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    oc = c if other is None else _corners(*other)
    lo, hi, olo, ohi = c.min(1), c.max(1), oc.min(1), oc.max(1)
    out = []
    for i in range(len(c)):
        near = ((lo[i] <= ohi) & (olo <= hi[i])).all(1) if len(oc) else np.zeros(0, dtype=bool)
        if other is None:
            near[:i + 1] = False
            near &= ~(t[:, :, None] == t[i][None, None, :]).any((1, 2))
        out.extend((i, int(j)) for j in np.flatnonzero(near) if _meets(c[i], oc[j]))
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def is_intersecting(vertices, triangles, other):
    return len(triangle_pairs(vertices, triangles, other)) > 0


# ---- the composed answers ----------------------------------------------------------------------------------------------------------
def boundary_or_shared_edges(triangles):
    """whether some edge key is not met by exactly two triangle edges (is_edge_manifold(False) is its negation; AC13)"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if not len(t):
        return False
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    return bool((np.unique(e, axis=0, return_counts=True)[1] != 2).any())


def is_watertight(vertices, triangles):
    return (not boundary_or_shared_edges(triangles) and len(non_manifold_vertices(triangles, len(np.asarray(vertices).reshape(-1, 3)))) == 0
            and len(triangle_pairs(vertices, triangles)) == 0)

"""The restatement of AC15 (tests/mesh_checks_ref.py) judged by properties, without a device: its triangle-triangle test against
exact integer / rational predicates written independently of it, its links, orientation and volume on meshes whose answers are known
by construction."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import mesh_checks_ref as R
import tsdf_mesh_ref as M
from mesh_checks_cases import CUBE, CUBE_V, TET, TET_V, bowtie, fan, moebius, sphere


# ---- exact predicates on integer triangles -------------------------------------------------------------------------------------------
def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _normal(t):
    return _cross(_sub(t[1], t[0]), _sub(t[2], t[0]))


def _flat(t, n):
    """the triangle's plane as 2D: the axis of the largest |n| dropped (a bijection of the plane, since that component is not 0)"""
    k = max(range(3), key=lambda i: abs(n[i]))
    return lambda p: tuple(p[i] for i in range(3) if i != k)


def _orient2(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _in_tri2(p, t, strict):
    s = [_orient2(t[k], t[(k + 1) % 3], p) for k in range(3)]
    if strict:
        return all(x > 0 for x in s) or all(x < 0 for x in s)
    return all(x >= 0 for x in s) or all(x <= 0 for x in s)


def _on_seg2(a, b, p):
    return _orient2(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def _seg_seg2(a, b, c, d):
    """closed 2D segments meet"""
    o1, o2, o3, o4 = _orient2(a, b, c), _orient2(a, b, d), _orient2(c, d, a), _orient2(c, d, b)
    if ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0)):
        return True
    return _on_seg2(a, b, c) or _on_seg2(a, b, d) or _on_seg2(c, d, a) or _on_seg2(c, d, b)


def _edge_meets(p, q, t, strict):
    """closed: the segment p q meets the closed triangle t.  strict: it crosses t's relative interior, one end strictly on each side."""
    n = _normal(t)
    sp, sq = _dot(n, _sub(p, t[0])), _dot(n, _sub(q, t[0]))
    flat = _flat(t, n)
    t2 = [flat(x) for x in t]
    if sp == 0 and sq == 0:
        if strict:
            return False
        p2, q2 = flat(p), flat(q)
        return (_in_tri2(p2, t2, False) or _in_tri2(q2, t2, False) or any(_seg_seg2(p2, q2, t2[k], t2[(k + 1) % 3]) for k in range(3)))
    if (sp > 0 and sq > 0) or (sp < 0 and sq < 0) or (strict and (sp == 0 or sq == 0)):
        return False
    w = Fraction(sp, sp - sq)
    x = tuple(Fraction(a) + w * (b - a) for a, b in zip(p, q))
    return _in_tri2(flat(x), t2, strict)


def _clip_area(p, q):
    """area of the intersection of two 2D triangles (Sutherland-Hodgman with rationals), doubled"""
    if _orient2(*q) < 0:
        q = [q[0], q[2], q[1]]
    poly = [tuple(Fraction(c) for c in x) for x in p]
    for k in range(3):
        a, b = q[k], q[(k + 1) % 3]
        out = []
        for i in range(len(poly)):
            s, e = poly[i - 1], poly[i]
            ss, se = _orient2(a, b, s), _orient2(a, b, e)
            if (ss >= 0) != (se >= 0):
                w = ss / (ss - se)
                out.append((s[0] + w * (e[0] - s[0]), s[1] + w * (e[1] - s[1])))
            if se >= 0:
                out.append(e)
        poly = out
        if not poly:
            return 0
    return abs(sum(poly[i - 1][0] * poly[i][1] - poly[i][0] * poly[i - 1][1] for i in range(len(poly))))


def exact(v, u):
    """-> (closed, proper) for two non-degenerate integer triangles"""
    edges = lambda t: [(t[k], t[(k + 1) % 3]) for k in range(3)]
    closed = any(_edge_meets(p, q, u, False) for p, q in edges(v)) or any(_edge_meets(p, q, v, False) for p, q in edges(u))
    proper = any(_edge_meets(p, q, u, True) for p, q in edges(v)) or any(_edge_meets(p, q, v, True) for p, q in edges(u))
    n = _normal(v)
    if not proper and all(_dot(n, _sub(x, v[0])) == 0 for x in u):
        flat = _flat(v, n)
        proper = _clip_area([flat(x) for x in v], [flat(x) for x in u]) > 0
    return closed, proper


def reported(v, u):
    f = lambda t: tuple(tuple(float(c) for c in x) for x in t)
    return R.tri_tri(f(v), f(u))


def check_bracket(v, u):
    closed, proper = exact(v, u)
    assert not proper or closed
    for a, b in ((v, u), (u, v)):
        got = reported(a, b)
        assert not proper or got, ("a proper intersection was missed", a, b)
        assert not got or closed, ("disjoint triangles were reported", a, b)
    return closed, proper


def _random_triangles(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        t = tuple(tuple(int(c) for c in x) for x in rng.integers(-3, 4, (3, 3)))
        if any(_normal(t)):
            out.append(t)
    return out


def test_tri_tri_random_integer_pairs_lie_in_the_exact_bracket():
    ts = _random_triangles(1, 6000)
    n_closed = n_proper = 0
    for v, u in zip(ts[0::2], ts[1::2]):
        closed, proper = check_bracket(v, u)
        n_closed += closed
        n_proper += proper
    assert n_proper > 300 and n_closed - n_proper > 30 and n_closed < 2900          # the sample has all three kinds


def test_tri_tri_random_coplanar_pairs_lie_in_the_exact_bracket():
    rng = np.random.default_rng(2)
    done = 0
    while done < 1500:
        k, h = int(rng.integers(0, 3)), int(rng.integers(-3, 4))
        pts = rng.integers(-3, 4, (6, 2))
        tri = [tuple(tuple(int(c) for c in np.insert(p, k, h)) for p in pts[s:s + 3]) for s in (0, 3)]
        if any(_normal(tri[0])) and any(_normal(tri[1])):
            check_bracket(*tri)
            done += 1


ENUMERATED = {
    "piercing": (((0, 0, 0), (3, 0, 0), (0, 3, 0)), ((1, 1, -1), (1, 1, 2), (2, 2, 2)), True, True),
    "edge through the interior": (((-3, -3, 0), (3, -3, 0), (0, 3, 0)), ((0, 0, -2), (0, 0, 2), (3, 3, 3)), True, True),
    "touching at a vertex": (((0, 0, 0), (2, 0, 0), (0, 2, 0)), ((0, 0, 0), (-1, -1, 1), (-1, -2, 2)), True, False),
    "vertex on the interior": (((0, 0, 0), (3, 0, 0), (0, 3, 0)), ((1, 1, 0), (1, 1, 2), (2, 1, 2)), True, False),
    "shared edge position": (((0, 0, 0), (2, 0, 0), (0, 2, 0)), ((0, 0, 0), (2, 0, 0), (0, 0, 2)), True, False),
    "coplanar shared edge": (((0, 0, 0), (2, 0, 0), (0, 2, 0)), ((0, 0, 0), (2, 0, 0), (0, -2, 0)), True, False),
    "coplanar identical": (((0, 0, 1), (2, 0, 1), (0, 2, 1)), ((0, 0, 1), (2, 0, 1), (0, 2, 1)), True, True),
    "coplanar overlapping": (((0, 0, 0), (3, 0, 0), (0, 3, 0)), ((1, 1, 0), (3, 1, 0), (1, 3, 0)), True, True),
    "coplanar contained": (((-3, -3, 2), (3, -3, 2), (0, 3, 2)), ((-1, -1, 2), (1, -1, 2), (0, 1, 2)), True, True),
    "coplanar touching at a vertex": (((0, 0, 0), (2, 0, 0), (0, 2, 0)), ((2, 0, 0), (3, 0, 0), (3, 1, 0)), True, False),
    "coplanar disjoint": (((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((2, 2, 0), (3, 2, 0), (2, 3, 0)), False, False),
    "coplanar in a tilted plane": (((0, 0, 0), (2, 0, 2), (0, 2, 0)), ((1, 0, 1), (3, 0, 3), (1, 2, 1)), True, True),
    "parallel planes": (((0, 0, 0), (2, 0, 0), (0, 2, 0)), ((0, 0, 1), (2, 0, 1), (0, 2, 1)), False, False),
    "crossing planes, apart": (((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((3, 3, -1), (3, 3, 1), (3, 2, 1)), False, False),
    "crossing lines, intervals apart": (((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((2, 0, -1), (3, 0, 1), (2, 1, 1)), False, False),
}


@pytest.mark.parametrize("name", sorted(ENUMERATED))
def test_tri_tri_enumerated_configurations(name):
    v, u, want_closed, want_proper = ENUMERATED[name]
    for perm in itertools.permutations(range(3)):
        closed, proper = check_bracket(tuple(v[i] for i in perm), u)
        assert (closed, proper) == (want_closed, want_proper)          # the exact predicates themselves, judged by hand
    if want_closed == want_proper:
        assert reported(v, u) == want_closed and reported(u, v) == want_closed


def test_epsilon_is_absolute_and_decides_nothing_on_integers():
    assert R.EPSILON == 1e-6
    v, u = ((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((0, 0, 1), (1, 0, 1), (0, 1, 1))
    assert not reported(v, u)
    tiny = lambda t: tuple(tuple(c * 1e-4 for c in x) for x in t)          # the same pair, ten thousand times smaller: now "coplanar"
    assert R.tri_tri(tiny(v), tiny(u))


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def shared_edges_run_both_ways(t):
    seen = {}
    for a, b, c in np.asarray(t).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            seen.setdefault((min(p, q), max(p, q)), []).append(p < q)
    return all(len(d) == 1 or sorted(d) == [False, True] for d in seen.values())


def test_links():
    v, t = bowtie()
    assert R.non_manifold_vertices(t, len(v)).tolist() == [0]
    v, t = fan(12)
    pinched = np.concatenate([t[:5], t[6:11]])               # two separate wedges about the apex
    assert R.non_manifold_vertices(pinched, len(v)).tolist() == [0]
    v, t = fan(5000)
    assert len(R.non_manifold_vertices(t, len(v))) == 0
    v, t = fan(40, closed=False)
    assert len(R.non_manifold_vertices(t, len(v))) == 0      # an open fan: the link is a path
    assert len(R.non_manifold_vertices([[0, 0, 1]], 2)) == 0 and len(R.non_manifold_vertices([[2, 2, 2]], 3)) == 0
    assert R.non_manifold_vertices([[0, 0, 1], [0, 2, 3], [0, 4, 5]], 6).tolist() == [0]         # (a, a, b) adds no link edge to a
    assert len(R.non_manifold_vertices([[0, 1, 1]], 2)) == 0                                      # u == w: one node, one component
    assert R.non_manifold_vertices(np.zeros((0, 3)), 4).dtype == np.int32


def test_orientation_repairs_a_randomly_flipped_closed_surface():
    v, t = sphere()
    assert shared_edges_run_both_ways(t)
    rng = np.random.default_rng(5)
    flip = rng.random(len(t)) < 0.5
    flip[0] = False
    mixed = t.copy()
    mixed[flip] = mixed[flip][:, [0, 2, 1]]
    assert not shared_edges_run_both_ways(mixed)
    tn = M.triangle_normals(v, mixed)
    ok, fixed, ftn = R.orient_triangles(mixed, tn)
    assert ok and shared_edges_run_both_ways(fixed) and np.array_equal(fixed[0], mixed[0]) and np.array_equal(fixed, t)
    assert np.array_equal(ftn[flip], -tn[flip]) and np.array_equal(ftn[~flip], tn[~flip])
    flip[0] = True                                            # triangle 0 keeps its winding: the whole surface comes back inside out
    mixed = t.copy()
    mixed[flip] = mixed[flip][:, [0, 2, 1]]
    ok, fixed, _ = R.orient_triangles(mixed)
    assert ok and np.array_equal(fixed, t[:, [0, 2, 1]])


def test_orientation_of_one_sided_and_branching_meshes():
    v, t = moebius(11)
    assert len(t) == 11 and R.edge_count(t) == 22
    ok, same, _ = R.orient_triangles(t)
    assert not ok and np.array_equal(same, t)
    ok, _ = R.orientation(moebius(12)[1])                     # an even band closes with two sides
    assert ok
    book = [[0, 1, 2 + k] for k in range(5)]
    assert not R.orientation(book)[0]
    assert not R.orientation([[0, 1, 2], [0, 1, 3], [1, 0, 4]])[0]          # three on an edge, whatever their directions
    assert R.orientation(book[:2])[0] and R.orientation(book[:2])[1].tolist() == [False, True]
    ok, flip = R.orientation([[0, 1, 2], [1, 1, 3], [0, 1, 3], [3, 3, 3]])          # repeated indices take no part
    assert ok and flip.tolist() == [False, False, True, False]


def test_orientation_seeds_every_component_by_its_smallest_triangle():
    a = np.asarray(TET, dtype=np.int32)
    b = a[:, [0, 2, 1]] + 4                                   # the second tetrahedron inward
    t = np.concatenate([a[:1], b[:1], a[1:], b[1:]])
    t[2] = t[2][[0, 2, 1]]
    t[5] = t[5][[0, 2, 1]]
    ok, flip = R.orientation(t)
    assert ok and np.flatnonzero(flip).tolist() == [2, 5]
    _, fixed, _ = R.orient_triangles(t)
    assert np.array_equal(fixed[0], a[0]) and np.array_equal(fixed[1], b[0]) and shared_edges_run_both_ways(fixed)


def test_volume():
    assert R.volume(CUBE_V, CUBE) == 8.0 and R.is_watertight(CUBE_V, CUBE) and R.orientation(CUBE)[0] and not R.orientation(CUBE)[1].any()
    assert R.euler_poincare_characteristic(8, CUBE) == 2
    assert R.volume(TET_V, TET) == 4.5
    moved = TET_V + np.array([5, -7, 2], dtype=np.float32)
    assert R.volume(moved, TET) == 4.5
    assert R.volume(moved, np.asarray(TET)[:, [0, 2, 1]]) == 4.5          # inside out: the absolute value
    assert R.volume(moved, np.zeros((0, 3), dtype=np.int32)) == 0.0


def test_sphere_is_sound_and_its_volume_lies_between_its_own_two_balls():
    v, t = sphere()
    assert R.is_watertight(v, t) and R.orientation(t)[0] and R.euler_poincare_characteristic(len(v), t) == 2
    x = v.astype(np.float64)
    centre = x.mean(0)
    reach = np.sqrt(((x - centre) ** 2).sum(1)).max()
    a, b, c = (x[t[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    plane = np.abs(((a - centre) * n).sum(1)) / np.sqrt((n * n).sum(1))
    assert 0.0 < plane.min() < reach
    ball = lambda r: 4.0 / 3.0 * math.pi * r ** 3
    assert ball(plane.min()) < R.volume(v, t) < ball(reach)


def test_watertight():
    v, t = sphere()
    assert not R.is_watertight(v, t[1:]) and R.boundary_or_shared_edges(t[1:])                    # a boundary edge
    bv, bt = bowtie()
    assert not R.boundary_or_shared_edges(bt) and len(R.triangle_pairs(bv, bt)) == 0 and not R.is_watertight(bv, bt)      # the vertex alone
    # two closed tetrahedra, the second pushed into the first along the diagonal
    v2 = np.concatenate([TET_V, TET_V + np.float32(0.5)])
    t2 = np.concatenate([np.asarray(TET), np.asarray(TET) + 4]).astype(np.int32)
    assert not R.boundary_or_shared_edges(t2) and len(R.non_manifold_vertices(t2, 8)) == 0
    pairs = R.triangle_pairs(v2, t2)
    # by hand: the second tetrahedron's corner 4 = (0.5, 0.5, 0.5) lies inside the first, its corners 5, 6, 7 = (3.5, 0.5, 0.5), ...
    # outside beyond the slanted face 2 (x + y + z = 3).  So the slanted face is crossed by the three edges out of corner 4 -- each
    # belongs to two of the faces 4, 5, 7 that meet at corner 4 -- and no other face of the first is reached (x, y, z >= 0.5 > 0);
    # the far face 6 (x + y + z = 4.5) is beyond the first tetrahedron.
    assert pairs.tolist() == [[2, 4], [2, 5], [2, 7]] and pairs.dtype == np.int32
    assert not R.is_watertight(v2, t2)
    assert R.is_intersecting(TET_V, TET, (TET_V + np.float32(0.5), TET)) and not R.is_intersecting(TET_V, TET, (TET_V + np.float32(9), TET))
    assert not R.is_intersecting(TET_V, TET, (np.zeros((0, 3)), np.zeros((0, 3))))
    # coincident positions under different indices are not skipped, a shared index is
    twice = np.concatenate([TET_V[:3], TET_V[:3]])
    assert R.triangle_pairs(twice, [[0, 1, 2], [3, 4, 5]]).tolist() == [[0, 1]]
    assert len(R.triangle_pairs(twice, [[0, 1, 2], [0, 4, 5]])) == 0

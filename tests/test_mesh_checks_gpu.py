"""GPU suite of the mesh checks (kpx_mesh.hip, kpx_raycast.hip; AC15): every output of every method == the restatement
tests/mesh_checks_ref.py, bit for bit, and the pair search three ways -- box hierarchy == the device's brute form == the restatement --
on marching-cubes meshes, triangle counts on the tree's leaf / fan-out and the compaction's tile boundaries (read from
include/kinectpx.h), hand-built degenerate, coplanar, one-sided and pinched meshes, dense and empty pair lists."""
import functools
import os
import re

import numpy as np
import pytest

import mesh_checks_ref as R
import tsdf_mesh_ref as M
from mesh_checks_cases import TET, TET_V, bowtie, fan, moebius, sphere

pytestmark = pytest.mark.gpu

_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kinectpx.h")).read()
_define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, _HEADER).group(1))
LEAF, FAN = _define("KPX_RAYSCENE_LEAF"), _define("KPX_RAYSCENE_FANOUT")
SIZES = [0, 1, LEAF - 1, LEAF, LEAF + 1, LEAF * FAN, LEAF * FAN + 1, LEAF * FAN * FAN + 1]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(None)
def random_mesh(res):
    """test_raycast_gpu.random_mesh restated: res 8: 458 triangles, 13: 2408, 24: 16 548"""
    rng = np.random.default_rng(1000 + res)
    n = res ** 3
    f = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    where = rng.random(n) < 0.08
    f[where] = special[rng.integers(0, 4, int(where.sum()))]
    w = np.where(rng.random(n) < 0.1, 0.0, rng.integers(1, 9, n)).astype(np.float32)
    c = rng.uniform(0.0, 255.0, (n, 3)).astype(np.float32)
    v, _, t, _ = M.extract_triangle_mesh(f, w, c, res, (res * 0.013) / res, np.array((-0.37, 1.91, 12.3)))
    return v, t


@functools.lru_cache(None)
def mesh(name):
    """-> vertices float32 (V, 3), triangles int32 (T, 3); read-only"""
    kind, _, arg = name.partition("-")
    rng = np.random.default_rng(77)
    if kind == "res":
        v, t = random_mesh(int(arg))
    elif kind == "cut":                                      # the first n triangles of the resolution-13 mesh
        v, t = random_mesh(13)
        t = t[:int(arg)]
    elif name == "sphere":
        v, t = sphere()
    elif name == "flipped":                                  # the sphere, a seeded random half of it inside out
        v, t = sphere()
        t = t.copy()
        k = np.random.default_rng(5).random(len(t)) < 0.5
        t[k] = t[k][:, [0, 2, 1]]
    elif name == "open":                                     # the sphere without its first triangle
        v, t = sphere()
        t = t[1:]
    elif name == "book":                                     # five triangles on one edge
        v, t = rng.random((7, 3)), [[0, 1, 2 + k] for k in range(5)]
    elif name == "duplicate":                                # every triangle of the book twice
        v, t = rng.random((7, 3)), [[0, 1, 2 + k] for k in range(5)] * 2
    elif name == "degenerate":                               # repeated indices, collinear corners, a repeated triangle, an unused vertex
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [1, 1, 0.5], [3, 3, 3], [0.5, 0.5, 2]])
        t = [[0, 1, 3], [0, 1, 2], [1, 1, 4], [1, 4, 2], [4, 4, 4], [0, 1, 2], [2, 6, 2], [1, 2, 4]]
    elif name == "grid":                                     # flat, axis-aligned, integer corners: every neighbour is coplanar
        x, y = np.meshgrid(np.arange(7.0), np.arange(7.0), indexing="ij")
        v = np.stack([x, y, np.ones_like(x)], -1).reshape(-1, 3)
        i = (np.arange(6)[:, None] * 7 + np.arange(6)[None, :]).reshape(-1)
        t = np.concatenate([np.stack([i, i + 7, i + 8], 1), np.stack([i, i + 8, i + 1], 1)])
    elif name == "millimetres":                              # the resolution-8 mesh in millimetres, thousands from the origin
        v, t = random_mesh(8)
        v = (v.astype(np.float64) - v.astype(np.float64).mean(0)) * 1000.0 + np.array((5000.0, -3000.0, 2500.0))
    elif name == "disjoint":                                 # 70 000 triangles that share nothing, one inside each cell of a lattice
        k = np.arange(70000)
        cell = np.stack([k % 50, (k // 50) % 50, k // 2500], 1).astype(np.float64)
        v = (cell[:, None, :] + 0.1 + 0.7 * rng.random((70000, 3, 3))).reshape(-1, 3)
        t = np.arange(210000).reshape(-1, 3)
    elif name == "soup":                                     # 300 random triangles in a unit cube: many crossing pairs
        v, t = rng.random((900, 3)), np.arange(900).reshape(-1, 3)
    elif name == "coincident":                               # 200 copies of one triangle under distinct indices: 19 900 pairs
        v, t = np.tile(rng.random((3, 3)), (200, 1)), np.arange(600).reshape(-1, 3)
    elif name == "moebius":
        v, t = moebius(11)
    elif name == "bowtie":
        v, t = bowtie()
    elif name == "fan":                                      # a closed fan of 5000 triangles about one apex
        v, t = fan(5000)
    elif name == "tetrahedra":                               # two closed tetrahedra, one pushed into the other
        v, t = np.concatenate([TET_V, TET_V + np.float32(0.5)]), np.concatenate([np.asarray(TET), np.asarray(TET) + 4])
    else:
        raise KeyError(name)
    return np.asarray(v, dtype=np.float32).reshape(-1, 3), np.asarray(t, dtype=np.int32).reshape(-1, 3)


@functools.lru_cache(None)
def ref_pairs(name):
    return R.triangle_pairs(*mesh(name))


@functools.lru_cache(None)
def ref_orientation(name):
    return R.orientation(mesh(name)[1])


def build(v, t, tn=None, vn=None):
    from kinectpy_amd import o3d
    m = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(v), o3d.utility.Vector3iVector(t))
    if tn is not None:
        m.triangle_normals = o3d.utility.Vector3dVector(tn)
    if vn is not None:
        m.vertex_normals = o3d.utility.Vector3dVector(vn)
    return m


def host(t):
    return None if t is None else t.cpu().numpy()


def watertight(name):
    from kinectpy_amd import ops
    return ops.mesh_is_watertight(*mesh(name))


def check_topology(name):
    """links, orientation, Euler characteristic, volume: device == restatement"""
    from kinectpy_amd import ops
    v, t = mesh(name)
    m = build(v, t)
    want = R.non_manifold_vertices(t, len(v))
    got = m.get_non_manifold_vertices()
    assert same(got, want), (got, want)
    assert m.is_vertex_manifold() == (len(want) == 0)
    ok, flip = ref_orientation(name)
    dok, dflip, _, _ = ops.mesh_orientation(v, t)
    assert dok == ok and m.is_orientable() == ok and np.array_equal(host(dflip).astype(bool), flip)
    tn = np.random.default_rng(len(t)).normal(size=(len(t), 3)).astype(np.float32)
    vn = np.random.default_rng(len(v)).normal(size=(len(v), 3)).astype(np.float32)
    m2 = build(v, t, tn if len(t) else None, vn if len(v) else None)
    rok, rt, rtn = R.orient_triangles(t, tn)
    assert m2.orient_triangles() == rok
    assert same(host(m2._tri), rt) and same(host(m2._vert), v)
    if len(t):
        assert same(host(m2._tnrm), rtn)
    if len(v):
        assert same(host(m2._vnrm), vn)
    assert m.euler_poincare_characteristic() == R.euler_poincare_characteristic(len(v), t)
    vol = ops.mesh_volume(v, t)
    assert same(np.float64(vol), np.float64(R.volume(v, t))), (vol, R.volume(v, t))
    assert same(host(m._tri), t)                             # the queries left the mesh alone
    return m


def check_pairs(name, brute=True):
    """pair search: hierarchy == device brute == restatement, list and any forms; is_watertight from its three parts"""
    from kinectpy_amd import ops
    v, t = mesh(name)
    want = ref_pairs(name)
    m = build(v, t)
    got = np.asarray(m.get_self_intersecting_triangles())
    assert same(got.reshape(-1, 2), want), (got.shape, want.shape)
    assert m.is_self_intersecting() == (len(want) > 0)
    if brute:
        assert same(host(ops.mesh_self_intersections(v, t, brute=True)), want)
        assert ops.mesh_is_self_intersecting(v, t, brute=True) == (len(want) > 0)
    sound = not R.boundary_or_shared_edges(t) and len(R.non_manifold_vertices(t, len(v))) == 0 and len(want) == 0
    assert ops.mesh_is_watertight(v, t) == sound
    if sound and ref_orientation(name)[0]:
        assert same(np.float64(m.get_volume()), np.float64(R.volume(v, t)))
    else:
        with pytest.raises(RuntimeError):
            m.get_volume()
    return want


@pytest.mark.parametrize("name", ["res-8", "res-13", "res-24", "sphere", "flipped", "open", "book", "duplicate", "degenerate", "grid", "millimetres",
                                  "disjoint", "soup", "coincident", "moebius", "bowtie", "fan", "tetrahedra", "cut-2047", "cut-2048", "cut-2049"]
                         + ["cut-%d" % n for n in SIZES])
def test_topology_matches_the_restatement(name):
    check_topology(name)


@pytest.mark.parametrize("name", ["res-8", "res-13", "sphere", "flipped", "open", "book", "duplicate", "degenerate", "grid", "millimetres", "soup",
                                  "coincident", "moebius", "bowtie", "fan", "tetrahedra", "cut-2047", "cut-2048", "cut-2049"]
                         + ["cut-%d" % n for n in SIZES])
def test_pairs_three_ways(name):
    check_pairs(name)


def test_known_answers():
    assert len(ref_pairs("soup")) > 500 and len(ref_pairs("coincident")) == 19900 and len(ref_pairs("grid")) == 0
    assert ref_pairs("tetrahedra").tolist() == [[2, 4], [2, 5], [2, 7]]
    assert not ref_orientation("moebius")[0] and not ref_orientation("book")[0] and ref_orientation("flipped")[0]
    m = build(*mesh("sphere"))
    assert watertight("sphere") and m.is_orientable() and m.euler_poincare_characteristic() == 2 and m.get_volume() > 0.0
    assert not watertight("open") and not watertight("bowtie") and not watertight("tetrahedra")
    assert build(*mesh("bowtie")).get_non_manifold_vertices().tolist() == [0] and build(*mesh("fan")).is_vertex_manifold()
    fixed = build(*mesh("flipped"))
    assert fixed.orient_triangles() and same(host(fixed._tri)[0], mesh("flipped")[1][0])
    back = host(fixed._tri)
    assert same(back, mesh("sphere")[1]) or same(back, mesh("sphere")[1][:, [0, 2, 1]])


def test_disjoint_triangles_have_no_partner():
    """70 000 triangles in cells of their own: no two exact boxes overlap, so the restated list is empty by construction"""
    v, t = mesh("disjoint")
    c = v[t]
    assert (np.floor(c.min(1)) == np.floor(c.max(1))).all() and len(np.unique(np.floor(c.min(1)), axis=0)) == len(t)
    m = build(v, t)
    assert len(m.get_self_intersecting_triangles()) == 0 and not m.is_self_intersecting()
    assert not watertight("disjoint")                         # every edge is a boundary


def test_large_mesh_pairs_against_the_restatement_on_a_slice():
    """resolution 24 (16 548 triangles, a tree of seven levels): the hierarchy's pairs of the first 512 query triangles"""
    from kinectpy_amd import ops
    v, t = mesh("res-24")
    got = host(ops.mesh_self_intersections(v, t))
    c = v[t].astype(np.float64)
    lo, hi = c.min(1), c.max(1)
    want = []
    for i in range(512):
        near = ((lo[i] <= hi) & (lo <= hi[i])).all(1)
        near[:i + 1] = False
        near &= ~(t[:, :, None] == t[i][None, None, :]).any((1, 2))
        want.extend((i, int(j)) for j in np.flatnonzero(near) if R._meets(c[i], c[j]))
    assert same(got[got[:, 0] < 512], np.asarray(want, dtype=np.int32).reshape(-1, 2))
    assert (got[:, 0] < got[:, 1]).all() and (np.diff(got[:, 0].astype(np.int64) << 32 | got[:, 1]) > 0).all()


def test_is_intersecting():
    from kinectpy_amd import ops
    v, t = mesh("sphere")
    a = build(v, t)
    shifted, far = v + np.float32(0.75), v + np.float32(40.0)
    assert R.is_intersecting(v, t, (shifted, t)) and not R.is_intersecting(v, t, (far, t))
    assert a.is_intersecting(build(shifted, t)) and not a.is_intersecting(build(far, t))
    assert not a.is_intersecting(build(np.zeros((0, 3)), np.zeros((0, 3)))) and not build(np.zeros((0, 3)), np.zeros((0, 3))).is_intersecting(a)
    assert a.is_intersecting(a)                               # no shared-vertex exemption between two meshes
    scene = ops.rayscene_build(shifted, t)
    want = R.triangle_pairs(v, t, (shifted, t))
    assert same(host(ops.rayscene_triangle_pairs(scene, v, t)), want) and same(host(ops.rayscene_triangle_pairs(scene, v, t, brute=True)), want)
    assert ops.rayscene_triangles_meet(scene, v, t, brute=True)
    with pytest.raises(RuntimeError):
        a.is_intersecting((v, t))


def test_a_mesh_that_is_not_orientable_is_left_alone():
    for name in ("moebius", "book", "duplicate"):
        v, t = mesh(name)
        tn, vn = M.triangle_normals(v, t), M.vertex_normals(v, t)
        m = build(v, t, tn, vn)
        assert m.orient_triangles() is False
        assert same(host(m._vert), v) and same(host(m._tri), t) and same(host(m._tnrm), tn) and same(host(m._vnrm), vn)


def test_get_volume_raises_on_the_open_sphere():
    with pytest.raises(RuntimeError, match="watertight"):
        build(*mesh("open")).get_volume()
    with pytest.raises(RuntimeError):
        build(*mesh("moebius")).get_volume()


def test_repetition_repeats_its_bits():
    from kinectpy_amd import ops
    v, t = mesh("soup")
    first = host(ops.mesh_self_intersections(v, t))
    for _ in range(3):
        assert same(host(ops.mesh_self_intersections(v, t)), first)
    v, t = mesh("res-24")
    runs = [(host(ops.mesh_non_manifold_vertices(v, t)), host(ops.mesh_orientation(v, t)[1]), ops.mesh_volume(v, t)) for _ in range(3)]
    for r in runs[1:]:
        assert same(r[0], runs[0][0]) and same(r[1], runs[0][1]) and same(np.float64(r[2]), np.float64(runs[0][2]))


def test_arguments_are_checked_before_the_device_is_touched():
    import torch
    from kinectpy_amd import _lib as L, ops
    v, t = mesh("res-8")
    with pytest.raises(RuntimeError, match="no scene"):
        ops.rayscene_triangle_pairs(ops.RayScene(torch.zeros(1 << 16, dtype=torch.uint8, device=L.device()), len(t)), v, t, True)
    with pytest.raises(RuntimeError, match="RayScene"):
        ops.rayscene_triangle_pairs(None, v, t)
    scene = ops.rayscene_build(v, t)
    with pytest.raises(RuntimeError, match="built from"):
        ops.rayscene_triangle_pairs(scene, v, t[:-1], True)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_non_manifold_vertices(v, t + 1)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.mesh_orientation(v[:5], t)
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="finite"):
        ops.mesh_self_intersections(bad, t)

"""GPU suite of the mesh queries (kpx_raycast.hip; AC14): the device hierarchy == the device's brute form == the restatement
tests/raycast_ref.py, bit for bit, for every output of every query -- on marching-cubes meshes of several sizes, triangle counts that
sit on the tree's leaf and fan-out boundaries (read from include/kinectpx.h), hand-built degenerate cases, and rays and points placed
on the geometry's edges: on vertices, along edges, in a triangle's plane, axis-parallel with both zeros, invalid."""
import functools
import os
import re

import numpy as np
import pytest

import raycast_ref as R
import tsdf_mesh_ref as M

pytestmark = pytest.mark.gpu

_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kinectpx.h")).read()
_define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, _HEADER).group(1))
LEAF, FAN = _define("KPX_RAYSCENE_LEAF"), _define("KPX_RAYSCENE_FANOUT")
SIZES = [0, 1, LEAF - 1, LEAF, LEAF + 1, LEAF * FAN, LEAF * FAN + 1, LEAF * FAN * FAN + 1]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@functools.lru_cache(None)
def random_mesh(res):
    """test_mesh_ops_gpu.random_mesh restated: res 8: 458 triangles, 13: 2408, 24: 16 548"""
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
        f, w = M.sphere_volume()
        v, _, t, _ = M.extract_triangle_mesh(f, w, None, 16, 1.0, (0.0, 0.0, 0.0))
    elif name == "book":                                     # five triangles on one edge
        v, t = rng.random((7, 3)), [[0, 1, 2 + k] for k in range(5)]
    elif name == "duplicate":                                # every triangle of the book twice: a tie goes to the lower index
        v, t = rng.random((7, 3)), [[0, 1, 2 + k] for k in range(5)] * 2
    elif name == "degenerate":                               # repeated indices, collinear corners, a repeated triangle, an unused vertex
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [1, 1, 0.5], [3, 3, 3], [0.5, 0.5, 2]])
        t = [[0, 1, 3], [0, 1, 2], [1, 1, 4], [1, 4, 2], [4, 4, 4], [0, 1, 2], [2, 6, 2], [1, 2, 4]]
    elif name == "grid":                                     # flat, axis-aligned, integer corners: coplanar rays, rays along edges
        x, y = np.meshgrid(np.arange(7.0), np.arange(7.0), indexing="ij")
        v = np.stack([x, y, np.ones_like(x)], -1).reshape(-1, 3)
        i = (np.arange(6)[:, None] * 7 + np.arange(6)[None, :]).reshape(-1)
        t = np.concatenate([np.stack([i, i + 7, i + 8], 1), np.stack([i, i + 8, i + 1], 1)])
    elif name == "millimetres":                              # the resolution-8 mesh in millimetres, far from the origin
        v, t = random_mesh(8)
        v = (v.astype(np.float64) - v.astype(np.float64).mean(0)) * 1000.0 + np.array((5000.0, -3000.0, 2500.0))
    else:
        raise KeyError(name)
    return np.asarray(v, dtype=np.float32).reshape(-1, 3), np.asarray(t, dtype=np.int32).reshape(-1, 3)


def make_rays(v, t, n, seed=0):
    """n rays around a mesh: a third from random origins in and around its box towards points near its vertices, the rest placed on
    the geometry -- from a vertex, from a vertex along an edge, from outside through a vertex, axis-parallel with +0 and -0, looking
    away (hits only behind the origin) -- and a few invalid ones (zero direction, NaN, inf)"""
    rng = np.random.default_rng(seed)
    if len(t) == 0 or len(v) == 0:
        v, t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 1e-3)
    tri = v[t[rng.integers(0, len(t), n)]].astype(np.float64)                      # (n, 3, 3): a triangle per ray
    o = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (n, 3))
    d = tri.mean(1) + 0.02 * ext * rng.normal(size=(n, 3)) - o
    kind = np.arange(n) % 12
    k = kind == 1
    o[k], d[k] = tri[k, 0], rng.normal(size=(int(k.sum()), 3))                     # from a vertex
    k = kind == 2
    o[k], d[k] = tri[k, 0], tri[k, 1] - tri[k, 0]                                  # from a vertex along an edge
    k = kind == 3
    d[k] = tri[k, 2] - o[k]                                                        # through a vertex
    k = kind == 4
    axis = rng.integers(0, 3, n)
    sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    zero = np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0)
    zero[np.arange(n), axis] = sign
    o[k] = tri[k].mean(1) - 0.7 * ext * zero[k] * (np.abs(zero[k]) > 0)
    d[k] = zero[k]                                                                 # axis-parallel, towards a triangle
    k = kind == 5
    o[k], d[k] = tri[k].mean(1), zero[k]                                           # axis-parallel from (nearly) on a triangle
    k = kind == 6
    d[k] = o[k] - tri[k].mean(1)
    o[k] = hi + 0.3 * ext                                                          # outside, looking away
    rays = np.concatenate([o, d], 1).astype(np.float32)
    k = np.flatnonzero(kind == 7)
    rays[k[0::4], 3:] = 0.0
    rays[k[1::4], 3:] = (0.0, -0.0, 0.0)
    rays[k[2::4], rng.integers(0, 6, len(k[2::4]))] = np.nan
    rays[k[3::4], rng.integers(0, 6, len(k[3::4]))] = np.inf
    return rays


def make_queries(v, t, n, seed=0):
    """n points: random around the box, far outside, on vertices, on edge midpoints, in faces, NaN"""
    rng = np.random.default_rng(seed + 100)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 1e-3)
    tri = v[t[rng.integers(0, len(t), n)]].astype(np.float64)
    q = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n, 3))
    kind = np.arange(n) % 8
    q[kind == 1] = tri[kind == 1, 1]
    q[kind == 2] = 0.5 * (tri[kind == 2, 0] + tri[kind == 2, 2])
    q[kind == 3] = tri[kind == 3].mean(1)
    q[kind == 4] = lo + ext * rng.normal(size=(int((kind == 4).sum()), 3)) * 1e4
    q = q.astype(np.float32)
    k = np.flatnonzero(kind == 5)
    q[k[::3], rng.integers(0, 3, len(k[::3]))] = np.nan
    q[k[1::3], rng.integers(0, 3, len(k[1::3]))] = -np.inf
    return q


def build(geometries):
    from kinectpy_amd import o3d
    scene = o3d.t.geometry.RaycastingScene()
    for g, (v, t) in enumerate(geometries):
        assert scene.add_triangles(v, t) == g
    return scene


def assert_rays(scene, ref, rays, windows=()):
    """cast, occluded (the whole line and every window) and count: hierarchy == brute == restatement; then the NumPy interface"""
    from kinectpy_amd import ops
    s = scene._built()
    want = R.cast_rays(ref, rays)
    for brute in (False, True):
        got = host(ops.rayscene_cast(s, rays, brute=brute))
        for k in ("t", "t_hit", "primitive_uvs", "primitive_normals", "geometry_ids", "primitive_ids"):
            assert same(got[k], want[k]), (k, brute, np.flatnonzero((bits(got[k]) != bits(want[k])).reshape(len(rays), -1).any(1))[:5])
        assert np.array_equal(ops.rayscene_count(s, rays, brute=brute).cpu().numpy(), R.count_intersections(ref, rays))
        for tnear, tfar in ((0.0, np.inf),) + tuple(windows):
            assert np.array_equal(ops.rayscene_occluded(s, rays, tnear, tfar, brute=brute).cpu().numpy() != 0, R.test_occlusions(ref, rays, tnear, tfar))
    out = scene.cast_rays(rays)
    assert out["geometry_ids"].dtype == np.uint32 and out["primitive_ids"].dtype == np.uint32 and out["t_hit"].dtype == np.float32
    assert same(out["t_hit"], want["t_hit"]) and np.array_equal(out["primitive_ids"], want["primitive_ids"].view(np.uint32))
    miss = np.isinf(want["t_hit"])
    assert (out["geometry_ids"][miss] == scene.INVALID_ID).all() and (out["primitive_ids"][miss] == scene.INVALID_ID).all()
    return want


def assert_closest(scene, ref, q):
    from kinectpy_amd import ops
    s = scene._built()
    want = R.closest_points(ref, q)
    for brute in (False, True):
        got = host(ops.rayscene_closest(s, q, brute=brute))
        for k in ("d2", "points", "distance", "geometry_ids", "primitive_ids"):
            assert same(got[k], want[k]), (k, brute, np.flatnonzero((bits(got[k]) != bits(want[k])).reshape(len(q), -1).any(1))[:5])
    out = scene.compute_closest_points(q)
    assert same(out["points"], want["points"]) and np.array_equal(out["primitive_ids"], want["primitive_ids"].view(np.uint32))
    assert same(scene.compute_distance(q), want["distance"])
    return want


def windows_of(want):
    """(tnear, tfar) pairs that cut the hits: around the median hit, exactly one hit's t, and an empty window"""
    t = want["t"][np.isfinite(want["t"])]
    if len(t) == 0:
        return ((0.5, 2.0),)
    med = float(np.median(t))
    return ((med, np.inf), (0.0, med), (med, med), (float(t.max()) * 2 + 1.0, np.inf), (2.0, 1.0))


@pytest.mark.parametrize("name,n_rays,n_queries", [("res-8", 700, 300), ("res-13", 500, 200), ("res-24", 300, 100), ("sphere", 600, 300),
                                                   ("millimetres", 600, 300), ("book", 300, 200), ("duplicate", 300, 200),
                                                   ("degenerate", 300, 200), ("grid", 300, 200)])
def test_mesh(name, n_rays, n_queries):
    v, t = mesh(name)
    scene, ref = build([(v, t)]), R.Scene([(v, t)])
    rays = make_rays(v, t, n_rays)
    want = assert_rays(scene, ref, rays)
    assert_rays(scene, ref, rays[:64], windows_of(want))
    hit = np.isfinite(want["t"])
    assert hit.sum() > n_rays // 6 and (~hit).sum() > n_rays // 12
    if name == "duplicate":
        assert (want["primitive_ids"][hit] < 5).all()
    got = assert_closest(scene, ref, make_queries(v, t, n_queries))
    assert (got["primitive_ids"] >= 0).sum() > n_queries // 2 and (got["primitive_ids"] < 0).sum() > 0


@pytest.mark.parametrize("n", SIZES)
def test_triangle_counts_on_the_tree_boundaries(n):
    v, t = mesh(f"cut-{n}")
    assert len(t) == n
    scene, ref = build([(v, t)]), R.Scene([(v, t)])
    rays = make_rays(v, t, 200, seed=n)
    want = assert_rays(scene, ref, rays)
    q = make_queries(v, t, 100, seed=n) if n else np.zeros((3, 3), np.float32)
    if n == 0:
        assert np.isinf(want["t_hit"]).all()
        with pytest.raises(RuntimeError, match="no triangle"):
            scene.compute_closest_points(q)
    else:
        assert np.isfinite(want["t_hit"]).any()
        assert_closest(scene, ref, q)


@functools.lru_cache(None)
def many_rays():
    v, t = mesh("res-8")
    rays = make_rays(v, t, 4097, seed=3)
    ref = R.Scene([(v, t)])
    return rays, R.cast_rays(ref, rays), R.count_intersections(ref, rays)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_ray_counts(n):
    """the last block of a launch is full, one short, one over; results are per ray, so a prefix of the rays gives a prefix of them"""
    rays, want, count = many_rays()
    scene = build([mesh("res-8")])
    lead = (n,) if n != 64 else (4, 16)
    out = scene.cast_rays(rays[:n].reshape(lead + (6,)))
    assert out["t_hit"].shape == lead and out["primitive_uvs"].shape == lead + (2,) and out["primitive_normals"].shape == lead + (3,)
    assert same(out["t_hit"].reshape(-1), want["t_hit"][:n]) and same(out["primitive_uvs"].reshape(-1, 2), want["primitive_uvs"][:n])
    assert same(out["primitive_normals"].reshape(-1, 3), want["primitive_normals"][:n])
    assert np.array_equal(out["primitive_ids"].reshape(-1), want["primitive_ids"][:n].view(np.uint32))
    cnt = scene.count_intersections(rays[:n].reshape(lead + (6,)))
    assert cnt.dtype == np.int32 and cnt.shape == lead and np.array_equal(cnt.reshape(-1), count[:n])
    occ = scene.test_occlusions(rays[:n].reshape(lead + (6,)))
    assert occ.dtype == bool and occ.shape == lead and np.array_equal(occ.reshape(-1), np.isfinite(want["t"][:n]))
    q = np.zeros(lead + (3,), np.float32)
    if n:
        assert scene.compute_distance(q).shape == lead and scene.compute_closest_points(q)["points"].shape == lead + (3,)
        assert scene.compute_occupancy(q).shape == lead and scene.compute_signed_distance(q).shape == lead


def test_hand_placed_rays_and_points():
    """one triangle with integer corners: every special position is exact in float32"""
    v = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1], [0, 0, 3]], np.float32)
    t = np.array([[0, 1, 2], [0, 1, 3]], np.int32)
    scene, ref = build([(v, t)]), R.Scene([(v, t)])
    rays = np.array([[1, 1, 0, 0, 0, 1], [1, 1, 1, 0, 0, 1], [1, 1, 1, 0, -0.0, -1], [0, 0, 1, 0, 0, 1], [2, 0, 1, 0, 0, 1], [2, 2, 1, 1, 1, 0],
                     [-1, 1, 1, 1, 0, 0], [-1, 0, 1, 1, 0, -0.0], [1, 1, 2, 0, 0, 1], [1, 1, 0, 0, 0, 1e-30], [1, 1, 0, 0, 0, 1e30],
                     [2, 2, 0, 0, 0, 1], [2, 2, 0, 1e-20, 0, 1], [1, 0, 5, 0, 0, -1], [1, -1, 2, 0, 1, 0]], np.float32)
    want = assert_rays(scene, ref, rays, ((1.0, 1.0), (0.0, 0.5), (1.5, np.inf)))
    assert want["t_hit"][:5].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and np.isinf(want["t_hit"][8])
    assert want["primitive_ids"][3] == 0 and (want["primitive_ids"][13], want["t_hit"][13]) == (0, 4.0) and (want["primitive_ids"][14], want["t_hit"][14]) == (1, 1.0)
    q = np.array([[0, 0, 1], [2, 0, 1], [1, 1, 1], [1, 0, 0], [1, -1, 1], [1e6, 1e6, -1e6], [np.nan, 0, 0], [2, 2, 1], [1, 0, 2]], np.float32)
    got = assert_closest(scene, ref, q)
    assert got["primitive_ids"].tolist() == [0, 0, 0, 0, 0, 0, -1, 0, 1] and got["distance"][:4].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_two_geometries_and_a_later_add():
    va, ta = mesh("sphere")
    vb, tb = mesh("res-8")
    vb = ((vb - vb.mean(0)) * 40.0 + np.float32(8.0)).astype(np.float32)       # the random mesh laid over the sphere
    scene, ref = build([(va, ta)]), R.Scene([(va, ta)])
    rays, q = make_rays(va, ta, 300, seed=5), np.concatenate([make_queries(va, ta, 100, seed=5), make_queries(vb, tb, 50, seed=6)])
    first = assert_rays(scene, ref, rays)
    assert_closest(scene, ref, q)
    assert scene.add_triangles(vb, tb) == 1
    ref = R.Scene([(va, ta), (vb, tb)])
    second = assert_rays(scene, ref, rays)
    got = assert_closest(scene, ref, q)
    assert set(np.unique(second["geometry_ids"])) == {-1, 0, 1} and set(np.unique(got["geometry_ids"])) == {-1, 0, 1}
    assert (second["primitive_ids"][second["geometry_ids"] == 1] < len(tb)).all() and not same(first["t"], second["t"])
    from kinectpy_amd import o3d
    m = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(vb), o3d.utility.Vector3iVector(tb))
    assert scene.add_triangles(m) == 2
    third = scene.cast_rays(rays)                                                    # the same triangles again: the lower geometry wins
    assert same(third["t_hit"], second["t_hit"]) and np.array_equal(third["geometry_ids"], second["geometry_ids"].view(np.uint32))


def test_occupancy_and_signed_distance():
    v, t = mesh("sphere")
    scene, ref = build([(v, t)]), R.Scene([(v, t)])
    q = np.random.default_rng(4).uniform(0.5, 15.5, (5, 60, 3)).astype(np.float32)
    occ, sd = scene.compute_occupancy(q), scene.compute_signed_distance(q)
    assert occ.dtype == np.float32 and occ.shape == (5, 60) and sd.dtype == np.float32 and sd.shape == (5, 60)
    assert np.array_equal(occ.reshape(-1) != 0, R.occupancy(ref, q)) and same(sd.reshape(-1), R.signed_distance(ref, q))
    r = np.linalg.norm(q - np.array((7.3, 8.1, 6.6)), axis=2)
    assert (occ[r < 5.0] == 1).all() and (occ[r > 5.6] == 0).all() and (sd[r < 5.0] < 0).all() and (sd[r > 5.6] > 0).all()
    dev = scene.compute_signed_distance(q, device=True)
    assert dev.is_cuda and same(dev.cpu().numpy(), sd)
    with pytest.raises(NotImplementedError):
        scene.compute_occupancy(q, nsamples=5)


def test_a_repeated_call_repeats_its_bits():
    v, t = mesh("res-13")
    rays, q = make_rays(v, t, 500, seed=9), make_queries(v, t, 200, seed=9)
    a, b = build([(v, t)]), build([(v, t)])
    from kinectpy_amd import ops
    for brute in (False, True):
        x, y, z = (host(ops.rayscene_cast(s._built(), rays, brute=brute)) for s in (a, a, b))
        assert all(same(x[k], y[k]) and same(x[k], z[k]) for k in x)
        x, y, z = (host(ops.rayscene_closest(s._built(), q, brute=brute)) for s in (a, a, b))
        assert all(same(x[k], y[k]) and same(x[k], z[k]) for k in x)


def test_a_buffer_that_is_no_scene_is_rejected():
    import torch
    from kinectpy_amd import _lib, ops
    scene = build([mesh("book")])._built()
    rays = make_rays(*mesh("book"), 8)
    with pytest.raises(_lib.KinectPxError, match="holds no scene"):
        ops.rayscene_cast(ops.RayScene(torch.zeros_like(scene.buf), 5), rays)
    with pytest.raises(_lib.KinectPxError, match="scene_bytes"):
        ops.rayscene_cast(ops.RayScene(scene.buf[:64].clone(), 5), rays)
    with pytest.raises(_lib.KinectPxError, match="out of range"):
        ops.rayscene_build(np.zeros((3, 3), np.float32), np.array([[0, 1, 3]], np.int32))
    with pytest.raises(_lib.KinectPxError, match="not finite"):
        ops.rayscene_build(np.full((3, 3), np.inf, np.float32), np.array([[0, 1, 2]], np.int32))


def test_render_mesh_depth_on_the_ring():
    """the resolution-32 ring through fuse_depth_tsdf(mesh=True), rendered from the ring's own sensors at 80 x 72"""
    from kinectpy_amd import o3d
    from kinectpy_amd.preprocessing.fusion import fuse_depth_tsdf, render_mesh_depth
    from kinectpy_amd.utils import synth
    W, H, K4 = 80, 72, (63.0, 63.0, 40.0, 36.0)
    intrinsic = o3d.camera.PinholeCameraIntrinsic(W, H, *K4)
    _, depth, rgb, _, truth = synth.sensor_ring(4, xy=synth.small_xy(8))
    m = fuse_depth_tsdf(depth[0], rgb[0], intrinsic, truth, 2000.0, 32, (-1000.0, -1100.0, 1500.0), mesh=True)
    v, t = m._vert.cpu().numpy(), m._tri.cpu().numpy()
    assert len(t) > 500
    img = render_mesh_depth(m, intrinsic, truth)
    assert img.shape == (4, H, W) and img.dtype == np.float32
    ref = R.Scene([(v, t)])
    for s, E in enumerate([np.eye(4)] + [np.linalg.inv(T) for T in truth]):
        rays = R.create_rays_pinhole(intrinsic.intrinsic_matrix, E, W, H, 0.0)
        want = R.cast_rays(ref, rays)["t_hit"].reshape(H, W)
        want = np.where(np.isfinite(want), want, np.float32(0.0)).astype(np.float32)
        assert same(img[s], want), s
        raw = depth[0, s].reshape(H, W).astype(np.float64)
        both = (img[s] > 0) & (raw > 0)
        assert both.sum() > 100
        print(f"sensor {s}: {int((img[s] > 0).sum())} pixels rendered, {int(both.sum())} with a raw depth, median |rendered - raw| = "
              f"{np.median(np.abs(img[s][both] - raw[both])):.2f} mm")
        # the surface lies within the truncation band of the depth it was fused from: 4 voxels of 62.5 mm
        assert np.median(np.abs(img[s][both] - raw[both])) < 250.0
    assert same(render_mesh_depth(m, intrinsic, truth, 40, 36)[0], render_mesh_depth(m, intrinsic, truth, 40, 36)[0])

"""CPU suite of the mesh queries (AC14): the restatement tests/raycast_ref.py judged by the properties a correct
ray cast and a correct closest point must have, the claim that the contract's two box clauses decide nothing on ordinary data,
create_rays_pinhole, and RaycastingScene's argument checks, which must fire before a device is looked for."""
import functools

import numpy as np
import pytest

import raycast_ref as R
import tsdf_mesh_ref as M

CENTRE, RADIUS = np.array((7.3, 8.1, 6.6)), 5.3


@functools.lru_cache(None)
def sphere():
    f, w = M.sphere_volume()
    v, _, t, _ = M.extract_triangle_mesh(f, w, None, 16, 1.0, (0.0, 0.0, 0.0))
    return v, t, R.Scene([(v, t)])


@functools.lru_cache(None)
def soup(scale, offset):
    """200 random triangles of edge ~0.3 in the unit cube, scaled and moved"""
    rng = np.random.default_rng(5)
    c = rng.random((200, 1, 3)) + 0.3 * (rng.random((200, 3, 3)) - 0.5)
    v = (c.reshape(-1, 3) * scale + np.asarray(offset)).astype(np.float32)
    return v, np.arange(600).reshape(-1, 3), R.Scene([(v, np.arange(600).reshape(-1, 3))])


def grid():
    """a flat axis-aligned 6 x 6 grid of squares at z = 1, two triangles each"""
    x, y = np.meshgrid(np.arange(7.0), np.arange(7.0), indexing="ij")
    v = np.stack([x, y, np.ones_like(x)], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(6)[:, None] * 7 + np.arange(6)[None, :]).reshape(-1)
    t = np.concatenate([np.stack([i, i + 7, i + 8], 1), np.stack([i, i + 8, i + 1], 1)])
    return v, t, R.Scene([(v, t)])


def centre_rays(n, seed=0):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return np.concatenate([np.broadcast_to(CENTRE, (n, 3)), d], 1).astype(np.float32)


def test_rays_from_the_centre_of_the_sphere_hit_once():
    v, t, scene = sphere()
    rays = centre_rays(400)
    assert np.array_equal(R.count_intersections(scene, rays), np.ones(400, np.int32))
    out = R.cast_rays(scene, rays)
    c32 = CENTRE.astype(np.float32).astype(np.float64)
    n = M._normalize(M._cross(v, t))
    plane = np.abs((n * (v.astype(np.float64)[t[:, 0]] - c32)).sum(1))
    reach = out["t"] * np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1)
    assert (reach >= plane.min() * (1 - 1e-12)).all() and (reach <= np.linalg.norm(v - c32, axis=1).max() * (1 + 1e-12)).all()
    assert (out["geometry_ids"] == 0).all() and (out["primitive_ids"] >= 0).all() and (out["primitive_ids"] < len(t)).all()
    uv = out["primitive_uvs"].astype(np.float64)
    assert (uv >= 0).all() and (uv.sum(1) <= 1 + 1e-6).all()
    # the hit point o + t d equals the barycentric point (1 - u - v) v0 + u v1 + v v2 of the reported triangle
    tri = v.astype(np.float64)[t[out["primitive_ids"]]]
    p_ray = rays[:, :3].astype(np.float64) + out["t"][:, None] * rays[:, 3:].astype(np.float64)
    p_tri = tri[:, 0] + uv[:, :1] * (tri[:, 1] - tri[:, 0]) + uv[:, 1:] * (tri[:, 2] - tri[:, 0])
    assert np.abs(p_ray - p_tri).max() < 1e-4                  # float32 u, v on triangles of edge ~1 at coordinates ~16
    assert np.array_equal(out["primitive_normals"], M.triangle_normals(v, t)[out["primitive_ids"]])
    assert R.test_occlusions(scene, rays).all() and not R.test_occlusions(scene, rays, 0.0, 1e-3).any()
    back = rays.copy()
    back[:, :3] = (c32 + 20.0 * rays[:, 3:] / np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)).astype(np.float32)
    assert not R.count_intersections(scene, back).any()         # outside, looking away: every hit lies behind the origin


def test_occupancy_and_signed_distance_on_the_sphere():
    _, _, scene = sphere()
    q = np.random.default_rng(1).uniform(0.5, 15.5, (400, 3)).astype(np.float32)
    r = np.linalg.norm(q - CENTRE, axis=1)
    inside, outside = r < RADIUS - 0.3, r > RADIUS + 0.3           # the mesh lies within a fraction of a voxel of the sphere
    assert inside.sum() > 30 and outside.sum() > 200
    occ = R.occupancy(scene, q)
    assert occ[inside].all() and not occ[outside].any()
    sd = R.signed_distance(scene, q)
    assert (sd[inside] < 0).all() and (sd[outside] > 0).all()
    assert np.abs(np.abs(sd[inside | outside]) - np.abs(r[inside | outside] - RADIUS)).max() < 0.3


def test_the_closest_point_lies_in_its_triangle_and_beats_its_samples():
    v, t, scene = sphere()
    q = np.random.default_rng(2).uniform(0.0, 16.0, (300, 3)).astype(np.float32)
    out = R.closest_points(scene, q)
    assert (out["geometry_ids"] == 0).all()
    tri = v.astype(np.float64)[t[out["primitive_ids"]]]
    p = out["points"].astype(np.float64)
    # rounding the fp64 point to float32 moves a coordinate below 16 by at most 2^-24 16 ~ 1e-6: within 2e-6 of the plane and of
    # the three edge half-planes
    n = M._normalize(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
    assert np.abs(((p - tri[:, 0]) * n).sum(1)).max() < 2e-6
    for k in range(3):
        a, b = tri[:, k], tri[:, (k + 1) % 3]
        inward = np.cross(n, M._normalize(b - a))
        assert (((p - a) * inward).sum(1) > -2e-6).all()
    w = np.random.default_rng(3).dirichlet((1.0, 1.0, 1.0), 200)
    samples = np.einsum("sk,qkc->qsc", w, tri)
    d2 = ((q.astype(np.float64)[:, None, :] - samples) ** 2).sum(2).min(1)
    assert (out["d2"] <= d2 * (1 + 1e-12)).all()
    assert np.array_equal(out["distance"], np.sqrt(out["d2"]).astype(np.float32))
    # and no triangle of the mesh has a nearer sample
    every = np.einsum("sk,tkc->tsc", w[:20], v.astype(np.float64)[t]).reshape(-1, 3)
    for i in range(0, 300, 30):
        assert out["d2"][i] <= ((q[i].astype(np.float64) - every) ** 2).sum(1).min() * (1 + 1e-12)


def test_closest_point_regions():
    """one triangle, queries over each of the seven regions: vertices, edges, face"""
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float32)
    scene = R.Scene([(v, [[0, 1, 2]])])
    q = np.array([[-1, -1, 1], [3, -1, 0], [-1, 3, 2], [1, -1, 0], [-1, 1, 0], [2, 2, 0], [0.5, 0.5, 3], [0, 0, 0], [1, 0, 0]], np.float32)
    want = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0], [0, 0, 0], [1, 0, 0]], np.float32)
    out = R.closest_points(scene, q)
    assert np.array_equal(out["points"], want)
    assert np.array_equal(out["d2"], ((q.astype(np.float64) - want) ** 2).sum(1))
    nan = R.closest_points(scene, np.array([[np.nan, 0, 0], [np.inf, 0, 0]], np.float32))
    assert np.isnan(nan["points"]).all() and np.isnan(nan["distance"]).all() and (nan["primitive_ids"] == -1).all()
    with pytest.raises(RuntimeError):
        R.closest_points(R.Scene([]), q)


def test_ties_and_invalid_rays():
    v = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)
    scene = R.Scene([(v, [[0, 1, 2]]), (v, [[0, 1, 2], [0, 1, 2]])])
    rays = np.array([[0.25, 0.25, 0, 0, 0, 2], [0.25, 0.25, 0, 0, 0, 0], [0.25, 0.25, 0, 0, 0, np.nan], [np.inf, 0.25, 0, 0, 0, 1],
                     [0.25, 0.25, 2, 0, 0, 1], [0.25, 0.25, 1, 0, -0.0, 1]], np.float32)
    out = R.cast_rays(scene, rays)
    assert np.array_equal(out["t_hit"], np.array([0.5, np.inf, np.inf, np.inf, np.inf, 0.0], np.float32))
    assert out["geometry_ids"].tolist() == [0, -1, -1, -1, -1, 0] and out["primitive_ids"].tolist() == [0, -1, -1, -1, -1, 0]
    assert R.count_intersections(scene, rays).tolist() == [3, 0, 0, 0, 0, 3]
    assert R.test_occlusions(scene, rays, 0.5, 0.5).tolist() == [True, False, False, False, False, False]
    assert R.test_occlusions(scene, rays, 0.6, 9.0).tolist() == [False] * 6
    assert np.array_equal(out["primitive_normals"][0], np.array([0, 0, 1], np.float32)) and not out["primitive_normals"][1].any()


def test_the_box_clauses_decide_nothing():
    """share of Moeller-Trumbore hits the t-interval clause removes: 0; share of pairs where gap2 exceeds the distance: 0 -- on the
    sphere, on triangle soups at unit scale and at millimetre scale far from the origin, and on a flat axis-aligned grid with
    axis-parallel rays through its vertices and along its edges"""
    rng = np.random.default_rng(11)
    total = 0
    for v, t, scene in (sphere(), soup(1.0, (0.0, 0.0, 0.0)), soup(1000.0, (5000.0, -3000.0, 2500.0))):
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        o = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (600, 3))
        target = v[rng.integers(0, len(v), 600)] + 0.05 * (hi - lo) * rng.normal(size=(600, 3))
        (ri, _, _, _, _), removed = R.hits(scene, np.concatenate([o, target - o], 1).astype(np.float32))
        assert len(ri) > 300 and removed == 0
        total += len(ri)
        q = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (100, 3))
        D, _, dd, gap = R.closest_all(scene, np.concatenate([q, v[:50]]).astype(np.float32))
        assert not (gap > dd).any() and not np.isnan(D[:, (scene.hi - scene.lo).min(1) > 0]).all(0).any()
    v, t, scene = grid()
    x, y = np.meshgrid(np.arange(7.0), np.arange(7.0), indexing="ij")
    n = x.size
    down = np.stack([x.ravel(), y.ravel(), np.full(n, 3.0), np.zeros(n), -np.zeros(n), np.full(n, -1.0)], 1)
    along = np.stack([np.full(n, -1.0), y.ravel(), np.ones(n), np.ones(n), np.zeros(n), -np.zeros(n)], 1)
    (ri, _, tt, _, _), removed = R.hits(scene, np.concatenate([down, along]).astype(np.float32))
    assert removed == 0 and len(ri) >= n and (tt[ri < n] == 2.0).all()
    assert total + len(ri) > 1500


def test_create_rays_pinhole():
    from kinectpy_amd.geometry import RaycastingScene
    K = np.array([[63.0, 0.0, 40.25], [0.0, 61.5, 36.0], [0.0, 0.0, 1.0]])
    rays = RaycastingScene.create_rays_pinhole(K, np.eye(4), 80, 72, pixel_center=0.0)
    assert rays.shape == (72, 80, 6) and rays.dtype == np.float32
    y, x = np.meshgrid(np.arange(72.0), np.arange(80.0), indexing="ij")
    want = np.stack([(x - 40.25) / 63.0, (y - 36.0) / 61.5, np.ones_like(x)], -1).astype(np.float32)
    assert np.array_equal(rays[:, :, 3:], want) and not rays[:, :, :3].any()
    E = np.eye(4)
    E[:3, :3] = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
    E[:3, 3] = (10.0, -20.0, 30.0)
    for c in (0.5, 0.0):
        got = RaycastingScene.create_rays_pinhole(intrinsic_matrix=K, extrinsic_matrix=E, width_px=9, height_px=7, pixel_center=c)
        assert np.array_equal(got.view(np.uint32), R.create_rays_pinhole(K, E, 9, 7, c).view(np.uint32))
    assert np.allclose(got[0, 0, :3], -E[:3, :3].T @ E[:3, 3], rtol=1e-6)
    # the field-of-view form: an orthonormal camera frame, recovered from the rays through the central pixel and its neighbours
    W, H, fov = 64, 48, 70.0
    eye, centre = np.array((1.0, 2.0, 3.0)), np.array((-2.0, 0.5, 9.0))
    rays = RaycastingScene.create_rays_pinhole(fov, centre, eye, (0.1, 1.0, 0.2), W, H, pixel_center=0.0).astype(np.float64)
    assert np.array_equal(rays[:, :, :3].reshape(-1, 3), np.broadcast_to(eye, (W * H, 3)))
    f = 0.5 * W / np.tan(np.deg2rad(0.5 * fov))
    z = rays[H // 2, W // 2, 3:]
    xr, yr = (rays[H // 2, W // 2 + 8, 3:] - z) * (f / 8), (rays[H // 2 + 8, W // 2, 3:] - z) * (f / 8)
    Rm = np.stack([xr, yr, z])
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-5 and np.linalg.det(Rm) > 0.999
    assert np.abs(z - (centre - eye) / np.linalg.norm(centre - eye)).max() < 1e-6
    for bad in ((K, np.eye(3), 4, 4), (K, np.eye(4), 4), (200.0, centre, eye, (0, 1, 0), 4, 4)):
        with pytest.raises(RuntimeError, match="create_rays_pinhole"):
            RaycastingScene.create_rays_pinhole(*bad)


def test_argument_errors_are_raised_without_a_device():
    """every message below is RaycastingScene's own: a scene with host arrays never asks for the device before its arguments pass"""
    from kinectpy_amd import o3d
    assert o3d.t.geometry.RaycastingScene.INVALID_ID == 0xFFFFFFFF
    scene = o3d.t.geometry.RaycastingScene()
    v, t = np.zeros((4, 3), np.float32), np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    for bad_v, bad_t, msg in ((np.zeros((4, 2), np.float32), t, r"\(V, 3\)"), (v, t.reshape(-1), r"\(V, 3\)"), (v.astype(np.int32), t, "float32 or float64"),
                              (v, t.astype(np.float32), "must be integers"), (v, t + 2, "out of range"), (v, t - 1, "out of range"),
                              (np.full((4, 3), np.nan), t, "not finite"), (np.full((4, 3), 1e300), t, "not finite"), (v, None, "missing")):
        with pytest.raises(RuntimeError, match=msg):
            scene.add_triangles(bad_v, bad_t)
    with pytest.raises(RuntimeError, match="no triangle"):
        scene.compute_closest_points(np.zeros((2, 3), np.float32))
    assert scene.add_triangles(v.astype(np.float64), t.astype(np.int64)) == 0 and scene.add_triangles(v, t.astype(np.uint32)) == 1
    for fn in (scene.cast_rays, scene.test_occlusions, scene.count_intersections):
        with pytest.raises(RuntimeError, match="last dimension must be 6"):
            fn(np.zeros((5, 3), np.float32))
        with pytest.raises(RuntimeError, match="float32 or float64"):
            fn(np.zeros((5, 6), np.int32))
    for fn in (scene.compute_closest_points, scene.compute_distance, scene.compute_signed_distance, scene.compute_occupancy):
        with pytest.raises(RuntimeError, match="last dimension must be 3"):
            fn(np.zeros((5, 6), np.float32))
        with pytest.raises(RuntimeError, match="float32 or float64"):
            fn(np.zeros((5, 3), np.int64))
    for fn in (scene.compute_signed_distance, scene.compute_occupancy):
        with pytest.raises(NotImplementedError, match="nsamples"):
            fn(np.zeros((5, 3), np.float32), nsamples=3)
    with pytest.raises(RuntimeError, match="not a number"):
        scene.test_occlusions(np.zeros((5, 6), np.float32), tnear=float("nan"))

"""ISS keypoints on the MI355X against the float64 restatement of Open3D's ComputeISSKeypoints (tests/iss_ref.py): saliency within the
covariance tolerance wherever the reference decides, suppression index for index, the whole call on points the rounding cannot move."""
import numpy as np
import pytest
import torch

from kinectpy_amd import o3d, ops
from kinectpy_amd.geometry import PointCloud
from tests import iss_ref as R

pytestmark = pytest.mark.gpu

NEXT1 = float(np.nextafter(1.0, 2.0))


def npy(t):
    return t.cpu().numpy()


def _nonmax_both(pts, s, r, mn):
    got = npy(ops.iss_nonmax(pts, s, r, mn))
    keep, _ = R.nonmax(s, len(pts), R.radius_pairs(pts, r), mn)
    assert got.dtype == np.int32 and np.array_equal(got, np.flatnonzero(keep)), (r, mn, len(got), int(keep.sum()))
    return got


# ---- saliency parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,factor", R.PARITY_CASES)
def test_saliency_parity_and_suppression_of_it(base_cloud, name, factor):
    pts, r, pairs, ref = R.parity_reference(name, factor, base_cloud)
    n = len(pts)
    if factor > 40:
        assert ref["count"].mean() > 1100
    got = npy(ops.iss_saliency(pts, r))
    dec = ref["decided"]
    print(name, r, "neighbours", ref["count"].mean(), "undecided", int((~dec).sum()))
    assert (~dec).sum() <= 0.01 * n
    zero_ref, zero_got = ref["s"] == 0, got == 0
    assert dec[zero_ref].any() and dec[~zero_ref].any()
    assert np.array_equal(zero_got[dec], zero_ref[dec]), int((zero_got != zero_ref)[dec].sum())
    nz = dec & ~zero_ref
    err = np.abs(got - ref["s"])[nz]
    tol = R.tolerance(ref["e"][nz, 2], pts[nz].astype(np.float64))
    print("  worst error / tolerance", float((err / tol).max()))
    assert np.all(err <= tol)
    # pass 2 alone on pass 1's own output: the same doubles go through the kernel and NumPy
    keep, _ = R.nonmax(got, n, pairs, 5)
    idx = npy(ops.iss_nonmax(pts, got, r, 5))
    assert np.array_equal(idx, np.flatnonzero(keep))
    assert factor < 1 or len(idx) > 0


# ---- suppression, exact ---------------------------------------------------------------------------------------------------------------
def _lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return g[np.random.default_rng(1).permutation(len(g))]


def test_nonmax_crafted_saliencies():
    pts = _lattice(13, 11, 7)                                  # 1001 points, spacing 1
    n = len(pts)
    rng = np.random.default_rng(3)
    rand = rng.uniform(0.1, 1.0, n)
    for r in (NEXT1, 1.8, 2.5):
        for mn in (0, 1, 5, 7, 28, 10_000):
            _nonmax_both(pts, rand, r, mn)
    # all equal: every point with enough neighbours survives
    got = _nonmax_both(pts, np.full(n, 0.25), NEXT1, 6)
    cnt = R.counts(n, R.radius_pairs(pts, NEXT1))
    assert np.array_equal(got, np.flatnonzero(cnt >= 6)) and 0 < len(got) < n
    # exact ties between neighbours: both survive; a single maximum
    tie = rand.copy()
    a = int(np.flatnonzero((pts == [6, 5, 3]).all(1))[0])
    b = int(np.flatnonzero((pts == [6, 5, 4]).all(1))[0])
    tie[[a, b]] = 2.0
    got = _nonmax_both(pts, tie, NEXT1, 1)
    assert a in got and b in got
    one = np.full(n, 0.5)
    one[a] = 0.75
    got = _nonmax_both(pts, one, 1e150, 1)
    assert np.array_equal(got, [a])
    # zeros, negatives and NaN are never keypoints and never suppress a positive maximum
    mixed = rand.copy()
    mixed[::3] = 0.0
    mixed[1::3] = -rand[1::3]
    mixed[5::7] = np.nan
    for r in (NEXT1, 1.8):
        got = _nonmax_both(pts, mixed, r, 1)
        assert np.all(mixed[got] > 0)
    assert len(_nonmax_both(pts, -rand, 1.8, 0)) == 0 and len(_nonmax_both(pts, np.zeros(n), 1.8, 0)) == 0
    # radius below the spacing: every positive point is alone; min_neighbors above 1 empties the result
    got = _nonmax_both(pts, mixed, 0.5, 1)
    assert np.array_equal(got, np.flatnonzero(mixed > 0))
    assert len(_nonmax_both(pts, mixed, 0.5, 2)) == 0
    # radius 1e150: the global maximum, if the cloud is large enough
    assert np.array_equal(_nonmax_both(pts, rand, 1e150, n), [int(np.argmax(rand))])
    assert len(_nonmax_both(pts, rand, 1e150, n + 1)) == 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _end_to_end(pts, rs, rn, **kw):
    ref = R.iss_keypoints(pts, rs, rn, **kw)
    got, sal = ops.iss_keypoints(pts, rs, rn, want_saliency=True, **kw)
    got, sal = npy(got), npy(sal)
    n = len(pts)
    assert got.dtype == np.int32 and np.all(np.diff(got) > 0)
    rsal = ref["sal"]
    safe = R.safe_points(ref, pts, kw.get("min_neighbors", 5))
    print("unsafe", int((~safe).sum()), "of", n, "keypoints", len(ref["idx"]))
    assert (~safe).sum() <= 0.02 * n
    is_kp = np.zeros(n, bool)
    is_kp[got] = True
    assert np.array_equal(is_kp[safe], ref["keep"][safe]), int((is_kp != ref["keep"])[safe].sum())
    assert (safe & ref["keep"]).any() and (safe & ~ref["keep"] & (rsal["s"] > 0)).any()
    return ref, got


@pytest.mark.parametrize("shape,rs,rn", R.SLAB_CASES)
def test_keypoints_explicit_radii(shape, rs, rn):
    _end_to_end(R.bumpy_slab(*shape, seed=6), rs, rn)


def test_keypoints_default_radii_and_resolution():
    pts = R.bumpy_slab(*R.SLAB_DEFAULT, seed=4)
    res = R.resolution(pts)
    g = ops.model_resolution(pts)
    assert g.dtype == torch.float64 and g.is_cuda and abs(float(g) - res) <= 1e-12 * res
    assert float(ops.model_resolution(pts)) == float(g)
    # no pair distance within 1e-9 relative of either defaulted radius: the 1e-12 on the resolution cannot move a neighbour set
    p64 = pts.astype(np.float64)
    for r in (6.0 * res, 4.0 * res):
        wide = R.radius_pairs(pts, r * (1 + 2e-9))
        d = np.sqrt(((p64[wide[:, 0]] - p64[wide[:, 1]]) ** 2).sum(1))
        assert not np.any(np.abs(d - r) <= 1e-9 * r)
    ref, got = _end_to_end(pts, 0.0, 0.0)
    assert ref["radii"] == (6.0 * res, 4.0 * res)
    # one radius given, the other 0: both are replaced
    assert np.array_equal(npy(ops.iss_keypoints(pts, 123.0, 0.0)), got) and np.array_equal(npy(ops.iss_keypoints(pts, 0.0, 7.0)), got)


# ---- geometry with a known answer -----------------------------------------------------------------------------------------------------
def test_corner_of_three_planes():
    """three 40 x 40 unit lattices in the coordinate planes, jittered by 0.01: away from the axes (where two planes meet) and from its
    own rim a plane's neighbourhood is a symmetric disc -- e2 / e1 is 1 up to the jitter, far above gamma_21 -- so no keypoint may lie
    there; the radii sit between lattice distances (3 < 3.08 < sqrt 10, 2 < 2.05 < sqrt 5), out of the jitter's reach"""
    rng = np.random.default_rng(11)
    u, v = np.meshgrid(np.arange(40, dtype=np.float64), np.arange(40, dtype=np.float64), indexing="ij")
    u, v, z = u.ravel(), v.ravel(), np.zeros(1600)
    planes = [np.stack(c, 1) for c in ((u, v, z), (u, z, v), (z, u, v))]
    pts = (np.concatenate(planes) + rng.normal(scale=0.01, size=(4800, 3))).astype(np.float32)
    rs, rn = 3.08, 2.05
    kp = npy(ops.iss_keypoints(pts, rs, rn, 0.975, 0.975, 5))
    assert len(kp) > 0
    uu, vv = np.tile(u, 3), np.tile(v, 3)
    to_axis, to_rim = np.minimum(uu, vv), np.minimum(39 - uu, 39 - vv)       # in-plane distances to the axes / to the plane's outer rim
    interior = np.minimum(to_axis, to_rim) >= rs + 0.1
    assert interior.sum() > 3000 and not interior[kp].any()
    assert (to_axis[kp] < rs).any()                                           # some keypoints sit on the edges between the planes
    assert np.all(npy(ops.iss_saliency(pts, rs))[interior] == 0)


# ---- edge shapes ----------------------------------------------------------------------------------------------------------------------
def test_edge_shapes():
    empty = np.zeros((0, 3), np.float32)
    assert ops.iss_saliency(empty, 1.0).shape == (0,) and len(ops.iss_nonmax(empty, np.zeros(0), 1.0)) == 0
    assert len(ops.iss_keypoints(empty)) == 0 and len(ops.iss_keypoints(empty, 1.0, 1.0)) == 0 and float(ops.model_resolution(empty)) == 0.0
    one = np.array([[1.5, -2.0, 3.0]], np.float32)
    assert npy(ops.iss_saliency(one, 1.0, min_neighbors=0)).tolist() == [0.0] and len(ops.iss_keypoints(one)) == 0
    assert len(ops.iss_keypoints(one, 1.0, 1.0, min_neighbors=0)) == 0
    rng = np.random.default_rng(2)
    four = rng.normal(size=(4, 3)).astype(np.float32)              # n = min_neighbors - 1
    assert np.all(npy(ops.iss_saliency(four, 100.0)) == 0) and len(ops.iss_keypoints(four, 100.0, 100.0)) == 0
    assert np.all(npy(ops.iss_saliency(four, 100.0, 2.0, 2.0, min_neighbors=4)) > 0)       # ratios never reach 2
    same = np.tile(np.array([[3.25, -7.5, 1000.0]], np.float32), (300, 1))
    assert np.all(npy(ops.iss_saliency(same, 1.0)) == 0) and len(ops.iss_keypoints(same, 1.0, 1.0)) == 0 and len(ops.iss_keypoints(same)) == 0
    line = np.stack([np.arange(200.0), 2 * np.arange(200.0), -np.arange(200.0)], 1).astype(np.float32)
    s = npy(ops.iss_saliency(line, 20.0))
    ref = R.saliency(line, R.radius_pairs(line, 20.0))
    assert np.all(np.abs(s) <= R.tolerance(ref["e"][:, 2], line.astype(np.float64)))          # e3 = e2 = 0 up to rounding
    flat = np.concatenate([rng.uniform(0, 50, (3000, 2)), np.full((3000, 1), 7.0)], 1).astype(np.float32)      # bounding box flat in z
    s = npy(ops.iss_saliency(flat, 4.0))
    assert np.all(s == 0) and len(ops.iss_keypoints(flat, 4.0, 3.0)) == 0
    flat_ref = R.iss_keypoints(flat, 4.0, 3.0, min_neighbors=5)
    assert (flat_ref["sal"]["count"] >= 5).mean() > 0.9
    # strict <: two points at distance exactly 1
    two = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    assert npy(ops.iss_nonmax(two, [1.0, 2.0], 1.0, 1)).tolist() == [0, 1] and npy(ops.iss_nonmax(two, [1.0, 2.0], NEXT1, 1)).tolist() == [1]
    assert npy(ops.iss_nonmax(two, [1.0, 2.0], 1.0, 2)).tolist() == [] and npy(ops.iss_nonmax(two, [1.0, 2.0], NEXT1, 2)).tolist() == [1]
    assert np.all(npy(ops.iss_saliency(two, 1.0, min_neighbors=1)) == 0)                        # alone: zero covariance
    s2 = npy(ops.iss_saliency(two, NEXT1, min_neighbors=1, gamma_21=2.0, gamma_32=2.0))         # together: C = diag(1/4, 0, 0)
    assert np.all(s2 == 0)                                                                      # e3 / e2 = 0 / 0 is NaN: fails
    # non-contiguous and float64 inputs
    pts, h = R.parity_cloud("base4k")
    r = float(np.round(5.6 * h, 3))
    want = npy(ops.iss_saliency(pts, r))
    wide = np.zeros((len(pts), 5), np.float64)
    wide[:, 1:4] = pts
    assert np.array_equal(npy(ops.iss_saliency(wide[:, 1:4], r)), want)
    assert np.array_equal(npy(ops.iss_saliency(torch.as_tensor(wide).cuda()[:, 1:4], r)), want)
    assert np.array_equal(npy(ops.iss_nonmax(wide[:, 1:4], torch.as_tensor(want).cuda()[::1], r, 5)), npy(ops.iss_nonmax(pts, want, r, 5)))
    with pytest.raises(RuntimeError):
        ops.iss_saliency(pts, -1.0)
    with pytest.raises(RuntimeError):
        ops.iss_nonmax(pts, want, float("inf"))
    with pytest.raises(RuntimeError):
        ops.iss_keypoints(pts, 1.0, 1.0, min_neighbors=-1)


# ---- API ------------------------------------------------------------------------------------------------------------------------------
def test_compute_iss_keypoints_and_feature_selection(base_cloud):
    pts, h = R.parity_cloud("base4k", base_cloud)
    rs, rn = float(np.round(5.6 * h, 3)), float(np.round(4.0 * h, 3))
    rng = np.random.default_rng(8)
    pc = PointCloud(pts)
    pc.colors = o3d.utility.Vector3dVector(rng.uniform(size=(len(pts), 3)))
    pc.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(radius=3 * h, max_nn=30))
    idx = npy(ops.iss_keypoints(pts, rs, rn))
    kp = o3d.geometry.keypoint.compute_iss_keypoints(pc, rs, rn)
    want = pc.select_by_index(idx)
    assert len(idx) > 0 and isinstance(kp, PointCloud) and kp.has_colors() and kp.has_normals()
    for a in ("points", "colors", "normals"):
        assert np.array_equal(np.asarray(getattr(kp, a)), np.asarray(getattr(want, a)))
    assert np.array_equal(np.asarray(kp.points), pts[idx].astype(np.float64))
    assert len(o3d.geometry.keypoint.compute_iss_keypoints(PointCloud()).points) == 0
    assert np.array_equal(npy(pc._iss_keypoint_indices(rs, rn)), idx)
    fe = o3d.pipelines.registration.compute_fpfh_feature(pc, o3d.geometry.KDTreeSearchParamHybrid(radius=5 * h, max_nn=40))
    data = fe.data
    sel, inv = fe.select_by_index(idx), fe.select_by_index(idx, invert=True)
    assert sel.num() == len(idx) and sel.dimension() == 33 and np.array_equal(sel.data, data[:, idx])
    assert np.array_equal(inv.data, np.delete(data, idx, axis=1))
    assert np.array_equal(fe.select_by_index(torch.as_tensor(idx[::-1].copy()).cuda()).data, data[:, idx])
    assert np.array_equal(fe.select_by_index([5, 2, 5]).data, data[:, [2, 5]])
    with pytest.raises(RuntimeError):
        fe.select_by_index([len(pts)])


@pytest.fixture(scope="module")
def view_clouds(oracle):
    """the two cluttered views of tests/test_global_registration_gpu.py"""
    from kinectpy_amd.utils import synth
    xy, ex = synth.xy_table(), synth.clutter()
    out = []
    for i, seed in ((0, 100), (1, 101)):
        E = synth.camera_pose(i, 16)
        dep = synth.render_depth(E, seed=seed, xy=xy, extra=ex)
        out.append((E, oracle.rgbd_compact(oracle.unproject_u16(dep, xy))[0]))
    return out


def test_global_registration_with_keypoints(view_clouds, monkeypatch):
    import time
    from kinectpy_amd.preprocessing import registration as reg
    (E0, tgt_full), (E1, src_full) = view_clouds
    voxel, trials, seed = 35.0, 3, 41
    sizes = []
    real = o3d.pipelines.registration.registration_ransac_based_on_feature_matching

    def spy(source, target, sf, tf, *a, **k):
        r = real(source, target, sf, tf, *a, **k)
        sizes.append((len(source.points), len(target.points), sf.num(), tf.num(), len(r.correspondence_set)))
        return r
    monkeypatch.setattr(o3d.pipelines.registration, "registration_ransac_based_on_feature_matching", spy)
    run = lambda **k: reg.execute_global_registration(PointCloud(tgt_full), PointCloud(src_full), voxel_size=voxel, ransac_n_trials=trials, seed=seed, **k)
    t0 = time.perf_counter()
    T_plain = run()
    t1 = time.perf_counter()
    full = sizes[-1]
    T_none = run(keypoints=None)
    assert T_plain is not None and np.array_equal(T_plain, T_none) and sizes[-1] == full
    t2 = time.perf_counter()
    T_key = run(keypoints=True)
    t3 = time.perf_counter()
    key = sizes[-1]
    print("points / features / correspondences: full", full, "keypoints", key, "wall s: full %.3f keypoints %.3f" % (t1 - t0, t3 - t2))
    assert key[0] == key[2] and key[1] == key[3] and 3 <= key[0] < full[0] and 3 <= key[1] < full[1]
    assert T_key is not None
    T_true = np.linalg.inv(E0) @ E1
    ang = np.degrees(np.arccos(np.clip((np.trace(T_key[:3, :3].T @ T_true[:3, :3]) - 1) / 2, -1, 1)))
    print("keypoints: angle", ang, "translation error", np.abs(T_key[:3, 3] - T_true[:3, 3]).max())
    assert ang < 6.0 and np.abs(T_key[:3, 3] - T_true[:3, 3]).max() < 250.0
    # a dict of ISS parameters goes through; radii that leave fewer than three keypoints fall back to the full clouds
    T_dict = run(keypoints=dict(salient_radius=6 * voxel, non_max_radius=4 * voxel))
    assert T_dict is not None and sizes[-1][0] < full[0]
    T_fallback = run(keypoints=dict(salient_radius=1e-3, non_max_radius=1e-3))
    assert sizes[-1] == full and np.array_equal(T_fallback, T_plain)

"""CPU suite: the NumPy restatement of the image operators and the RGB-D odometry (tests/odometry_ref.py) is the oracle of
tests/test_odometry_gpu.py, so it is pinned here against independent formulations, and the fixtures (tests/odometry_scenes.py) against
the conditions the GPU comparison relies on; plus the parts of the public surface that need no device.

Figures of the restatement on the fixtures (80 x 72, noise-free, millimetres, option (30, 0, 6000), motion 1.5 degrees / 40.4 mm;
spreads over three permuted summation orders, R = rotation entries, t = translation in mm, info relative to its largest entry;
margins in pixels and millimetres):

    case                        success  spread R   spread t   spread info  rounding margin  depth margin
    identity-hybrid-20-10-5     yes      1.1e-15    7.9e-12    4.8e-15      8.6e-06          2.5e-03
    perturbed-hybrid-20-10-5    yes      1.5e-15    9.0e-12    3.1e-15      4.5e-06          6.5e-03
    identity-color-20-10-5      no (no correspondence left on the 20 x 18 level)       5.7e-04          6.3e-02
    identity-hybrid-3           yes      9.0e-17    3.1e-13    4.6e-15      2.4e-05          4.8e-03
    perturbed-color-3           yes      2.8e-13    1.6e-09    2.4e-15      5.3e-06          4.8e-03
    identity-hybrid-0-0-2       yes      2.1e-16    4.3e-13    4.3e-15      6.4e-05          4.8e-03
    identity-color-0-0-2        yes      3.1e-14    1.7e-10    1.5e-15      1.0e-05          3.3e-04

    one iteration from the perturbed pose (jacobian, level): correspondences, spread of JTJ, JTr (relative), of the new pose
    colour 0 / 1 / 2            1272 / 313 / 74    2.4e-15 / 1.2e-15 / 4.4e-16    1.1e-15 / 1.7e-15 / 1.6e-16    6.1e-10 / 8.0e-10 / 2.4e-10
    hybrid 0 / 1 / 2            1272 / 313 / 74    2.5e-15 / 6.6e-16 / 5.1e-16    1.0e-15 / 5.7e-16 / 2.8e-16    5.0e-12 / 7.5e-13 / 1.1e-12

identity-hybrid-20-10-5 ends 0.31 degrees / 26.8 mm from the rendered motion (start: 1.50 degrees / 40.4 mm).
The accuracy is bounded by the fixture, not by the method: the nearest-pixel residual D_t(u_t, v_t) - p_z carries the sub-pixel offset
times the depth gradient, which on the floor of an 80 x 72 image is tens of millimetres per pixel.  The same scene at 320 x 288 gives
0.04 degrees / 0.7 mm (hybrid) and 0.02 degrees / 2.1 mm (colour).
"""
import numpy as np
import pytest
from scipy.ndimage import correlate1d

import odometry_ref as R
import odometry_scenes as S

FILTERS = [R.GAUSSIAN3, R.GAUSSIAN5, R.GAUSSIAN7, R.SOBEL3DX, R.SOBEL3DY]


# ----------------------------------------------------------------- the restatement's image operators
@pytest.mark.parametrize("kind", FILTERS)
def test_filters_equal_scipy_correlate1d(kind):
    """a direct scipy formulation: correlate1d along x in float64, rounded to float32, then along y.  scipy sums the taps in its own
    order, so the two agree within one rounding of the float64 accumulation (2^-52 relative to the sum of |tap x value|) before the
    float32 rounding -- at most one float32 ulp apart, and equal wherever that accumulation is exact"""
    rng = np.random.default_rng(3)
    for shape in ((72, 80), (53, 75)):
        a = rng.uniform(0.0, 4000.0, size=shape).astype(np.float32)
        tx, ty = R.TAPS[kind]
        want = correlate1d(a.astype(np.float64), tx, axis=1, mode="nearest").astype(np.float32)
        want = correlate1d(want.astype(np.float64), ty, axis=0, mode="nearest").astype(np.float32)
        got = R.image_filter(a, kind)
        assert got.dtype == np.float32 and got.shape == shape
        ulp = np.spacing(np.maximum(np.abs(want), np.float32(4000.0)))
        assert np.all(np.abs(got - want) <= ulp)
    small = np.arange(12, dtype=np.float32).reshape(3, 4)          # integers: every accumulation is exact
    tx, ty = R.TAPS[kind]
    want = correlate1d(correlate1d(small.astype(np.float64), tx, axis=1, mode="nearest"), ty, axis=0, mode="nearest")
    assert np.array_equal(R.image_filter(small, kind), want.astype(np.float32))


def test_sobel_of_a_ramp_and_nan_spread():
    v, u = np.mgrid[0:20, 0:30].astype(np.float32)
    ramp = 3.0 * u - 2.0 * v + 5.0
    dx, dy = R.image_filter(ramp, R.SOBEL3DX), R.image_filter(ramp, R.SOBEL3DY)
    assert np.all(dx[1:-1, 1:-1] == 8.0 * 3.0) and np.all(dy[1:-1, 1:-1] == 8.0 * -2.0)          # (-1 0 1) x (1 2 1): 2 x 4 x slope
    assert np.all(R.SOBEL_SCALE * dx[1:-1, 1:-1] == 3.0)
    assert np.all(dx[1:-1, 0] == 4.0 * 3.0)                       # the border pixel is repeated: a one-sided difference
    a = np.ones((9, 9), np.float32)
    a[4, 4] = np.nan
    g = R.image_filter(a, R.GAUSSIAN3)
    assert np.isnan(g[3:6, 3:6]).all() and np.isnan(g).sum() == 9 and np.all(g[~np.isnan(g)] == 1.0)


def test_pyramid_shapes_and_block_means():
    a = S.odd_image()
    pyr = R.create_pyramid(a, 3, False)
    assert [p.shape for p in pyr] == [(53, 75), (26, 37), (13, 18)]
    blk = a[:2, :2].astype(np.float32)
    assert np.array_equal(pyr[1][0, 0], (((blk[0, 0] + blk[0, 1]) + blk[1, 0]) + blk[1, 1]) / np.float32(4), equal_nan=True)
    assert np.isnan(pyr[1]).any() and not np.isnan(pyr[1]).all()
    g = R.create_pyramid(a, 2, True)
    assert np.array_equal(g[1], R.downsample(R.image_filter(a, R.GAUSSIAN3)), equal_nan=True)


# ----------------------------------------------------------------- correspondences
def test_collision_scene_equals_brute_force():
    ds, dt, K, T, dmax = S.collision()
    got, want = R.correspondence(K, T, ds, dt, dmax), R.correspondence_brute(K, T, ds, dt, dmax)
    assert np.array_equal(got, want) and len(got) > 1000
    tpx = got[:, 3].astype(np.int64) * S.W + got[:, 2]
    assert np.all(np.diff(tpx) > 0)                               # ascending in (v_t, u_t), one row per target pixel
    # two sources on one target exist, z' ties exactly, and the smaller source index is the one kept
    full = {}
    M, Kt = R.projection(K, T)
    for vs in range(S.H):
        for us in range(S.W):
            q = [2000.0 * ((M[i][0] * us + M[i][1] * vs) + M[i][2]) + Kt[i] for i in range(3)]
            ut, vt = int(q[0] / q[2] + 0.5), int(q[1] / q[2] + 0.5)
            assert q[2] == 2600.0
            full.setdefault((ut, vt), []).append(vs * S.W + us)
    shared = {k: v for k, v in full.items() if len(v) > 1}
    assert len(shared) > 100
    kept = {(r[2], r[3]): r[1] * S.W + r[0] for r in got.tolist()}
    assert all(kept[k] == min(v) for k, v in shared.items())


def test_pair_correspondences_equal_brute_force():
    lv = S.levels_reference()
    for level, T in ((0, np.eye(4)), (0, S.scene()["truth"]), (1, S.scene()["truth"]), (2, S.perturbed_init())):
        Kl = R.level_camera(S.K4, level)
        got = R.correspondence(Kl, T, lv[level][1], lv[level][3], 30.0)
        assert np.array_equal(got, R.correspondence_brute(Kl, T, lv[level][1], lv[level][3], 30.0)) and len(got) > 50


# ----------------------------------------------------------------- the chain
def test_restatement_moves_towards_the_rendered_motion():
    """identity-hybrid-20-10-5: the final pose is closer to the rendered motion than odo_init = I is, in angle and in translation.
    Achieved: 0.31 degrees / 26.8 mm against 1.50 degrees / 40.4 mm at the start (see the module docstring for what bounds it)."""
    truth = S.scene()["truth"]
    r = S.chain_reference("identity-hybrid-20-10-5")
    e0, e1 = S.pose_error(np.eye(4), truth), S.pose_error(r["T"], truth)
    print(f"start {e0[0]:.3f} deg {e0[1]:.2f} mm -> final {e1[0]:.3f} deg {e1[1]:.2f} mm")
    assert r["success"] and abs(e0[0] - S.MOTION_DEG) < 1e-9
    assert e1[0] < e0[0] and e1[1] < e0[1]
    Rm = r["T"][:3, :3]
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and np.array_equal(r["T"][3], [0, 0, 0, 1])
    assert np.array_equal(r["info"], r["info"].T) and np.all(np.linalg.eigvalsh(r["info"]) > 0)


@pytest.mark.parametrize("case", list(S.CHAIN_CASES))
def test_decision_margins_of_the_fixtures(case):
    """a condition on the FIXTURES: over every correspondence search of the case (normalisation, every iteration, information matrix,
    the permuted runs included) no projected coordinate comes within 1e-6 pixels of a rounding boundary and no depth difference within
    1e-6 mm of depth_diff_max, so a device pose that differs in its last bits cannot change a correspondence"""
    m = S.chain_reference(case)["margins"]
    print(f"{case}: rounding margin {m.rounding:.3e} px, depth margin {m.depth_diff:.3e} mm")
    assert m.rounding > 1e-6 and m.depth_diff > 1e-6


def test_decision_margins_of_the_given_pose_cases():
    """the correspondence and single-iteration cases of the GPU suite start from given poses"""
    lv, m = S.levels_reference(), R.Margins()
    for level in range(3):
        for T in (np.eye(4), S.scene()["truth"], S.perturbed_init()):
            R.correspondence(R.level_camera(S.K4, level), T, lv[level][1], lv[level][3], 30.0, m)
    ds, dt, K, T, dmax = S.collision()
    R.correspondence(K, T, ds, dt, dmax, m)
    print(f"rounding margin {m.rounding:.3e} px, depth margin {m.depth_diff:.3e} mm")
    assert m.rounding > 1e-6 and m.depth_diff > 1e-6


def test_summation_order_spread():
    """tabulates what the GPU suite takes its tolerances from: the largest change of T (absolute), of the information matrix and of
    one iteration's sums (relative to their largest entry) when the correspondences are summed in permuted orders.  Pure rounding: no
    run may change a success flag or an iteration's correspondence count (asserted inside the fixtures), and ten times the spread
    cannot reach a decision margin: a rotation entry off by e moves a projection by at most fx (|x| + |y| + |z|) / z e < 200 e pixels
    and z' by at most 18000 e mm (depth_max 6000), a translation off by e by at most fx / z_min e = 0.25 e pixels and e mm."""
    print("case                         success  spread R    spread t    spread info")
    for case in S.CHAIN_CASES:
        r = S.chain_reference(case)
        print(f"{case:28s} {str(r['success']):7s}  {r['spread_R']:.2e}    {r['spread_t']:.2e}    {r['spread_info']:.2e}")
        assert 10.0 * (200.0 * r["spread_R"] + 0.25 * r["spread_t"]) < r["margins"].rounding
        assert 10.0 * (18000.0 * r["spread_R"] + r["spread_t"]) < r["margins"].depth_diff
        assert r["spread_info"] < 1e-13
    print("iteration (jacobian, level)  count  spread JTJ  spread JTr  spread T")
    for jac in (R.COLOR, R.HYBRID):
        for level in range(3):
            r = S.iteration_reference(jac, level)
            print(f"({jac}, {level})                       {r['count']:5d}  {r['spread_JTJ']:.2e}    {r['spread_JTr']:.2e}    {r['spread_T']:.2e}")
            assert r["solved"] and r["count"] > 50 and r["spread_JTJ"] < 1e-13


def test_failure_inputs_of_the_restatement():
    (Is, Ds), (It, Dt) = S.images("A"), S.images("B")
    ok, T, G = R.odometry(Is, np.zeros_like(Ds), It, np.zeros_like(Dt), S.K4, None, R.HYBRID, S.option())
    assert not ok and np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6))
    flat_i, flat_d = np.full((S.H, S.W), 0.5, np.float32), np.full((S.H, S.W), 2000.0, np.float32)
    ok, T, G = R.odometry(flat_i, flat_d, flat_i, flat_d, S.K4, None, R.COLOR, S.option())
    assert not ok and np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6))
    ok, T, _ = R.odometry(Is, Ds, Is, Ds, S.K4, None, R.HYBRID, S.option())          # A -> A: zero residuals, the pose stays
    assert ok and np.abs(T - np.eye(4)).max() < 1e-12


# ----------------------------------------------------------------- public surface without a device
def test_option_aliases_and_namespace():
    from kinectpy_amd import o3d
    odo = o3d.pipelines.odometry
    o = odo.OdometryOption()
    assert o.iteration_number_per_pyramid_level == [20, 10, 5] and (o.depth_diff_max, o.depth_min, o.depth_max) == (0.03, 0.0, 4.0)
    o = odo.OdometryOption([3, 2], max_depth_diff=30, min_depth=1, max_depth=4000)
    assert (o.depth_diff_max, o.depth_min, o.depth_max) == (30.0, 1.0, 4000.0) and (o.max_depth_diff, o.min_depth, o.max_depth) == (30.0, 1.0, 4000.0)
    o.max_depth = 5000
    assert o.depth_max == 5000.0 and "depth_max = 5000" in repr(o)
    with pytest.raises(TypeError):
        odo.OdometryOption(depth_diff_max=1, max_depth_diff=2)
    with pytest.raises(RuntimeError):
        odo.OdometryOption([])
    with pytest.raises(RuntimeError):
        odo.OdometryOption([1] * 9)
    assert odo.RGBDOdometryJacobianFromColorTerm().kind == "color" and odo.RGBDOdometryJacobianFromHybridTerm().kind == "hybrid"
    assert [t.name for t in o3d.geometry.ImageFilterType] == ["Gaussian3", "Gaussian5", "Gaussian7", "Sobel3Dx", "Sobel3Dy"]
    for name in ("compute_rgbd_odometry", "compute_rgbd_odometry_batch", "compute_correspondence"):
        assert callable(getattr(odo, name))


def test_image_pair_check_returns_identities_without_a_device():
    """[O3D] CheckRGBDImagePair: anything but float32 intensity + float32 depth of the intrinsic's size -> (False, I, I)"""
    from kinectpy_amd import o3d
    odo, s = o3d.pipelines.odometry, S.scene()
    K = o3d.camera.PinholeCameraIntrinsic(S.W, S.H, *S.K4)
    good = S.rgbd(s["depth_A"], s["rgb_A"])
    rgb3 = o3d.geometry.RGBDImage.create_from_color_and_depth(s["rgb_A"].reshape(S.H, S.W, 3), s["depth_A"].reshape(S.H, S.W), 1.0, 6000.0,
                                                             convert_rgb_to_intensity=False)
    raw = o3d.geometry.RGBDImage(np.asarray(good.color), s["depth_A"].reshape(S.H, S.W))
    wrong_size = o3d.camera.PinholeCameraIntrinsic(S.W + 1, S.H, *S.K4)
    for src, tgt, k in ((rgb3, good, K), (good, raw, K), (good, good, wrong_size), (o3d.geometry.RGBDImage(), good, K)):
        ok, T, G = odo.compute_rgbd_odometry(src, tgt, k)
        assert ok is False and np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6)) and T.dtype == np.float64
    with pytest.raises(TypeError):
        odo.compute_rgbd_odometry(good, good, K, np.eye(4), object())
    with pytest.raises(RuntimeError):
        odo.compute_rgbd_odometry(good, good, K, np.eye(3))
    for bad in (np.zeros((4, 4), np.uint16), np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(RuntimeError):
            o3d.geometry.Image(bad).filter(o3d.geometry.ImageFilterType.Gaussian3)
        with pytest.raises(RuntimeError):
            o3d.geometry.Image(bad).create_pyramid(2)


def test_native_argument_checks():
    import ctypes as C
    from kinectpy_amd import _lib
    lib = _lib.load()
    assert lib.kpx_odometry_workspace_bytes(1, 80, 72, 3) > 0 and lib.kpx_odometry_workspace_bytes(1, 80, 72, 9) == 0
    assert lib.kpx_odometry_workspace_bytes(1, 4, 4, 4) == 0 and lib.kpx_odometry_workspace_bytes(4, 640, 576, 3) > lib.kpx_odometry_workspace_bytes(1, 640, 576, 3)
    assert lib.kpx_image_workspace_bytes(1, 80, 72) >= 80 * 72 * 4 and lib.kpx_image_workspace_bytes(0, 80, 72) == 0
    assert lib.kpx_image_filter(None, None, 1, 80, 72, 7, None, 0, None) == -1 and b"filter type" in lib.kpx_last_error()
    assert lib.kpx_image_downsample(None, None, 1, 1, 72, None) == -1
    z = C.c_double(30.0)
    assert lib.kpx_rgbd_odometry(1, None, None, None, None, 0, None, None, z, z, 80, 72, None, None, 5, 3, None, z, z, z, None, None, 0, None) == -1
    assert b"jacobian" in lib.kpx_last_error()
    assert lib.kpx_rgbd_odometry(1, None, None, None, None, 0, None, None, z, z, 80, 72, None, None, 1, 9, None, z, z, z, None, None, 0, None) == -1
    assert b"level" in lib.kpx_last_error()

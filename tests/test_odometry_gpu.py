"""GPU suite (-m gpu): the image operators and the RGB-D odometry (kpx_odometry.hip) against their NumPy restatement
tests/odometry_ref.py on the fixtures of tests/odometry_scenes.py (80 x 72 pixels, millimetres).

Bit for bit: filters, pyramids, correspondences (the decisions of AC11).  Within max(10 x spread, 1e-12): the sums of one iteration
(relative to their largest entry), the poses (absolute) and the information matrix, where `spread` is what the restatement itself shows
when it sums the correspondences in permuted orders (tests/test_odometry_cpu.py tabulates it and asserts that it cannot reach a
decision margin of the fixtures).  Bit-identical again: a batch against its single calls, and a call against its repetition.

Measured on an MI355X (device - restatement, tolerance in brackets):

    one iteration, colour, levels 0 / 1 / 2    JTJ 2.1e-15 / 6.7e-16 / 1.1e-16, JTr 1.2e-15 / 1.2e-15 / 1.6e-16 (1e-12)
                                               T 5.5e-10 (6.1e-09) / 3.7e-10 (8.0e-09) / 2.4e-11 (2.4e-09)
    one iteration, hybrid, levels 0 / 1 / 2    JTJ 1.4e-15 / 6.6e-16 / 1.9e-16, JTr 1.0e-15 / 3.8e-16 / 1.4e-16 (1e-12)
                                               T 5.0e-14 (5.0e-11) / 3.7e-13 (7.5e-12) / 7.3e-13 (1.1e-11)
    identity-hybrid-20-10-5     T 4.4e-12 (7.9e-11)   information 2.2e-15 (1e-12)
    perturbed-hybrid-20-10-5    T 7.2e-12 (9.0e-11)   information 1.9e-15
    identity-hybrid-3           T 1.9e-13 (3.1e-12)   information 1.8e-15
    perturbed-color-3           T 1.7e-09 (1.6e-08)   information 1.2e-15
    identity-hybrid-0-0-2       T 1.7e-13 (4.3e-12)   information 1.8e-15
    identity-color-0-0-2        T 9.0e-11 (1.7e-09)   information 8.1e-16
    drift check (degrees, mm; bump 2.0, 53.9 on sensor 2)   with masks (0.17, 2.1) (0.07, 3.4) (3.58, 54.1) (0.19, 11.6)
                                                            without    (0.13, 3.3) (0.10, 5.7) (4.94, 46.9) (0.09, 3.6)
"""
import numpy as np
import pytest

import odometry_ref as R
import odometry_scenes as S
from kinectpy_amd.utils import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o3d():
    from kinectpy_amd import o3d as m
    return m


@pytest.fixture(scope="module")
def ops():
    from kinectpy_amd import ops as m
    return m


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def intrinsic(o3d):
    return o3d.camera.PinholeCameraIntrinsic(S.W, S.H, *S.K4)


def mm_option(o3d, iterations=(20, 10, 5)):
    return o3d.pipelines.odometry.OdometryOption(list(iterations), **S.OPTION_MM)


def jacobian(o3d, kind):
    odo = o3d.pipelines.odometry
    return odo.RGBDOdometryJacobianFromColorTerm() if kind == R.COLOR else odo.RGBDOdometryJacobianFromHybridTerm()


def tol(spread):
    return max(10.0 * spread, 1e-12)


# ----------------------------------------------------------------- image operators
def _test_images():
    depth = R.preprocess_depth(S.images("B")[1], S.option())          # 80 x 72 with NaN where the render has no depth
    return {"80x72": depth, "75x53": S.odd_image()}


@pytest.mark.parametrize("name", ["80x72", "75x53"])
def test_image_filters_equal_restatement(o3d, name):
    img = _test_images()[name]
    assert np.isnan(img).any()
    for ft in o3d.geometry.ImageFilterType:
        got = o3d.geometry.Image(img).filter(ft)
        assert isinstance(got, o3d.geometry.Image) and same(np.asarray(got), R.image_filter(img, ft.value)), ft


@pytest.mark.parametrize("name", ["80x72", "75x53"])
@pytest.mark.parametrize("gauss", [True, False])
def test_pyramids_equal_restatement(o3d, name, gauss):
    img = _test_images()[name]
    pyr = o3d.geometry.Image(img).create_pyramid(3, gauss)
    want = R.create_pyramid(img, 3, gauss)
    assert len(pyr) == 3 and all(same(np.asarray(p), w) for p, w in zip(pyr, want))
    for ft in (o3d.geometry.ImageFilterType.Sobel3Dx, o3d.geometry.ImageFilterType.Gaussian5):
        f = o3d.geometry.Image.filter_pyramid(pyr, ft)
        assert len(f) == 3 and all(same(np.asarray(p), w) for p, w in zip(f, R.filter_pyramid(want, ft.value)))


def test_image_stack_equals_single_images(ops):
    a, b = R.preprocess_depth(S.images("A")[1], S.option()), R.preprocess_depth(S.images("B")[1], S.option())
    got = ops.image_filter(np.stack([a, b]), "gaussian7").cpu().numpy()
    assert same(got[0], R.image_filter(a, R.GAUSSIAN7)) and same(got[1], R.image_filter(b, R.GAUSSIAN7))
    down = ops.image_downsample(np.stack([a, b])).cpu().numpy()
    assert same(down[0], R.downsample(a)) and same(down[1], R.downsample(b))


# ----------------------------------------------------------------- correspondences
def test_correspondences_equal_restatement(o3d):
    odo, lv, truth = o3d.pipelines.odometry, S.levels_reference(), S.scene()["truth"]
    opt = mm_option(o3d)
    cases = [(0, np.eye(4)), (0, truth), (1, truth), (2, truth), (1, S.perturbed_init()), (2, np.eye(4))]
    for level, T in cases:
        Kl = R.level_camera(S.K4, level)
        Km = np.array([[Kl[0], 0, Kl[2]], [0, Kl[1], Kl[3]], [0, 0, 1.0]])
        got = odo.compute_correspondence(Km, T, lv[level][1], lv[level][3], opt)
        want = R.correspondence(Kl, T, lv[level][1], lv[level][3], opt.depth_diff_max)
        assert got.dtype == np.int32 and same(got, want) and len(want) > 50, (level, len(got), len(want))


def test_collision_scene_keeps_the_smallest_source_index(o3d):
    ds, dt, K, T, dmax = S.collision()
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    got = o3d.pipelines.odometry.compute_correspondence(Km, T, ds, dt, mm_option(o3d))
    want = R.correspondence(K, T, ds, dt, dmax)
    assert same(got, want) and len(want) > 1000
    assert same(got, R.correspondence_brute(K, T, ds, dt, dmax))


# ----------------------------------------------------------------- one iteration from a given pose
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("jac", [R.COLOR, R.HYBRID])
def test_one_iteration_equals_restatement(ops, jac, level):
    ref = S.iteration_reference(jac, level)
    lv, Kl = S.levels_reference()[level], R.level_camera(S.K4, level)
    g = ops.odometry_iteration(*lv, Kl, ref["init"], "color" if jac == R.COLOR else "hybrid", S.OPTION_MM["depth_diff_max"])
    dA, db = R.sums_difference(g["sums"][:21], ref["sums"][:21]), R.sums_difference(g["JTr"], ref["sums"][21:27])
    dT = float(np.abs(g["transformation"] - ref["T"]).max())
    print(f"jacobian {jac} level {level}: count {g['count']}; JTJ {dA:.2e} (tol {tol(ref['spread_JTJ']):.2e}), JTr {db:.2e} (tol {tol(ref['spread_JTr']):.2e}), "
          f"T {dT:.2e} (tol {tol(ref['spread_T']):.2e})")
    assert g["count"] == ref["count"] and g["solved"] and ref["solved"]
    assert dA <= tol(ref["spread_JTJ"]) and db <= tol(ref["spread_JTr"]) and dT <= tol(ref["spread_T"])
    assert abs(g["r2"] - ref["sums"][27]) <= tol(ref["spread_JTJ"]) * abs(ref["sums"][27])
    assert np.array_equal(g["JTJ"], g["JTJ"].T)


# ----------------------------------------------------------------- the whole chain
def _single(o3d, case):
    src, tgt, init, jac, its = S.CHAIN_CASES[case]
    s = S.scene()
    T0 = S.perturbed_init() if init == "perturbed" else np.eye(4)
    return o3d.pipelines.odometry.compute_rgbd_odometry(S.rgbd(s["depth_" + src], s["rgb_" + src]), S.rgbd(s["depth_" + tgt], s["rgb_" + tgt]),
                                                        intrinsic(o3d), T0, jacobian(o3d, jac), mm_option(o3d, its))


@pytest.mark.parametrize("case", list(S.CHAIN_CASES))
def test_chain_equals_restatement(o3d, case):
    ref = S.chain_reference(case)
    ok, T, G = _single(o3d, case)
    assert ok is ref["success"] and T.shape == (4, 4) and G.shape == (6, 6) and T.dtype == np.float64 and G.dtype == np.float64
    if not ref["success"]:
        assert np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6))
        return
    dT, dG = float(np.abs(T - ref["T"]).max()), R.sums_difference(G, ref["info"])
    print(f"{case}: T {dT:.2e} (tol {tol(ref['spread_T']):.2e}), information {dG:.2e} (tol {tol(ref['spread_info']):.2e})")
    assert dT <= tol(ref["spread_T"]) and dG <= tol(ref["spread_info"])
    Rm = T[:3, :3]
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12 and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.array_equal(G, G.T)
    ok2, T2, G2 = _single(o3d, case)                                # repeatability: bit-identical
    assert ok2 is ok and np.array_equal(T2, T) and np.array_equal(G2, G)


def test_failures_return_identities_and_leave_no_state(o3d):
    odo, s = o3d.pipelines.odometry, S.scene()
    K = intrinsic(o3d)
    good_s, good_t = S.rgbd(s["depth_A"], s["rgb_A"]), S.rgbd(s["depth_B"], s["rgb_B"])
    before = odo.compute_rgbd_odometry(good_s, good_t, K, np.eye(4), jacobian(o3d, R.HYBRID), mm_option(o3d))
    zero = np.zeros_like(s["depth_A"])
    flat_i, flat_d = np.full((S.H, S.W), 0.5, np.float32), np.full((S.H, S.W), 2000.0, np.float32)
    flat = o3d.geometry.RGBDImage(flat_i, flat_d)
    for src, tgt, jac in ((S.rgbd(zero, s["rgb_A"]), S.rgbd(zero, s["rgb_B"]), R.HYBRID), (flat, flat, R.COLOR)):
        ok, T, G = odo.compute_rgbd_odometry(src, tgt, K, np.eye(4), jacobian(o3d, jac), mm_option(o3d))
        assert ok is False and np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6))
        after = odo.compute_rgbd_odometry(good_s, good_t, K, np.eye(4), jacobian(o3d, R.HYBRID), mm_option(o3d))
        assert after[0] is True and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])


# ----------------------------------------------------------------- batch
def test_batch_is_bit_identical_to_single_calls(o3d):
    odo, s = o3d.pipelines.odometry, S.scene()
    K, opt = intrinsic(o3d), mm_option(o3d)
    pairs = [("A", "B", False), ("B", "A", False), ("A", "A", False), ("A", "P", True)]
    stack = lambda key, side: np.stack([s[key + "_" + p[side]] for p in pairs])
    n_px = S.W * S.H
    masks_t = np.stack([s["mask_P"] if p[2] else np.zeros(n_px, bool) for p in pairs]).astype(np.uint8)
    ok, T, G = odo.compute_rgbd_odometry_batch(stack("depth", 0), stack("rgb", 0), stack("depth", 1).reshape(4, S.H, S.W), stack("rgb", 1), K, None,
                                               jacobian(o3d, R.HYBRID), opt, depth_scale=1.0, depth_trunc=6000.0, masks_t=masks_t)
    assert ok.dtype == bool and ok.shape == (4,) and T.shape == (4, 4, 4) and G.shape == (4, 6, 6)
    for i, (a, b, masked) in enumerate(pairs):
        one = odo.compute_rgbd_odometry(S.rgbd(s["depth_" + a], s["rgb_" + a]), S.rgbd(s["depth_" + b], s["rgb_" + b], s["mask_P"] if masked else None), K,
                                        np.eye(4), jacobian(o3d, R.HYBRID), opt)
        assert one[0] is True and bool(ok[i]) and np.array_equal(T[i], one[1]) and np.array_equal(G[i], one[2]), (a, b)
    assert np.abs(T[2] - np.eye(4)).max() < 1e-12                   # A -> A: zero residuals
    assert not np.array_equal(T[0], T[3])                           # the mask does change the masked pair's input
    ok2, T2, G2 = odo.compute_rgbd_odometry_batch(stack("depth", 0), stack("rgb", 0), stack("depth", 1), stack("rgb", 1), K, None, jacobian(o3d, R.HYBRID),
                                                  opt, depth_scale=1.0, depth_trunc=6000.0, masks_t=masks_t)
    assert np.array_equal(ok2, ok) and np.array_equal(T2, T) and np.array_equal(G2, G)


# ----------------------------------------------------------------- drift check
def test_estimate_sensor_drift_finds_the_bumped_sensor(o3d):
    from kinectpy_amd.preprocessing.registration import estimate_sensor_drift
    xy, depth, rgb, _, _ = synth.sensor_ring(4, 2, synth.small_xy(8))
    depth, rgb = depth.copy(), rgb.copy()
    bump_deg, bump_t = 2.0, (30.0, -20.0, 40.0)
    bump_mm = float(np.linalg.norm(bump_t))
    E2 = synth.camera_pose(2, 4) @ S.rigid(bump_deg, (0.2, 1.0, -0.3), bump_t)
    d2, person2 = synth.render_depth(E2, person_shift=(5.0, 0.0, 0.0), seed=100 + 2 + 1000, xy=xy, return_person=True)
    depth[1, 2], rgb[1, 2] = d2, synth.mask_rgb(person2, seed=7 + 2)
    # the ring's colour images are the person-mask colours (background black): the mask is where they are not black; the odometry's
    # intensity comes from a painted room
    masks = (rgb != 0).any(-1)
    colors = np.stack([np.stack([S.paint(depth[f, g], E2 if (f, g) == (1, 2) else synth.camera_pose(g, 4), xy) for g in range(4)]) for f in range(2)])
    # the ring drops 10 % of its pixels at random: after the Gaussian's NaN spread 29 % of the 80 x 72 pixels are left, and a coarser
    # pyramid level has none -- the check runs at full resolution only
    opt = o3d.pipelines.odometry.OdometryOption([30], **S.OPTION_MM)
    ranks = []
    for use_masks in (True, False):
        rep = estimate_sensor_drift(depth[0], colors[0], depth[1], colors[1], intrinsic(o3d), masks[0] if use_masks else None,
                                    masks[1] if use_masks else None, opt)
        assert len(rep) == 4 and all(r["success"] for r in rep)
        print([(round(r["rotation_deg"], 3), round(r["translation"], 2)) for r in rep])
        for g, r in enumerate(rep):
            near_bump = abs(r["rotation_deg"] - bump_deg) < abs(r["rotation_deg"]) and abs(r["translation"] - bump_mm) < abs(r["translation"])
            near_zero = abs(r["rotation_deg"]) < abs(r["rotation_deg"] - bump_deg) and abs(r["translation"]) < abs(r["translation"] - bump_mm)
            assert near_bump if g == 2 else near_zero, (g, r["rotation_deg"], r["translation"])
        ranks.append((np.argsort([r["rotation_deg"] for r in rep]).tolist()[-1], np.argsort([r["translation"] for r in rep]).tolist()[-1]))
    assert ranks[0] == ranks[1] == (2, 2)

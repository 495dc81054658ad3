"""GPU suite (-m gpu): the image operators and the RGB-D odometry (kpx_odometry.hip) against their NumPy restatement
tests/odometry_ref.py on the fixtures of tests/odometry_scenes.py: 80 x 72 pixels in millimetres, and beside it 320 x 288 (360 blocks:
the last-ticket block's column loop takes a second round), crops with odd pyramid levels and levels of exactly four blocks and one
block, the same frames in metres, batches with their own poses, masks and a failing pair, and the drift check's inputs.

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
    one iteration at 320 x 288, level 0, from the perturbed pose (20501 correspondences, none in blocks 256 .. 359)
                      colour   JTJ 1.9e-15, JTr 7.0e-15 (1e-12)   T 2.1e-09 (2.6e-08)
                      hybrid   JTJ 4.7e-15, JTr 2.7e-15 (1e-12)   T 5.7e-10 (7.9e-09)
    the same from the rendered motion (68895 correspondences, 20054 of them in blocks 256 .. 359)
                      colour   JTJ 4.5e-15, JTr 4.0e-15 (1e-12)   T 1.2e-12 (1.2e-11)
                      hybrid   JTJ 2.5e-15, JTr 2.1e-15 (1e-12)   T 8.2e-14 (1.6e-12)
    320x288-hybrid-2-2-2        T 2.8e-11 (6.3e-10)   information 1.0e-14 (1e-12)
    320x288-hybrid-3            T 5.8e-10 (1.0e-08)   information 4.6e-14
    320x288-hybrid-0-0-2        T 5.8e-10 (1.0e-08)   information 4.5e-14
    320x288-color-2-2-2         T 2.9e-10 (9.4e-09)   information 4.9e-14
    320x288-color-3             T 1.9e-09 (1.9e-08)   information 5.0e-14
    320x288-color-0-0-2         T 1.8e-09 (1.8e-08)   information 1.5e-14
    75x53-hybrid-20-10-5        T 2.6e-12 (1.8e-11)   information 7.4e-16
    75x53-hybrid-4-3-2          T 3.8e-12 (1.5e-11)   information 7.2e-16
    75x53-color-3               T 5.1e-10 (2.3e-08)   information 2.9e-15
    79x71-hybrid-20-10-5        T 3.7e-12 (6.8e-11)   information 2.2e-15
    79x71-hybrid-4-3-2          T 2.6e-12 (1.9e-11)   information 2.7e-15
    79x71-color-3               T 9.0e-10 (1.9e-08)   information 7.4e-16
    65x65-hybrid-20-10-5        T 1.8e-12 (1.1e-10)   information 1.1e-15
    65x65-hybrid-4-3-2          T 4.4e-12 (6.4e-11)   information 4.1e-16
    65x65-color-3               T 2.9e-10 (1.0e-08)   information 1.5e-15
    75x53-color-4-3-2           the identities on both sides (no correspondence left on a coarse level)
    metres-hybrid-20-10-5       T 3.8e-16 (1e-12)     information 1.6e-15
    metres-trunc-hybrid-20-10-5 the identities on both sides (depth_trunc 3.5 leaves no correspondence within 0.03 m)
    metres-trunc-5.5-hybrid-20-10-5   T 1.8e-15 (1e-12)   information 1.8e-16   (the raw batch: the same figures, bit-identical to the host path)
    metres-trunc-5.5-reversed-hybrid-20-10-5   T 1.7e-15 (1e-12)   information 1.0e-14   (the raw batch likewise)
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


SMALL_SIZES = [(1, 1), (1, 2), (2, 1), (1, 7), (7, 1), (2, 2), (3, 2), (2, 3), (16, 16), (1, 255), (1, 257), (257, 1), (3, 171)]          # (H, W)


def _special_images(h, w, seed):
    """finite values, then the same with one NaN, one +inf, one -inf, and with all three at once (where the image has the room)"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-3.0, 900.0, size=(h, w)).astype(np.float32)
    n = h * w
    at = sorted({0, n // 2, n - 1})
    out = [base]
    for k, v in zip((at[0], at[-1], at[len(at) // 2]), (np.nan, np.inf, -np.inf)):
        a = base.copy()
        a.reshape(-1)[k] = v
        out.append(a)
    if n >= 16:
        a = base.copy()
        a.reshape(-1)[rng.choice(n, 6, replace=False)] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
        out.append(a)
    return out


@pytest.mark.parametrize("size", SMALL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_filters_at_small_sizes_and_block_edges(ops, size):
    """widths and heights below the tap count (both clamps act in one tap loop), pixel counts 255 / 256 / 257 / 513; NaN and both
    infinities (inf - inf and 0 x inf are NaN in the restatement and in the kernel alike); the filter by name and by its code"""
    h, w = size
    by_name = SMALL_SIZES.index(size) % 2 == 0
    for img in _special_images(h, w, 100 * h + w):
        for name, code in ops.IMAGE_FILTERS.items():
            got = ops.image_filter(img, name if by_name else code).cpu().numpy()
            assert same(got, R.image_filter(img, code)), (size, name)
    with pytest.raises(Exception, match="filter type"):
        ops.image_filter(np.zeros((h, w), np.float32), 5)


def _stack3():
    imgs = [S.odd_image(5), S.odd_image(6), S.odd_image(7)]
    imgs[1][3, 74], imgs[1][52, 0], imgs[2][0, 37], imgs[2][26, 74] = np.inf, -np.inf, -np.inf, np.inf
    return np.stack(imgs)


def test_stack_of_different_images_through_every_operator(ops):
    """the image stride times blockIdx.y: every slice of a stack of three different 75 x 53 images against its own single call and
    against the restatement"""
    st = _stack3()
    assert not same(st[0], st[1]) and not same(st[1], st[2])
    for name, code in ops.IMAGE_FILTERS.items():
        got = ops.image_filter(st, code if code % 2 else name).cpu().numpy()
        assert got.shape == st.shape
        for i in range(3):
            assert same(got[i], ops.image_filter(st[i], name).cpu().numpy()) and same(got[i], R.image_filter(st[i], code)), (name, i)
    down = ops.image_downsample(st).cpu().numpy()
    assert down.shape == (3, 26, 37)
    for i in range(3):
        assert same(down[i], ops.image_downsample(st[i]).cpu().numpy()) and same(down[i], R.downsample(st[i])), i


@pytest.mark.parametrize("size", [(2, 2), (3, 2), (5, 7), (53, 75), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramids_down_to_the_last_level(o3d, ops, size):
    """odd sizes drop a row or a column at every level; the deepest pyramid ends at a level with a side of 1 (64 x 64: seven levels,
    1 x 1), and one level more is the documented error"""
    h, w = size
    levels = int(np.log2(min(h, w))) + 1
    img = _special_images(h, w, 7 * h + w)[-1] if h * w >= 16 else _special_images(h, w, 7 * h + w)[0]
    assert same(ops.image_downsample(img).cpu().numpy(), R.downsample(img))
    for gauss in (True, False):
        pyr = o3d.geometry.Image(img).create_pyramid(levels, gauss)
        want = R.create_pyramid(img, levels, gauss)
        assert len(pyr) == levels and min(want[-1].shape) == 1 and all(same(np.asarray(p), q) for p, q in zip(pyr, want)), gauss
        with pytest.raises(RuntimeError, match="too small"):
            o3d.geometry.Image(img).create_pyramid(levels + 1, gauss)
    if size == (64, 64):
        assert levels == 7 and want[-1].shape == (1, 1)


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


@pytest.mark.parametrize("name", ["320x288", "75x53"])
def test_correspondences_beyond_one_camera(o3d, ops, name):
    """360 blocks, and levels of odd size (75 x 53, 37 x 26, 18 x 13) with their own cameras; through the wrapper and through
    ops.odometry_correspondence.  The pose is host data: no margin is involved."""
    f, lv = S.fixture(name), S.fixture_levels(name)
    odo = o3d.pipelines.odometry
    opt = odo.OdometryOption([1], **f["opt"])
    for level in range(3):
        Kl = R.level_camera(f["K4"], level)
        Km = np.array([[Kl[0], 0, Kl[2]], [0, Kl[1], Kl[3]], [0, 0, 1.0]])
        for T in (f["truth"], f["init"]):
            want = R.correspondence(Kl, T, lv[level][1], lv[level][3], opt.depth_diff_max)
            got = odo.compute_correspondence(Km, T, lv[level][1], lv[level][3], opt)
            direct = ops.odometry_correspondence(lv[level][1], lv[level][3], Kl, T, opt.depth_diff_max).cpu().numpy()
            assert got.dtype == np.int32 and same(got, want) and same(direct, want) and len(want) > 20, (level, len(got), len(want))


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


@pytest.mark.parametrize("pose", ["init", "truth"])
@pytest.mark.parametrize("jac", [R.COLOR, R.HYBRID])
def test_one_iteration_with_two_slab_columns_per_thread(ops, jac, pose):
    """level 0 of the 320 x 288 pair: 360 blocks, so threads 0 .. 103 of the last-ticket block add two columns of the slab each.  From
    the perturbed pose the columns of the second round are all zero (the correspondences lie on the far wall, in the upper blocks);
    from the rendered motion the floor corresponds too, and every block beyond 255 carries sums."""
    f = S.fixture("320x288")
    assert -(-f["W"] * f["H"] // 256) > 256                        # the shape cannot silently shrink below the second round of the loop
    ref = S.fixture_iteration_reference("320x288", jac, 0, pose)
    if pose == "truth":
        c = ref["correspondences"]
        assert len(np.unique((c[:, 3].astype(np.int64) * f["W"] + c[:, 2])[c[:, 3] * f["W"] + c[:, 2] >= 65536] // 256)) == 360 - 256
    g = ops.odometry_iteration(*S.fixture_levels("320x288")[0], f["K4"], ref["init"], "color" if jac == R.COLOR else "hybrid", f["opt"]["depth_diff_max"])
    dA, db = R.sums_difference(g["sums"][:21], ref["sums"][:21]), R.sums_difference(g["JTr"], ref["sums"][21:27])
    dT = float(np.abs(g["transformation"] - ref["T"]).max())
    print(f"320x288 jacobian {jac} level 0 from {pose}: count {g['count']}; JTJ {dA:.2e} (tol {tol(ref['spread_JTJ']):.2e}), "
          f"JTr {db:.2e} (tol {tol(ref['spread_JTr']):.2e}), T {dT:.2e} (tol {tol(ref['spread_T']):.2e})")
    assert g["count"] == ref["count"] and g["count"] > 10000 and g["solved"] and ref["solved"]
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


def _compare_chain(case, ref, run):
    ok, T, G = run()
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
    ok2, T2, G2 = run()                                             # repeatability: bit-identical
    assert ok2 is ok and np.array_equal(T2, T) and np.array_equal(G2, G)


@pytest.mark.parametrize("case", list(S.CHAIN_CASES))
def test_chain_equals_restatement(o3d, case):
    _compare_chain(case, S.chain_reference(case), lambda: _single(o3d, case))


def _fixture_call(o3d, name, jac, iterations, init=None):
    """compute_rgbd_odometry on a fixture of S.FIXTURES (float32 intensity and depth), from its perturbed pose unless another is given"""
    f = S.fixture(name)
    odo = o3d.pipelines.odometry
    return odo.compute_rgbd_odometry(o3d.geometry.RGBDImage(f["Is"], f["Ds"]), o3d.geometry.RGBDImage(f["It"], f["Dt"]),
                                     o3d.camera.PinholeCameraIntrinsic(f["W"], f["H"], *f["K4"]), f["init"] if init is None else init,
                                     jacobian(o3d, jac), odo.OdometryOption(list(iterations), **f["opt"]))


@pytest.mark.parametrize("case", list(S.NEW_CHAIN_CASES))
def test_chain_equals_restatement_beyond_one_camera(o3d, case):
    """320 x 288 (slab columns beyond one per thread), crops with odd levels and levels of exactly four blocks and one block, metres
    (Open3D's own units), a truncated metre pair; the cases of S.NEW_FAILURES return the identities"""
    name, jac, its = S.NEW_CHAIN_CASES[case]
    ref = S.new_chain_reference(case)
    assert ref["success"] is (case not in S.NEW_FAILURES)
    _compare_chain(case, ref, lambda: _fixture_call(o3d, name, jac, its))


def test_levels_without_iterations_change_nothing(o3d):
    """seven levels, 80 x 72 down to 1 x 1, with iterations on the finest only: bit for bit the one-level call.  One iteration on the
    1 x 1 level has no correspondence: the identities, and the next good call is unchanged."""
    odo, s = o3d.pipelines.odometry, S.scene()
    K, T0, jac = intrinsic(o3d), S.perturbed_init(), jacobian(o3d, R.HYBRID)
    src, tgt = S.rgbd(s["depth_A"], s["rgb_A"]), S.rgbd(s["depth_B"], s["rgb_B"])
    one = odo.compute_rgbd_odometry(src, tgt, K, T0, jac, mm_option(o3d, (2,)))
    seven = odo.compute_rgbd_odometry(src, tgt, K, T0, jac, mm_option(o3d, (0, 0, 0, 0, 0, 0, 2)))
    assert one[0] is True and seven[0] is True and np.array_equal(seven[1], one[1]) and np.array_equal(seven[2], one[2])
    assert not np.array_equal(one[1], T0)
    ok, T, G = odo.compute_rgbd_odometry(src, tgt, K, T0, jac, mm_option(o3d, (1, 0, 0, 0, 0, 0, 0)))
    assert ok is False and np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6))
    again = odo.compute_rgbd_odometry(src, tgt, K, T0, jac, mm_option(o3d, (2,)))
    assert again[0] is True and np.array_equal(again[1], one[1]) and np.array_equal(again[2], one[2])


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


def _own_pose():
    return S.rigid(0.4, (0.0, 1.0, 0.3), (-8.0, 5.0, 10.0))


def test_batch_with_its_own_poses_masks_and_a_failing_pair(o3d, ops):
    """six raw pairs, their own initial poses (pose + 16 pair), a source mask on pair 3, a target mask on pair 4, and two failures beside
    which the neighbours notice nothing: pair 2 has no source depth at all; pair 5 (S.holed_depth_A) has no correspondence on the
    coarsest level, fails there in the first iteration, and has hundreds on the finer levels that run afterwards with its flag set"""
    odo, s = o3d.pipelines.odometry, S.scene()
    K, opt, jac = intrinsic(o3d), mm_option(o3d), jacobian(o3d, R.HYBRID)
    n_px = S.W * S.H
    pairs = [("A", "B"), ("A", "B"), ("A", "B"), ("P", "A"), ("A", "P"), ("A", "B")]
    inits = np.stack([np.eye(4), S.perturbed_init(), s["truth"], np.linalg.inv(S.perturbed_init()), _own_pose(), S.perturbed_init()])
    depth_s, depth_t = (np.stack([s["depth_" + p[side]] for p in pairs]) for side in (0, 1))
    rgb_s, rgb_t = (np.stack([s["rgb_" + p[side]] for p in pairs]) for side in (0, 1))
    masks_s, masks_t = np.zeros((6, n_px), np.uint8), np.zeros((6, n_px), bool)
    masks_s[3], masks_t[4] = 255 * s["mask_P"], s["mask_P"]
    assert s["mask_P"].sum() > 50
    depth_s[5] = S.holed_depth_A()
    holed = depth_s.copy()
    holed[2] = 0
    kw = dict(depth_scale=1.0, depth_trunc=6000.0, masks_s=masks_s, masks_t=masks_t)
    ok, T, G = odo.compute_rgbd_odometry_batch(holed, rgb_s, depth_t, rgb_t, K, inits, jac, opt, **kw)
    assert ok.tolist() == [True, True, False, True, True, False]
    for i in (2, 5):
        assert np.array_equal(T[i], np.eye(4)) and np.array_equal(G[i], np.eye(6)), i
    lone = odo.compute_rgbd_odometry(S.rgbd(depth_s[5], s["rgb_A"]), S.rgbd(s["depth_B"], s["rgb_B"]), K, inits[5], jac, opt)
    assert lone[0] is False and np.array_equal(lone[1], np.eye(4)) and np.array_equal(lone[2], np.eye(6))

    def single(i, masked=True):
        a, b = pairs[i]
        return odo.compute_rgbd_odometry(S.rgbd(s["depth_" + a], s["rgb_" + a], s["mask_P"] if masked and i == 3 else None),
                                         S.rgbd(s["depth_" + b], s["rgb_" + b], s["mask_P"] if masked and i == 4 else None), K, inits[i], jac, opt)

    for i in (0, 1, 3, 4):
        one = single(i)
        assert one[0] is True and np.array_equal(T[i], one[1]) and np.array_equal(G[i], one[2]), i
    assert not np.array_equal(T[0], T[1])                           # the same frames from two poses: every pair starts from its own
    for i in (3, 4):                                                # and the masks do change what those pairs see
        bare = single(i, masked=False)
        assert not (np.array_equal(T[i], bare[1]) and np.array_equal(G[i], bare[2])), i
    # the entry point below the wrapper, with its correspondence counts: none for a failed pair, whatever its last launch found
    ok_o, T_o, G_o, n_o = ops.rgbd_odometry(holed, rgb_s, depth_t, rgb_t, S.W, S.H, S.K4, inits, "hybrid", (20, 10, 5), raw=True, depth_scale=1.0,
                                            depth_trunc=6000.0, mask_s=masks_s, mask_t=masks_t, **S.OPTION_MM)
    assert np.array_equal(ok_o, ok) and np.array_equal(T_o, T) and np.array_equal(G_o, G)
    assert n_o.dtype == np.int64 and n_o[2] == 0 and n_o[5] == 0 and all(n_o[i] > 500 for i in (0, 1, 3, 4))
    # pair 2's depth restored: it succeeds like its own call, and the other four are bit-identical to what they were beside the failure
    ok2, T2, G2 = odo.compute_rgbd_odometry_batch(depth_s, rgb_s, depth_t, rgb_t, K, inits, jac, opt, **kw)
    one = single(2)
    assert ok2.tolist() == [True] * 5 + [False] and one[0] is True and np.array_equal(T2[2], one[1]) and np.array_equal(G2[2], one[2])
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(T2[keep], T[keep]) and np.array_equal(G2[keep], G[keep])


def test_batch_of_two_pairs_at_320x288(o3d):
    """many blocks times several pairs through the ticket: every pair has its own ticket, count and slab"""
    odo, s = o3d.pipelines.odometry, S.scene_at(2)
    w, h = s["W"], s["H"]
    K, opt, jac = o3d.camera.PinholeCameraIntrinsic(w, h, *s["K4"]), mm_option(o3d, (2, 2, 2)), jacobian(o3d, R.HYBRID)
    pairs = [("A", "B"), ("B", "A")]
    inits = np.stack([S.perturbed_init(), np.linalg.inv(S.perturbed_init())])
    stack = lambda key, side: np.stack([s[key + "_" + p[side]] for p in pairs])
    ok, T, G = odo.compute_rgbd_odometry_batch(stack("depth", 0), stack("rgb", 0), stack("depth", 1), stack("rgb", 1), K, inits, jac, opt,
                                               depth_scale=1.0, depth_trunc=6000.0)
    for i, (a, b) in enumerate(pairs):
        one = odo.compute_rgbd_odometry(S.rgbd_at(s["depth_" + a], s["rgb_" + a], w, h), S.rgbd_at(s["depth_" + b], s["rgb_" + b], w, h), K, inits[i], jac, opt)
        assert one[0] is True and bool(ok[i]) and np.array_equal(T[i], one[1]) and np.array_equal(G[i], one[2]), (a, b)
    assert not np.array_equal(T[0], T[1])


@pytest.mark.parametrize("name", ["metres-trunc", "metres-trunc-5.5", "metres-trunc-5.5-reversed"])
def test_raw_conversion_in_metres_with_a_truncation_that_bites(o3d, name):
    """uint16 millimetre frames, depth_scale 1000, a depth_trunc that takes pixels away, Open3D's kind of option: the conversion in the
    kernel is the host's, bit for bit, and the chain is the restatement's on the host images.  depth_trunc 3.5 leaves this pair no
    correspondence within 0.03 m (S.fixture): all three fail alike; 5.5 cuts part of the far wall of B, the target -- or, reversed,
    the source -- and succeeds."""
    odo, s, f, whole = o3d.pipelines.odometry, S.scene(), S.fixture(name), S.fixture("metres")
    trunc, case = S.TRUNC_M[name], name + "-hybrid-20-10-5"
    K, opt, jac = intrinsic(o3d), odo.OdometryOption([20, 10, 5], **f["opt"]), jacobian(o3d, R.HYBRID)
    a, b = f["frames"]
    host = [o3d.geometry.RGBDImage.create_from_color_and_depth(s["rgb_" + n].reshape(S.H, S.W, 3), s["depth_" + n].reshape(S.H, S.W), 1000.0, trunc) for n in (a, b)]
    assert same(np.asarray(host[0].depth), f["Ds"]) and same(np.asarray(host[1].depth), f["Dt"])
    bitten = host[0] if a == "B" else host[1]                       # zeros it did not have at 6.0, in B at the least
    assert ((np.asarray(bitten.depth) == 0) & (whole["Dt"] > 0)).sum() > 500
    raw = (s["depth_" + a][None], s["rgb_" + a][None], s["depth_" + b][None], s["rgb_" + b][None])
    ok, T, G = odo.compute_rgbd_odometry_batch(*raw, K, f["init"][None], jac, opt, depth_scale=1000.0, depth_trunc=trunc)
    one = odo.compute_rgbd_odometry(host[0], host[1], K, f["init"], jac, opt)
    assert bool(ok[0]) is one[0] and np.array_equal(T[0], one[1]) and np.array_equal(G[0], one[2])
    ref = S.new_chain_reference(case)
    assert ref["success"] is (case not in S.NEW_FAILURES)
    _compare_chain(case + " (raw)", ref, lambda: (bool(ok[0]), T[0], G[0]))
    if ref["success"]:                                              # and without the truncation the result is another
        far = odo.compute_rgbd_odometry_batch(*raw, K, f["init"][None], jac, opt, depth_scale=1000.0, depth_trunc=6.0)
        assert bool(far[0][0]) and not np.array_equal(far[1][0], T[0])


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


def _same_report(a, b):
    return len(a) == len(b) and all(x["success"] is y["success"] and np.array_equal(x["transformation"], y["transformation"])
                                    and np.array_equal(x["information"], y["information"]) and x["rotation_deg"] == y["rotation_deg"]
                                    and x["translation"] == y["translation"] for x, y in zip(a, b))


def test_estimate_sensor_drift_takes_xyz_triples(o3d, tmp_path):
    """int16 XYZ triples (S, n_px, 3), as the pipeline holds its frames: the z column, a negative z clipped to "no measurement" """
    from kinectpy_amd.preprocessing.registration import estimate_sensor_drift
    _, _, depths, colors, masks = S.drift_directory(tmp_path)
    opt = mm_option(o3d, (4, 3, 2))
    z = depths.copy()
    at = np.flatnonzero(z[1, 1] > 0)[::211]                        # holes in a frame's z plane ...
    z[1, 1, at] = 0
    xyz = np.stack([np.full(depths.shape, 11, np.int16), np.full(depths.shape, -7, np.int16), depths.astype(np.int16)], -1)
    xyz[1, 1, at, 2] = -np.arange(1, len(at) + 1)                  # ... which the triples carry as negative z
    assert len(at) > 20 and xyz.shape == (2, 2, S.W * S.H, 3) and (xyz[..., 2] < 0).sum() == len(at)
    for m0, m1 in ((None, None), (masks[0], masks[1])):
        plane = estimate_sensor_drift(z[0], colors[0], z[1], colors[1], intrinsic(o3d), m0, m1, opt)
        triples = estimate_sensor_drift(xyz[0], colors[0], xyz[1], colors[1], intrinsic(o3d), m0, m1, opt)
        assert len(plane) == 2 and all(r["success"] for r in plane) and _same_report(triples, plane)
        whole = estimate_sensor_drift(depths[0], colors[0], depths[1], colors[1], intrinsic(o3d), m0, m1, opt)
        assert _same_report(whole[:1], plane[:1]) and not _same_report(whole[1:], plane[1:])          # the holes are seen, on their sensor only


def test_data_processor_drift_check(o3d, tmp_path, caplog):
    """DataProcessor's periodic check on a two-device, two-frame directory: frame set 0 is the reference, frame set 1 is compared with
    it through estimate_sensor_drift on the files' frames and mask_fn's masks"""
    from kinectpy_amd.preprocessing.data import DataProcessor
    from kinectpy_amd.preprocessing.registration import estimate_sensor_drift
    dirs, mask_fn, depths, colors, masks = S.drift_directory(tmp_path)
    opt = mm_option(o3d, (4, 3, 2))
    dp = DataProcessor(dirs, None, None, run=False, mask_fn=mask_fn, drift_check_every=1, drift_intrinsic=intrinsic(o3d), drift_option=opt)
    with caplog.at_level("INFO"):
        assert dp._drift_check(0) is None
        assert dp.drift_log == [] and not any("drift check" in r.getMessage() for r in caplog.records)
        report = dp._drift_check(1)
    assert len(dp.drift_log) == 1 and dp.drift_log[0][0] == 1 and dp.drift_log[0][1] is report
    assert sum("drift check, frame 1, device" in r.getMessage() for r in caplog.records) == 2
    direct = estimate_sensor_drift(depths[0], colors[0], depths[1], colors[1], intrinsic(o3d), masks[0], masks[1], opt)
    assert len(report) == 2 and all(r["success"] for r in report) and _same_report(report, direct)
    unmasked = estimate_sensor_drift(depths[0], colors[0], depths[1], colors[1], intrinsic(o3d), None, None, opt)
    assert not _same_report(report[:1], unmasked[:1]) and _same_report(report[1:], unmasked[1:])          # mask_fn's person mask is used

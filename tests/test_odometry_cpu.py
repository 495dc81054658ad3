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

The fixtures beyond that camera (S.fixture: 320 x 288 at K = (252, 252, 160, 144), top-left crops of the 80 x 72 images, the same frames
in metres with option (0.03, 0, 6.0); all from the perturbed pose).  "x bound": the margin over ten times the spread carried to a
projection and a z' through S.bound_constants -- at least 10 is asserted; the smallest is 12.4, the rounding margin of 320x288-color-3:

    case                                      success  spread R   spread t   spread info  rounding margin (x bound)  depth margin (x bound)
    320x288-hybrid-2-2-2                      yes      9.1e-16    6.3e-11    6.2e-15      1.0e-06 (1.64e+03)    2.0e-03 (2.54e+06)
    320x288-hybrid-3                          yes      8.5e-16    1.0e-09    2.9e-14      2.7e-06 (266)         6.9e-05 (6.79e+03)
    320x288-hybrid-0-0-2                      yes      8.8e-16    1.0e-09    2.8e-14      2.7e-06 (266)         6.9e-05 (6.79e+03)
    320x288-color-2-2-2                       yes      1.8e-13    9.4e-10    2.0e-14      5.7e-07 (53)          2.6e-04 (6.46e+03)
    320x288-color-3                           yes      3.4e-13    1.9e-09    2.9e-14      2.7e-07 (12.4)        6.5e-04 (8.15e+03)
    320x288-color-0-0-2                       yes      3.1e-13    1.7e-09    1.1e-14      6.0e-07 (30.1)        6.5e-04 (8.77e+03)
    75x53-hybrid-20-10-5                      yes      2.6e-15    1.8e-12    1.9e-15      4.5e-06 (4.64e+05)    9.8e-04 (2.01e+06)
    75x53-hybrid-4-3-2                        yes      2.5e-15    1.5e-12    1.8e-15      3.6e-05 (4.15e+06)    6.5e-03 (1.4e+07)
    75x53-color-3                             yes      4.1e-13    2.3e-09    1.4e-15      2.1e-06 (327)         6.5e-03 (6.72e+04)
    79x71-hybrid-20-10-5                      yes      1.9e-15    6.8e-12    4.6e-15      1.7e-06 (8.3e+04)     3.2e-03 (7.93e+06)
    79x71-hybrid-4-3-2                        yes      1.4e-15    1.9e-12    3.0e-15      2.6e-06 (3.43e+05)    6.5e-03 (2.41e+07)
    79x71-color-3                             yes      3.4e-13    1.9e-09    3.7e-16      6.4e-06 (1.17e+03)    6.5e-03 (8.09e+04)
    65x65-hybrid-20-10-5                      yes      2.6e-15    1.0e-11    1.5e-15      5.0e-06 (1.6e+05)     6.5e-03 (1.15e+07)
    65x65-hybrid-4-3-2                        yes      2.2e-15    6.4e-12    2.8e-15      4.9e-07 (2.41e+04)    4.3e-03 (9.4e+06)
    65x65-color-3                             yes      1.9e-13    1.0e-09    5.5e-16      4.3e-05 (1.48e+04)    1.6e-03 (3.78e+04)
    metres-hybrid-20-10-5                     yes      4.3e-16    1.2e-15    4.6e-15      5.5e-08 (1.43e+04)    1.8e-06 (2.08e+07)
    metres-trunc-5.5-hybrid-20-10-5           yes      3.6e-15    6.2e-15    1.1e-15      5.5e-07 (2.42e+04)    3.1e-06 (4.3e+06)
    metres-trunc-5.5-reversed-hybrid-20-10-5  yes      5.9e-16    3.1e-15    7.4e-15      6.7e-06 (7.51e+05)    3.2e-08 (2.38e+05)
    75x53-color-4-3-2                         no (no correspondence left on a coarse level)
    metres-trunc-hybrid-20-10-5               no (depth_trunc 3.5 takes the walls away, and nothing else of this pair corresponds within 0.03 m)

    one iteration at 320 x 288, level 0 (jacobian): correspondences (in blocks 256 .. 359), spread of JTJ, JTr (relative), of the new pose
    from the perturbed pose     colour / hybrid    20501 (0)        4.9e-15 / 6.3e-15    1.1e-14 / 4.6e-15    2.6e-09 / 7.9e-10
    from the rendered motion    colour / hybrid    68895 (20054)    1.4e-14 / 6.6e-15    3.0e-15 / 1.3e-14    1.2e-12 / 1.6e-13

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


# ----------------------------------------------------------------- the fixtures beyond one 80 x 72 millimetre camera
def test_new_fixture_shapes():
    """what the fixtures are for: 320 x 288 is more than 256 blocks of 256 pixels (two slab columns in some threads of the last-ticket
    block), the crops have levels of odd size, of exactly four blocks and of one block, and the metre frames are the millimetre ones"""
    f = S.fixture("320x288")
    assert (f["W"], f["H"]) == (320, 288) and -(-f["W"] * f["H"] // 256) == 360 and f["K4"] == (252.0, 252.0, 160.0, 144.0)
    assert [lv[0].shape for lv in S.fixture_levels("320x288")] == [(288, 320), (144, 160), (72, 80)]
    assert [lv[0].shape for lv in S.fixture_levels("75x53")] == [(53, 75), (26, 37), (13, 18)]
    assert [lv[0].shape for lv in S.fixture_levels("79x71")] == [(71, 79), (35, 39), (17, 19)]
    assert [lv[0].size for lv in S.fixture_levels("65x65")] == [65 * 65, 4 * 256, 256]
    m, mm = S.fixture("metres"), S.images("A")
    assert np.array_equal(m["Is"], mm[0]) and np.array_equal(m["Ds"], mm[1] / np.float32(1000.0)) and m["Ds"].max() == 5.5
    for name, n_s, n_t in (("metres-trunc", 3476, 3473), ("metres-trunc-5.5", 0, 850), ("metres-trunc-5.5-reversed", 850, 0)):          # the truncation bites: pixels it takes away
        cut = S.fixture(name)
        assert max(cut["Ds"].max(), cut["Dt"].max()) <= S.TRUNC_M[name] and (cut["Ds"] > 0).sum() > 1000
        ws, wt = (m["Dt"], m["Ds"]) if cut["frames"] == "BA" else (m["Ds"], m["Dt"])
        assert (((cut["Ds"] == 0) & (ws > 0)).sum(), ((cut["Dt"] == 0) & (wt > 0)).sum()) == (n_s, n_t)
    for name in S.FIXTURES:
        f = S.fixture(name)
        assert all(f[k].shape == (f["H"], f["W"]) and f[k].dtype == np.float32 for k in ("Is", "Ds", "It", "Dt"))


def test_crop_correspondences_equal_brute_force():
    f, lv = S.fixture("75x53"), S.fixture_levels("75x53")
    for level in range(3):
        for T in (f["truth"], f["init"]):
            Kl = R.level_camera(f["K4"], level)
            got = R.correspondence(Kl, T, lv[level][1], lv[level][3], 30.0)
            assert np.array_equal(got, R.correspondence_brute(Kl, T, lv[level][1], lv[level][3], 30.0)) and len(got) > 20, (level, len(got))


@pytest.mark.parametrize("case", list(S.NEW_CHAIN_CASES))
def test_margins_of_the_new_fixtures(case):
    """the success flag of every new case, and the relation of test_summation_order_spread with a further factor of ten.  "No decision
    within 1e-6 of a boundary" cannot hold at 92 160 pixels (millions of projected coordinates are drawn over a chain, and the metre
    scene's z' are 1e-3 as large); what the GPU comparison needs is that ten times the spread, carried through S.bound_constants to a
    projection and a z', stays below a tenth of the margin."""
    name = S.NEW_CHAIN_CASES[case][0]
    r, (rot_px, t_px, rot_z, t_z) = S.new_chain_reference(case), S.bound_constants(name)
    m = r["margins"]
    assert r["success"] is (case not in S.NEW_FAILURES)
    if not r["success"]:
        assert np.array_equal(r["T"], np.eye(4)) and np.array_equal(r["info"], np.eye(6))
        return
    b_px, b_z = 10.0 * (rot_px * r["spread_R"] + t_px * r["spread_t"]), 10.0 * (rot_z * r["spread_R"] + t_z * r["spread_t"])
    print(f"{case:24s} spread R {r['spread_R']:.2e} t {r['spread_t']:.2e} info {r['spread_info']:.2e}; rounding margin {m.rounding:.2e} px = "
          f"{m.rounding / b_px:.3g} x bound, depth margin {m.depth_diff:.2e} = {m.depth_diff / b_z:.3g} x bound")
    assert 10.0 * b_px < m.rounding and 10.0 * b_z < m.depth_diff
    assert r["spread_info"] < 1e-13
    Rm = r["T"][:3, :3]
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12 and np.array_equal(r["info"], r["info"].T)


def test_new_iteration_cases():
    """one iteration at level 0 of the 320 x 288 pair from given poses (host data: no margin is involved).  From the perturbed pose
    every correspondence lies on the far wall, in the upper part of the image: blocks 256 .. 359 hold none, and the second round of
    the column loop would add zeros.  From the rendered motion the floor corresponds as well: every one of those blocks holds some."""
    for pose, beyond in (("init", 0), ("truth", 104)):
        for jac in (R.COLOR, R.HYBRID):
            r = S.fixture_iteration_reference("320x288", jac, 0, pose)
            c = r["correspondences"]
            blocks = np.unique((c[:, 3].astype(np.int64) * 320 + c[:, 2]) // 256)
            print(f"320x288 ({jac}, 0) from {pose}: count {r['count']}, blocks beyond 255 with correspondences {(blocks >= 256).sum()}; "
                  f"spread JTJ {r['spread_JTJ']:.2e}  JTr {r['spread_JTr']:.2e}  T {r['spread_T']:.2e}")
            assert r["solved"] and r["count"] == len(c) > 10000 and r["spread_JTJ"] < 1e-13 and (blocks >= 256).sum() == beyond


def test_metre_scene_moves_towards_the_rendered_motion():
    """Open3D's own units: metres-hybrid-20-10-5 ends 0.31 degrees / 0.028 m from the rendered motion, where the millimetre chain ends"""
    f, r = S.fixture("metres"), S.new_chain_reference("metres-hybrid-20-10-5")
    e0, e1 = S.pose_error(f["init"], f["truth"]), S.pose_error(r["T"], f["truth"])
    print(f"start {e0[0]:.3f} deg {e0[1]:.4f} m -> final {e1[0]:.3f} deg {e1[1]:.4f} m")
    assert r["success"] and e1[0] < e0[0] and e1[1] < e0[1] and e1[1] < 0.05


def test_levels_without_iterations_change_nothing():
    """iterations (0, 0, 0, 0, 0, 0, 2) over seven levels (80 x 72 down to 1 x 1) is (2,) over one level, bit for bit: the coarse levels
    are built and never used.  One iteration on the 1 x 1 level has no correspondence, and neither has a source without depth."""
    (Is, Ds), (It, Dt) = S.images("A"), S.images("B")
    T0 = S.perturbed_init()
    assert [lv[0].shape for lv in R.prepare(Is, Ds, It, Dt, S.K4, T0, S.option((0,) * 7))][-1] == (1, 1)
    a = R.odometry(Is, Ds, It, Dt, S.K4, T0, R.HYBRID, S.option((0, 0, 0, 0, 0, 0, 2)))
    b = R.odometry(Is, Ds, It, Dt, S.K4, T0, R.HYBRID, S.option((2,)))
    assert a[0] and b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and not np.array_equal(a[1], T0)
    ok, T, G = R.odometry(Is, Ds, It, Dt, S.K4, T0, R.HYBRID, S.option((1, 0, 0, 0, 0, 0, 0)))
    assert not ok and np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6))
    ok, T, G = R.odometry(Is, np.zeros_like(Ds), It, Dt, S.K4, T0, R.HYBRID, S.option())
    assert not ok and np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6))


def test_holed_source_fails_on_the_coarsest_level_only():
    """the batch test's mid-chain failure: S.holed_depth_A() -> B from the perturbed pose has no correspondence on the 20 x 18 level,
    where the chain begins and fails, and has some on the two finer levels at that very pose"""
    s = S.scene()
    im = S.rgbd(S.holed_depth_A(), s["rgb_A"])
    Is, Ds, (It, Dt), T0 = np.asarray(im.color), np.asarray(im.depth), S.images("B"), S.perturbed_init()
    lv = R.prepare(Is, Ds, It, Dt, S.K4, T0, S.option())
    n = [len(R.correspondence(R.level_camera(S.K4, l), T0, lv[l][1], lv[l][3], 30.0)) for l in range(3)]
    assert n == [335, 29, 0]
    ok, T, G = R.odometry(Is, Ds, It, Dt, S.K4, T0, R.HYBRID, S.option())
    assert not ok and np.array_equal(T, np.eye(4)) and np.array_equal(G, np.eye(6))
    assert R.odometry(Is, Ds, It, Dt, S.K4, T0, R.HYBRID, S.option((5,)))[0]          # one level: the same pair succeeds


# ----------------------------------------------------------------- the drift check's frames (no device: files in, arrays out)
def test_data_processor_drift_frames(tmp_path, caplog):
    from kinectpy_amd import o3d
    from kinectpy_amd.preprocessing.data import DataProcessor
    dirs, mask_fn, depths, colors, masks = S.drift_directory(tmp_path)
    K = o3d.camera.PinholeCameraIntrinsic(S.W, S.H, *S.K4)
    with pytest.raises(RuntimeError):
        DataProcessor(dirs, None, None, run=False, drift_check_every=1)                # needs the intrinsic
    with pytest.raises(RuntimeError):
        DataProcessor(dirs, None, None, run=False, drift_check_every=0, drift_intrinsic=K)
    dp = DataProcessor(dirs, None, None, run=False, mask_fn=mask_fn, drift_check_every=1, drift_intrinsic=K)
    assert dp.number_of_devices == 2 and dp.drift_log == []
    for f in range(2):
        d, c, m = dp._drift_frames(f)
        assert d.dtype == np.int16 and d.shape == (2, S.W * S.H, 3) and np.array_equal(d[:, :, 2], depths[f].astype(np.int16))
        assert c.dtype == np.uint8 and np.array_equal(c, colors[f])
        assert m.dtype == bool and np.array_equal(m, masks[f])
    assert masks[1, 0].sum() > 50 and not masks[0].any()
    with caplog.at_level("INFO"):
        assert dp._drift_check(0) is None                            # frame set 0 is the reference: nothing to compare, nothing logged
    assert dp.drift_log == [] and not any("drift check" in r.getMessage() for r in caplog.records)
    assert DataProcessor(dirs, None, None, run=False, drift_check_every=1, drift_intrinsic=K)._drift_frames(1)[2] is None


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

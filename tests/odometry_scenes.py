"""Fixtures of the odometry suites (tests/test_odometry_cpu.py, tests/test_odometry_gpu.py): all on the 80 x 72 camera synth.small_xy(8),
K = (63, 63, 40, 36), millimetres.

  A / B      the empty room (the person moved out of sight) rendered noise-free from synth.camera_pose(0, 4) and from that pose composed
             with MOTION: 1.5 degrees about (0.3, 1, 0.2) and t = (25, -13, 29) mm (40.4 mm) -- chosen among its neighbours as one for which
             every chain case below keeps the decision margins tests/test_odometry_cpu.py asserts
  intensity  one smooth scalar field of the WORLD position per colour channel, evaluated at each pixel's unprojected point and
             quantised to uint8 (pixels without depth are black)
  person     pose B again with the person standing in the room, and the mask of the pixels that see it
  odd        a 75 x 53 float image with NaN holes for the image operators
  collision  a fronto-parallel wall at 2000 mm seen again from 600 mm further back: up to two source pixels land on one target pixel
             with exactly equal z'
"""
import functools

import numpy as np

from kinectpy_amd.geometry import RGBDImage
from kinectpy_amd.utils import synth

import odometry_ref as R

W, H = 80, 72
K4 = (63.0, 63.0, 40.0, 36.0)
OPTION_MM = dict(depth_diff_max=30.0, depth_min=0.0, depth_max=6000.0)
AWAY = (0.0, 1e6, 0.0)
MOTION_DEG, MOTION_AXIS, MOTION_T = 1.5, (0.3, 1.0, 0.2), (25.0, -13.0, 29.0)


def rigid(deg, axis, t):
    ax = np.asarray(axis, dtype=np.float64)
    ax = ax / np.linalg.norm(ax)
    a = np.deg2rad(deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    T[:3, 3] = t
    return T


def rotation_deg(T):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(T)[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))


def pose_error(T, truth):
    """(degrees, data units) between two rigid transforms"""
    D = np.asarray(T) @ np.linalg.inv(truth)
    return rotation_deg(D), float(np.linalg.norm(D[:3, 3]))


def paint(depth, E, xy):
    """uint8 (n_px, 3): the colour field at the world points of a rendered depth image (camera -> world E)"""
    z = depth.astype(np.float64)
    p = np.stack([np.nan_to_num(xy[:, 0]) * z, np.nan_to_num(xy[:, 1]) * z, z], 1) @ E[:3, :3].T + E[:3, 3]
    f = np.stack([0.5 + 0.22 * np.sin(p[:, 0] / 310.0) * np.cos(p[:, 1] / 270.0) + 0.2 * np.cos(p[:, 2] / 350.0 + p[:, 0] / 420.0),
                  0.5 + 0.3 * np.cos(p[:, 2] / 290.0 + p[:, 1] / 380.0) + 0.1 * np.sin(p[:, 0] / 200.0),
                  0.5 + 0.3 * np.sin(p[:, 1] / 240.0 + p[:, 0] / 330.0)], 1)
    rgb = np.clip(np.rint(255.0 * f), 0, 255).astype(np.uint8)
    rgb[depth == 0] = 0
    return rgb


@functools.lru_cache(maxsize=None)
def scene():
    """dict: xy, poses A / B, truth (source A -> target B), raw frames depth_* uint16 (n_px,), rgb_* uint8 (n_px, 3), mask_P bool"""
    xy = synth.small_xy(8)
    A = synth.camera_pose(0, 4)
    B = A @ rigid(MOTION_DEG, MOTION_AXIS, MOTION_T)
    s = {"xy": xy, "A": A, "B": B, "truth": np.linalg.inv(B) @ A}
    for name, E in (("A", A), ("B", B)):
        s["depth_" + name] = synth.render_depth(E=E, xy=xy, noise=0, drop=0, person_shift=AWAY)
        s["rgb_" + name] = paint(s["depth_" + name], E, xy)
    s["depth_P"], s["mask_P"] = synth.render_depth(E=B, xy=xy, noise=0, drop=0, return_person=True)
    s["rgb_P"] = paint(s["depth_P"], B, xy)
    return s


def rgbd(depth, rgb, mask=None):
    """the host path from raw frames to the odometry's input: RGBDImage with float32 intensity and float32 depth (millimetres)"""
    d = depth.reshape(H, W).copy()
    if mask is not None:
        d[mask.reshape(H, W) != 0] = 0
    return RGBDImage.create_from_color_and_depth(rgb.reshape(H, W, 3), d, depth_scale=1.0, depth_trunc=6000.0, convert_rgb_to_intensity=True)


def images(name, masked=False):
    """(intensity, depth) float32 (H, W) of frame 'A', 'B' or 'P'"""
    s = scene()
    im = rgbd(s["depth_" + name], s["rgb_" + name], s["mask_P"] if masked else None)
    return np.asarray(im.color), np.asarray(im.depth)


def option(iterations=(20, 10, 5)):
    return R.Option(iterations, **OPTION_MM)


def odd_image(seed=5):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-3.0, 900.0, size=(53, 75)).astype(np.float32)
    a[rng.random(a.shape) < 0.03] = np.nan
    a[0, 0] = a[52, 74] = a[20, 0] = np.nan                      # holes on corners and on an edge
    return a


def collision():
    """(depth_s, depth_t, K4, extrinsic, depth_diff_max)"""
    T = np.eye(4)
    T[2, 3] = 600.0
    return np.full((H, W), 2000.0, np.float32), np.full((H, W), 2600.0, np.float32), K4, T, 30.0


def perturbed_init():
    return rigid(0.7, (1.0, -0.4, 0.5), (12.0, 9.0, -15.0))


# the whole-chain cases of both suites: (source, target, init, jacobian, iterations)
CHAIN_CASES = {
    "identity-hybrid-20-10-5": ("A", "B", None, R.HYBRID, (20, 10, 5)),
    "perturbed-hybrid-20-10-5": ("A", "B", "perturbed", R.HYBRID, (20, 10, 5)),
    "identity-color-20-10-5": ("A", "B", None, R.COLOR, (20, 10, 5)),          # runs out of correspondences at 20 x 18: a failure
    "identity-hybrid-3": ("A", "B", None, R.HYBRID, (3,)),
    "perturbed-color-3": ("A", "B", "perturbed", R.COLOR, (3,)),
    "identity-hybrid-0-0-2": ("A", "B", None, R.HYBRID, (0, 0, 2)),
    "identity-color-0-0-2": ("A", "B", None, R.COLOR, (0, 0, 2)),
}


@functools.lru_cache(maxsize=None)
def chain_reference(case, n_perm=3):
    """the restatement's result of a chain case, its spread over permuted summation orders and its decision margins ->
    dict(success, T, info, spread_T (= max of spread_R, the rotation entries, and spread_t, the translation), spread_info, margins, ...)"""
    src, tgt, init, jac, its = CHAIN_CASES[case]
    T0 = perturbed_init() if init == "perturbed" else np.eye(4)
    (Is, Ds), (It, Dt) = images(src), images(tgt)
    m = R.Margins()
    ok, T, G = R.odometry(Is, Ds, It, Dt, K4, T0, jac, option(its), None, m)
    sR = st = sG = 0.0
    for k in range(n_perm):
        ok2, T2, G2 = R.odometry(Is, Ds, It, Dt, K4, T0, jac, option(its), 1000 * (k + 1), m)
        assert ok2 == ok
        sR, st = max(sR, float(np.abs(T2 - T)[:3, :3].max())), max(st, float(np.abs(T2 - T)[:3, 3].max()))
        sG = max(sG, R.sums_difference(G2, G))
    return {"success": ok, "T": T, "info": G, "spread_T": max(sR, st), "spread_R": sR, "spread_t": st, "spread_info": sG, "margins": m, "init": T0,
            "jacobian": jac, "iterations": its}


@functools.lru_cache(maxsize=None)
def levels_reference():
    """the A -> B pair's preprocessed pyramids at the identity (three levels), as R.prepare returns them"""
    (Is, Ds), (It, Dt) = images("A"), images("B")
    return R.prepare(Is, Ds, It, Dt, K4, np.eye(4), option())


@functools.lru_cache(maxsize=None)
def iteration_reference(jacobian, level, n_perm=3):
    """one iteration of the A -> B pair at `level` from perturbed_init(): the restatement's sums, count and new pose, and their spread
    over permuted correspondence orders (sums: relative to the largest |entry| of J^T J and of J^T r; pose: absolute)"""
    lv, Kl, T0 = levels_reference()[level], R.level_camera(K4, level), perturbed_init()
    m = R.Margins()
    sums, n, ok, T = R.iteration(*lv, Kl, T0, jacobian, OPTION_MM["depth_diff_max"], None, m)
    sA = sb = sT = 0.0
    for k in range(n_perm):
        s2, n2, ok2, T2 = R.iteration(*lv, Kl, T0, jacobian, OPTION_MM["depth_diff_max"], 1000 * (k + 1))
        assert (n2, ok2) == (n, ok)
        sA, sb = max(sA, R.sums_difference(s2[:21], sums[:21])), max(sb, R.sums_difference(s2[21:27], sums[21:27]))
        sT = max(sT, float(np.abs(T2 - T).max()))
    return {"sums": sums, "count": n, "solved": ok, "T": T, "spread_JTJ": sA, "spread_JTr": sb, "spread_T": sT, "margins": m, "init": T0}

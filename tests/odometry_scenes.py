"""Fixtures of the odometry suites (tests/test_odometry_cpu.py, tests/test_odometry_gpu.py).  The first set is on the 80 x 72 camera
synth.small_xy(8), K = (63, 63, 40, 36), millimetres; fixture() further down adds the same room at 320 x 288, crops, and metres.

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
import os

import numpy as np
from PIL import Image

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


def _chain_reference(Is, Ds, It, Dt, K, T0, jac, opt, n_perm):
    m = R.Margins()
    ok, T, G = R.odometry(Is, Ds, It, Dt, K, T0, jac, opt, None, m)
    sR = st = sG = 0.0
    for k in range(n_perm):
        ok2, T2, G2 = R.odometry(Is, Ds, It, Dt, K, T0, jac, opt, 1000 * (k + 1), m)
        assert ok2 == ok
        sR, st = max(sR, float(np.abs(T2 - T)[:3, :3].max())), max(st, float(np.abs(T2 - T)[:3, 3].max()))
        sG = max(sG, R.sums_difference(G2, G))
    return {"success": ok, "T": T, "info": G, "spread_T": max(sR, st), "spread_R": sR, "spread_t": st, "spread_info": sG, "margins": m, "init": T0,
            "jacobian": jac, "iterations": tuple(opt.iterations)}


@functools.lru_cache(maxsize=None)
def chain_reference(case, n_perm=3):
    """the restatement's result of a chain case, its spread over permuted summation orders and its decision margins ->
    dict(success, T, info, spread_T (= max of spread_R, the rotation entries, and spread_t, the translation), spread_info, margins, ...)"""
    src, tgt, init, jac, its = CHAIN_CASES[case]
    T0 = perturbed_init() if init == "perturbed" else np.eye(4)
    (Is, Ds), (It, Dt) = images(src), images(tgt)
    return _chain_reference(Is, Ds, It, Dt, K4, T0, jac, option(its), n_perm)


@functools.lru_cache(maxsize=None)
def levels_reference():
    """the A -> B pair's preprocessed pyramids at the identity (three levels), as R.prepare returns them"""
    (Is, Ds), (It, Dt) = images("A"), images("B")
    return R.prepare(Is, Ds, It, Dt, K4, np.eye(4), option())


def _iteration_reference(lv, Kl, T0, dmax, jacobian, n_perm):
    m = R.Margins()
    sums, n, ok, T = R.iteration(*lv, Kl, T0, jacobian, dmax, None, m)
    sA = sb = sT = 0.0
    for k in range(n_perm):
        s2, n2, ok2, T2 = R.iteration(*lv, Kl, T0, jacobian, dmax, 1000 * (k + 1))
        assert (n2, ok2) == (n, ok)
        sA, sb = max(sA, R.sums_difference(s2[:21], sums[:21])), max(sb, R.sums_difference(s2[21:27], sums[21:27]))
        sT = max(sT, float(np.abs(T2 - T).max()))
    return {"sums": sums, "count": n, "solved": ok, "T": T, "spread_JTJ": sA, "spread_JTr": sb, "spread_T": sT, "margins": m, "init": T0,
            "correspondences": R.correspondence(Kl, T0, lv[1], lv[3], dmax)}


@functools.lru_cache(maxsize=None)
def iteration_reference(jacobian, level, n_perm=3):
    """one iteration of the A -> B pair at `level` from perturbed_init(): the restatement's sums, count and new pose, and their spread
    over permuted correspondence orders (sums: relative to the largest |entry| of J^T J and of J^T r; pose: absolute)"""
    return _iteration_reference(levels_reference()[level], R.level_camera(K4, level), perturbed_init(), OPTION_MM["depth_diff_max"], jacobian, n_perm)


# ---- beyond the one 80 x 72 millimetre camera: more than 256 blocks, odd pyramid levels, metres ----------------------------------------
@functools.lru_cache(maxsize=None)
def scene_at(scale):
    """scene() on synth.small_xy(scale) with K4 * 8 / scale: the same room, poses and colour field; plus W, H, K4"""
    xy = synth.small_xy(scale)
    A = synth.camera_pose(0, 4)
    B = A @ rigid(MOTION_DEG, MOTION_AXIS, MOTION_T)
    s = {"xy": xy, "A": A, "B": B, "truth": np.linalg.inv(B) @ A, "W": synth.W // scale, "H": synth.H // scale,
         "K4": tuple(k * 8.0 / scale for k in K4)}
    for name, E in (("A", A), ("B", B)):
        s["depth_" + name] = synth.render_depth(E=E, xy=xy, noise=0, drop=0, person_shift=AWAY)
        s["rgb_" + name] = paint(s["depth_" + name], E, xy)
    return s


def rgbd_at(depth, rgb, w, h, depth_scale=1.0, depth_trunc=6000.0):
    """rgbd() for a frame of any size and unit"""
    return RGBDImage.create_from_color_and_depth(rgb.reshape(h, w, 3), depth.reshape(h, w), depth_scale=depth_scale, depth_trunc=depth_trunc,
                                                 convert_rgb_to_intensity=True)


OPTION_M = dict(depth_diff_max=0.03, depth_min=0.0, depth_max=6.0)
CROPS = {"75x53": (75, 53), "79x71": (79, 71), "65x65": (65, 65)}          # levels 37 x 26, 18 x 13; 39 x 35, 19 x 17; 32 x 32 (four blocks), 16 x 16 (one)
TRUNC_M = {"metres": 6.0, "metres-trunc": 3.5, "metres-trunc-5.5": 5.5, "metres-trunc-5.5-reversed": 5.5}          # depth_trunc of the metre fixtures
FIXTURES = ("320x288",) + tuple(CROPS) + tuple(TRUNC_M)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """a source / target pair beside scene(): dict(frames (the scene's frames it is made of, source then target), W, H, K4, opt (the OdometryOption values), unit (data units per millimetre), init
    (perturbed_init() in the pair's units), truth, Is, Ds, It, Dt float32 (H, W) as compute_rgbd_odometry takes them)
      320x288  scene_at(2): 360 blocks, so that the last-ticket block adds two slab columns in some threads; levels 160 x 144, 80 x 72
      crops    top-left crops of the 80 x 72 images with the same K4: levels of odd size, of exactly four blocks and one block
      metres   the 80 x 72 frames through depth_scale 1000 with Open3D's own kind of option, (0.03, 0, 6.0); metres-trunc: the same with
               depth_trunc 3.5, which cuts the far wall (at 5.5 m) and the side walls behind 3.5 m.  Every correspondence within 0.03 m
               of this pair lies on those walls -- on the floor one pixel is tens of millimetres of depth -- so that pair FAILS, on the
               host and on the device alike; metres-trunc-5.5 cuts only the part of the target's far wall behind 5.5 m (850 pixels)
               and succeeds.  No depth_trunc between 3.5 and 5.5 succeeds for A -> B: A sees the far wall head-on, every pixel of it at
               exactly 5.5 m, so anything below takes all of it.  metres-trunc-5.5-reversed is B -> A from the inverse pose: there the
               truncation bites the SOURCE (850 pixels) and the chain succeeds"""
    init, truth = perturbed_init(), scene()["truth"].copy()
    if name == "320x288":
        s = scene_at(2)
        w, h, K, opt, unit = s["W"], s["H"], s["K4"], OPTION_MM, 1.0
        ims = [rgbd_at(s["depth_" + f], s["rgb_" + f], w, h) for f in "AB"]
        planes = [(np.asarray(im.color), np.asarray(im.depth)) for im in ims]
    elif name in CROPS:
        w, h = CROPS[name]
        K, opt, unit = K4, OPTION_MM, 1.0
        planes = [tuple(np.ascontiguousarray(p[:h, :w]) for p in images(f)) for f in "AB"]
    elif name in TRUNC_M:
        s = scene()
        w, h, K, opt, unit = W, H, K4, OPTION_M, 1e-3
        frames = "BA" if name.endswith("-reversed") else "AB"
        ims = [rgbd_at(s["depth_" + f], s["rgb_" + f], w, h, 1000.0, TRUNC_M[name]) for f in frames]
        planes = [(np.asarray(im.color), np.asarray(im.depth)) for im in ims]
        init[:3, 3] *= 1e-3
        truth[:3, 3] *= 1e-3
        if frames == "BA":
            init, truth = np.linalg.inv(init), np.linalg.inv(truth)
    else:
        raise KeyError(name)
    (Is, Ds), (It, Dt) = planes
    return {"frames": frames if name in TRUNC_M else "AB", "W": w, "H": h, "K4": K, "opt": opt, "unit": unit, "init": init, "truth": truth, "Is": Is, "Ds": Ds, "It": It, "Dt": Dt}


def fixture_option(name, iterations=(20, 10, 5)):
    return R.Option(iterations, **fixture(name)["opt"])


def bound_constants(name):
    """how far a pose error moves a decision of the fixture: (pixels per unit error of a rotation entry, pixels per data unit of
    translation, z' per unit error of a rotation entry, z' per data unit of translation).  The derivation of
    test_summation_order_spread with the fixture's own fx and units: a rotation entry off by e moves a projection by at most
    fx (|x| + |y| + |z|) / z e < (200 fx / 63) e pixels -- the field of view (|x| + |y| + |z|) / z < 2.21 is the same at every
    resolution and for a crop -- and z' by at most 3 depth_max e; a translation off by e moves a projection by at most fx / z_min e
    (z_min = 252 mm: the renderer drops what is nearer than 250) and z' by e"""
    f = fixture(name)
    fx, unit = f["K4"][0], f["unit"]
    return 200.0 * fx / 63.0, 0.25 * fx / 63.0 / unit, 3.0 * f["opt"]["depth_max"], 1.0


# the chain cases of the fixtures above, all from perturbed_init(): (fixture, jacobian, iterations).  (From the identity the 320 x 288
# pair has depth differences exactly equal to depth_diff_max: a depth margin of 0.)  The colour term runs out of correspondences on
# the coarse levels of the crops, as identity-color-20-10-5 does at 80 x 72: it runs on one level there, and one multi-level case is
# kept as a failure.
NEW_CHAIN_CASES = {}
for _jac, _jn in ((R.HYBRID, "hybrid"), (R.COLOR, "color")):
    for _its in ((2, 2, 2), (3,), (0, 0, 2)):
        NEW_CHAIN_CASES["320x288-" + _jn + "-" + "-".join(map(str, _its))] = ("320x288", _jac, _its)
for _crop in CROPS:
    NEW_CHAIN_CASES[_crop + "-hybrid-20-10-5"] = (_crop, R.HYBRID, (20, 10, 5))
    NEW_CHAIN_CASES[_crop + "-hybrid-4-3-2"] = (_crop, R.HYBRID, (4, 3, 2))
    NEW_CHAIN_CASES[_crop + "-color-3"] = (_crop, R.COLOR, (3,))
NEW_CHAIN_CASES["75x53-color-4-3-2"] = ("75x53", R.COLOR, (4, 3, 2))          # a failure: no correspondence left on a coarse level
NEW_CHAIN_CASES["metres-hybrid-20-10-5"] = ("metres", R.HYBRID, (20, 10, 5))
NEW_CHAIN_CASES["metres-trunc-hybrid-20-10-5"] = ("metres-trunc", R.HYBRID, (20, 10, 5))          # a failure: see fixture()
NEW_CHAIN_CASES["metres-trunc-5.5-hybrid-20-10-5"] = ("metres-trunc-5.5", R.HYBRID, (20, 10, 5))
NEW_CHAIN_CASES["metres-trunc-5.5-reversed-hybrid-20-10-5"] = ("metres-trunc-5.5-reversed", R.HYBRID, (20, 10, 5))
NEW_FAILURES = ("75x53-color-4-3-2", "metres-trunc-hybrid-20-10-5")


@functools.lru_cache(maxsize=None)
def new_chain_reference(case, n_perm=3):
    """chain_reference() for a case of NEW_CHAIN_CASES"""
    name, jac, its = NEW_CHAIN_CASES[case]
    f = fixture(name)
    return _chain_reference(f["Is"], f["Ds"], f["It"], f["Dt"], f["K4"], f["init"], jac, fixture_option(name, its), n_perm)


@functools.lru_cache(maxsize=None)
def fixture_levels(name):
    """the fixture's preprocessed pyramids (three levels), normalised at its perturbed pose, as R.prepare returns them"""
    f = fixture(name)
    return R.prepare(f["Is"], f["Ds"], f["It"], f["Dt"], f["K4"], f["init"], fixture_option(name))


@functools.lru_cache(maxsize=None)
def fixture_iteration_reference(name, jacobian, level, pose="init", n_perm=3):
    """iteration_reference() on fixture_levels(name) from the fixture's "init" or "truth"; with the iteration's correspondences"""
    f = fixture(name)
    return _iteration_reference(fixture_levels(name)[level], R.level_camera(f["K4"], level), f[pose], f["opt"]["depth_diff_max"], jacobian, n_perm)


def holed_depth_A(drop=0.15, seed=17):
    """depth_A with 15 % of its pixels dropped at random: after the Gaussian's NaN spread level 0 keeps 335 correspondences with B at
    perturbed_init(), level 1 29 and level 2 none -- a chain over three levels fails in its FIRST iteration, on the coarsest level, and
    would find correspondences again on the finer ones"""
    d = scene()["depth_A"].copy()
    d[np.random.default_rng(seed).random(d.size) < drop] = 0
    return d


def write_device(root, stamps, depth_xyz, rgbs, shape=(synth.H, synth.W)):
    """one device's directory as the reference's recorder leaves it: color/<stamp>_rgb.png and depths/<stamp>_depth.dat (int16 XYZ)"""
    os.makedirs(os.path.join(root, "color")); os.makedirs(os.path.join(root, "depths"))
    os.makedirs(os.path.join(root, "filtered_and_registered_pointclouds"))
    for ts, xyz, rgb in zip(stamps, depth_xyz, rgbs):
        xyz.astype(np.int16).tofile(os.path.join(root, "depths", f"{ts}_depth.dat"))
        Image.fromarray(rgb.reshape(shape[0], shape[1], 3)).save(os.path.join(root, "color", f"{ts}_rgb.png"))


def drift_directory(root):
    """a two-device, two-frame recording of 80 x 72 frames under `root` for DataProcessor's drift check: device 0 sees A then P (B with
    the person, which mask_fn marks), device 1 sees B then A.  -> (dirs, mask_fn, depths uint16 (frame, device, n_px), colours uint8
    (frame, device, n_px, 3), masks bool (frame, device, n_px))"""
    s = scene()
    order = (("A", "B"), ("P", "A"))                                  # [frame][device]
    depths = np.stack([np.stack([s["depth_" + n] for n in row]) for row in order])
    colors = np.stack([np.stack([s["rgb_" + n] for n in row]) for row in order])
    masks = np.zeros(depths.shape, bool)
    masks[1, 0] = s["mask_P"]
    x, y = np.nan_to_num(s["xy"][:, 0]), np.nan_to_num(s["xy"][:, 1])
    dirs = [os.path.join(str(root), "master_1"), os.path.join(str(root), "sub_1")]
    for d, stamps in enumerate(((900, 1000), (905, 1004))):           # "900" sorts before "1000": numeric order
        xyz = [np.stack([np.rint(x * depths[f, d]), np.rint(y * depths[f, d]), depths[f, d]], 1) for f in range(2)]
        write_device(dirs[d], stamps, xyz, [colors[f, d] for f in range(2)], (H, W))
    by_image = {colors[f, d].tobytes(): masks[f, d] for f in range(2) for d in range(2)}

    def mask_fn(img):                                                 # stand-in for Mask R-CNN: the renderer's person mask
        return by_image[np.ascontiguousarray(img).tobytes()].reshape(img.shape[:2])

    return dirs, mask_fn, depths, colors, masks

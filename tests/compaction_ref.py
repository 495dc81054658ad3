"""Plain helpers (no GPU) for the stream-compaction tests: which form of the order-preserving compaction a call takes, inputs whose
kept items are laid out in whole tiles, NumPy references where the C oracle has none, and the comparison the GPU tests use.

`compact_form` restates the switch conditions of kpx_compact.h (compact_plan, compact_scan_threads, use_onepass), of kpx_container.hip
(points_plan) and of kpx_extract.hip (px8_plan, the vector-path conditions of kpx_depth_to_cloud / kpx_rgbd_compact); the constants
below must be moved with the library's."""
import numpy as np

TILE = 2048                  # kpx_compact.h kCompactTile = kCompactThreads (256) x kCompactItems (8)
ONE_PASS_TILES = 2048        # kpx_compact.h kOnePassTiles: the look-back kernels serve up to this many tiles (x frames)
SCAN_WIDE_ABOVE = 2048       # compact_scan_threads: 256 threads up to here, 1024 above
SCAN_ITEMS = 8               # kpx_compact.hip compact_scan_body: counts per thread and round
FRAME_MAJOR_MIN, FRAME_MAJOR_MAX = 8, 65535      # px8_plan: the frame-major one-pass grid's range of frame counts
FRAME_MAJOR_MAX_TILES = 65535                    # px8_plan: ... and the most tiles per frame (they are the grid's y dimension)
GATE_MM = 750.0

GENERIC_ONEPASS, GENERIC_THREE = "generic one-pass", "generic three-launch"
PX8_TILE_MAJOR, PX8_FRAME_MAJOR, PX8_THREE = "px8 one-pass tile-major", "px8 one-pass frame-major", "px8 three-launch"
POINTS_ONEPASS, POINTS_FLAGS = "points one-pass", "points flag/scan/scatter"
ALL_FORMS = (GENERIC_ONEPASS, GENERIC_THREE, PX8_TILE_MAJOR, PX8_FRAME_MAJOR, PX8_THREE, POINTS_ONEPASS, POINTS_FLAGS)


def tiles_of(n):
    """compact_tiles"""
    return -(-max(int(n), 1) // TILE)


def scan_shape(tiles):
    """the scan launch of a three-launch form: (threads, carry) -- carry: the row of tiles exceeds one round of 8 x blockDim counts"""
    threads = 1024 if tiles > SCAN_WIDE_ABOVE else 256
    return threads, tiles > SCAN_ITEMS * threads


def extract_is_vec(n, depth_off=0, rgb_off=None):
    """the 8-pixel path of kpx_depth_to_cloud / kpx_rgbd_compact: n % 8 == 0, the depth (or XYZ) buffer 16-byte aligned and the colour
    buffer, when there is one, 8-byte aligned.  *_off: the buffer's first byte modulo its alignment (rgb_off None: no colours)"""
    return n % 8 == 0 and depth_off % 16 == 0 and (rgb_off is None or rgb_off % 8 == 0)


def compact_form(n, frames, vec, lists=1, kind="extract", onepass=None, onepass_batch=True):
    """-> (form, scan): scan = (threads, carry) of the scan launch, None for a one-pass form.
    kind: "extract" (kpx_depth_to_cloud, kpx_rgbd_compact: px8_compact when `vec`, compact() otherwise), "generic" (every other caller
    of compact(): one frame) or "points" (compact_points: half-space with lists = 1, slab split with lists = 2).
    onepass / onepass_batch: KPX_ONEPASS (None = unset, 0, 1) and KPX_ONEPASS_BATCH (False = "0")."""
    tiles = tiles_of(n)
    use_onepass = lambda total: total <= ONE_PASS_TILES if onepass is None else bool(onepass)
    if kind == "points":
        assert frames == 1 and lists in (1, 2)
        if lists == 1 and use_onepass(tiles):
            return POINTS_ONEPASS, None
        return POINTS_FLAGS, scan_shape(tiles)
    assert lists == 1 and kind in ("extract", "generic") and (kind == "extract" or (frames == 1 and not vec))
    small = use_onepass(tiles * frames)
    if not vec:
        return (GENERIC_ONEPASS, None) if small else (GENERIC_THREE, scan_shape(tiles))
    if small:
        return PX8_TILE_MAJOR, None
    if onepass_batch and FRAME_MAJOR_MIN <= frames <= FRAME_MAJOR_MAX and tiles <= FRAME_MAJOR_MAX_TILES:
        return PX8_FRAME_MAJOR, None
    return PX8_THREE, scan_shape(tiles)


# ------------------------------------------------------------------------------------------------ tile plans
EMPTY, FULL, MIXED = 0, 1, 2


def tile_plan(tiles, rng, ends="lead"):
    """kinds of the tiles of one frame / cloud.  A run of three empty tiles: ends = "lead" at the start (the last, ragged tile is mixed and
    keeps its last item), "late" at the end (with the ragged tile; tile 1 holds items and a run of empties sits in the middle), "both" at
    the start and at the end.  Full tiles next to the runs and one in the middle; the rest mixed, with more whole empty and full tiles
    sprinkled in.  Needs at least 20 tiles."""
    assert tiles >= 20 and ends in ("lead", "late", "both")
    plan = np.full(tiles, MIXED, np.int8)
    r = rng.random(tiles)
    plan[r < 0.08] = EMPTY
    plan[r > 0.92] = FULL
    plan[:4] = MIXED
    plan[tiles - 4:] = MIXED
    if ends in ("lead", "both"):
        plan[0:3] = EMPTY
        plan[3] = FULL
    else:
        plan[4:7] = EMPTY
        plan[7] = FULL
    plan[tiles // 2] = FULL
    plan[tiles // 2 + 1] = MIXED
    if ends in ("late", "both"):
        plan[tiles - 4] = FULL
        plan[tiles - 3:] = EMPTY
    return plan


def _keep_mask(n, plan, rng):
    """the kept items of a plan: a mixed tile keeps its first item and drops its last (neither empty nor full), except the ragged last
    tile, which keeps the last item there is"""
    keep = np.zeros(len(plan) * TILE, bool)
    per_tile = keep.reshape(len(plan), TILE)
    per_tile[plan == FULL] = True
    mixed = np.flatnonzero(plan == MIXED)
    dens = rng.uniform(0.02, 0.98, size=(len(mixed), 1))
    per_tile[mixed] = rng.random((len(mixed), TILE)) < dens
    per_tile[mixed, 0] = True
    per_tile[mixed, TILE - 1] = False
    if plan[-1] == MIXED:
        keep[n - 1] = True
        if n % TILE != 1:
            keep[n - 2] = False
    return keep[:n]


# frame kinds of a batch, in order: a planned frame that starts with a run of empty tiles ("lead"), a completely empty frame between
# non-empty ones, a planned frame that ends with such a run ("late"), a completely full frame, then planned frames alternating the two plans
def frame_kinds(frames):
    kinds = ["lead", "empty", "late", "full"][:frames] if frames >= 3 else ["lead", "late"][:frames]
    while len(kinds) < frames:
        kinds.append("lead" if len(kinds) % 2 == 0 else "late")
    return kinds


def extract_batch(n, frames, seed, nan=True):
    """-> dict(depth u16 (F, n), xy f32 (n, 2), rgb u8 (F, n, 3), kinds, nan_px).
    A pixel is kept by the flag-less compaction exactly when its depth is non-zero and its table entry is finite (the table's
    magnitudes keep x and y away from 0).  The table's NaN entries sit in tile 8 and in the middle tile + 1 only, so the promised full
    tiles stay full; a NaN pixel is dropped from every frame, the "full" frame included (xyz_images patches that frame's image for
    the XYZ entry, which has no table).  rgb: random colours with zero pixels (the colour mask's holes), each frame its own density."""
    rng = np.random.default_rng(seed)
    tiles = tiles_of(n)
    xy = (rng.uniform(0.01, 0.6, size=(n, 2)) * rng.choice([-1.0, 1.0], size=(n, 2))).astype(np.float32)
    nan_px = np.zeros(n, bool)
    if nan:
        for t in (8, tiles // 2 + 1):
            nan_px[t * TILE + rng.choice(TILE, 37, replace=False)] = True
        xy[nan_px, rng.integers(0, 2, int(nan_px.sum()))] = np.nan
    kinds = frame_kinds(frames)
    depth = rng.integers(300, 6000, size=(frames, n)).astype(np.uint16)
    for f, kind in enumerate(kinds):
        if kind == "empty":
            depth[f] = 0
        elif kind != "full":
            depth[f][~_keep_mask(n, tile_plan(tiles, rng, kind), rng)] = 0
    rgb = rng.integers(1, 255, size=(frames, n, 3)).astype(np.uint8)
    for f in range(frames):
        rgb[f][rng.random(n) < rng.uniform(0.05, 0.6)] = 0
    return dict(depth=depth, xy=xy, rgb=rgb, kinds=kinds, nan_px=nan_px)


def xyz_images(batch, unproject):
    """the int16 XYZ images of a batch (unproject: oracle.unproject_u16); the full frame's NaN pixels are given a point, so that the
    XYZ entry sees a frame with every pixel kept"""
    xyz = np.stack([unproject(d, batch["xy"]) for d in batch["depth"]])
    for f, kind in enumerate(batch["kinds"]):
        if kind == "full":
            xyz[f][batch["nan_px"]] = (5, -7, 1000)
    return xyz


def tile_counts(idx, n):
    """kept items per tile from a kept-index list"""
    return np.bincount(np.asarray(idx, np.int64) // TILE, minlength=tiles_of(n))


def clustered_cloud(n, seed):
    """-> (pts f32 (n, 3), neg bool (n)): integer-valued coordinates, |x|, |z| <= 100 and 100 <= |y| <= 1000, y multiplied by a per-tile
    sign pattern (tile_plan: EMPTY = +, FULL = -, MIXED = random signs).  Every selection below is decided by the sign of y, in exact
    arithmetic: whole tiles are kept, whole tiles are dropped.  One NumPy call per coordinate block."""
    rng = np.random.default_rng(seed)
    pts = rng.integers(-100, 101, size=(n, 3)).astype(np.float32)
    neg = _keep_mask(n, tile_plan(tiles_of(n), rng, "both"), rng)
    y = rng.integers(100, 1001, size=n).astype(np.float32)
    pts[:, 1] = np.where(neg, -y, y)
    return pts, neg


HALF_PLANE = (0.5, 2.0, -0.25, 8.0)        # |0.5 x - 0.25 z + 8| <= 83 < 2 |y|: keeps exactly the points with y < 0
NONE_PLANE = (0.5, 2.0, -0.25, 4096.0)     # keeps nothing
ALL_PLANE = (0.5, 2.0, -0.25, -4096.0)     # keeps everything


def halfspace_ref(pts, plane):
    """floor_removal's half space: keep where a x + b y + c z + d is not >= 0 (float64, left to right)"""
    a, b, c, d = plane
    p = np.asarray(pts, np.float64)
    return np.flatnonzero(~(((a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]) + d >= 0)).astype(np.int32)


def slab_ref(pts, slab):
    """floor_removal's slab: (lower, upper) = (y >= max(y) - slab, y < max(y) - slab)"""
    y = np.asarray(pts)[:, 1].astype(np.float64)
    cut = y.max() - slab
    return np.flatnonzero(y >= cut).astype(np.int32), np.flatnonzero(y < cut).astype(np.int32)


def mask_select_ref(attr, idx, invert=False):
    """Open3D's SelectByIndex: mask semantics"""
    m = np.zeros(len(attr), bool)
    m[np.asarray(idx, np.int64)] = True
    return attr[~m] if invert else attr[m]


# ------------------------------------------------------------------------------------------------ the comparison
def compare_frames(got, want, tag=()):
    """got: per frame a tuple of arrays (None allowed) trimmed to the frame's count; want: the same from the reference.  Every frame,
    every array, bit for bit -- lengths (the counts) first."""
    assert len(got) == len(want), (tag, "frames", len(got), len(want))
    for f, (g, w) in enumerate(zip(got, want)):
        for j, (a, b) in enumerate(zip(g, w)):
            if a is None or b is None:
                continue
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape, (tag, "frame", f, "array", j, "count", a.shape, b.shape)
            if not np.array_equal(a, b):
                bad = np.flatnonzero((a != b).reshape(len(a), -1).any(1))
                raise AssertionError((tag, "frame", f, "array", j, "first differing row", int(bad[0]), "rows differing", len(bad)))


def compare_padded(pts, col, idx, cnt, want, tag=()):
    """the sync=False outputs (padded buffers (F, n, ..) and the device counts): the counts, and the rows below each count; what lies
    beyond a count is not compared"""
    ks = [int(k) for k in np.asarray(cnt)]
    assert ks == [len(w[0]) for w in want], (tag, "counts", ks)
    compare_frames([(pts[f, :k] if pts is not None else None, col[f, :k] if col is not None else None, idx[f, :k] if idx is not None else None)
                    for f, k in enumerate(ks)], want, tag)


# ------------------------------------------------------------------------------------------------ inputs of the forced-form runs
def forced_inputs():
    """the inputs every child process of the forced-form test (KPX_ONEPASS, KPX_ONEPASS_BATCH) and the parent's oracle build alike: 150 to
    400 tiles per compaction, so that a look-back walks more than one 64-tile window"""
    from kinectpy_amd.utils import synth
    from tests import globalreg_ref
    T = TILE
    rng = np.random.default_rng(77)
    room = synth.filter_cloud(150 * T + 5, seed=37)
    big = synth.filter_cloud(400 * T - 3, seed=38)
    nrm = rng.standard_normal(big.shape)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    src, tgt, corr = globalreg_ref.corres_scene(synth.frame_cloud(), 1000, 0.15, 0.0, 2000, 1)
    Ts = [np.eye(4), synth.t_star()]
    return dict(
        ext={"vec3": extract_batch(200 * T - 2040, 3, 31), "odd3": extract_batch(200 * T - 2047, 3, 32),
             "vec8": extract_batch(257 * T - 2040, 8, 33), "odd9": extract_batch(150 * T + 1, 9, 34)},
        cloud=clustered_cloud(300 * T + 5, 35)[0], cloud_2049=clustered_cloud(2049 * T - 3, 36)[0],
        room=room, big=big, big_col=rng.random(big.shape).astype(np.float32), big_nrm=nrm,
        batch=[np.ascontiguousarray(big[: 200 * T + 1]), np.ascontiguousarray(room[: 160 * T // 2 + 7] + np.float32(3.0))],
        fuse=[np.ascontiguousarray(big[: 180 * T]), np.ascontiguousarray(room[: 120 * T + 9])], fuse_T=Ts,
        ransac=(src, tgt, corr))

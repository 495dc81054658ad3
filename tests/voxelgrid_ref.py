"""NumPy restatement of the arithmetic contract AC10: Open3D's VoxelGrid -- the grid of a cloud, the dense
grid, space carving by depth maps and silhouettes, point inclusion and the bounds -- operation by operation in float64, every fused
multiply-add an exact one (tsdf_ref.fma).  Vectorised over voxels x corners.

A grid is (idx int64 (M, 3) strictly ascending in (gx, gy, gz), colours float32 (M, 3), origin float64[3], voxel size).
"""
import numpy as np

from tsdf_ref import ac1, depth_from_u16, fma  # noqa: F401  (fma and depth_from_u16 are part of this module's surface)

AXIS_BITS = 21
AXIS_CELLS = 1 << AXIS_BITS
MAX_IMAGES = 8              # KPX_VOXELGRID_MAX_IMAGES: images per launch of the carve kernel
INT_MAX = 2147483647
CORNER_SIGNS = np.array([[(t >> k) & 1 for k in range(3)] for t in range(8)], dtype=bool)          # (8, 3): True = centre + r


def keys_of(idx):
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    return (idx[:, 0] << (2 * AXIS_BITS)) | (idx[:, 1] << AXIS_BITS) | idx[:, 2]


def cell(points, origin, v):
    """g = floor((p - origin) / v) as float64 (N, 3): NaN and out-of-range values are left to the caller"""
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.floor((p - np.asarray(origin, np.float64).reshape(1, 3)) / float(v))


def in_range(f):
    """every component in [0, 2^21); NaN is not"""
    with np.errstate(invalid="ignore"):
        return ((f >= 0.0) & (f < float(AXIS_CELLS))).all(1)


# ---- constructors ------------------------------------------------------------------------------------------------------------------
def create_from_point_cloud(points, v, colors=None, origin=None):
    """points float32 (N, 3); origin None: min_bound - v 0.5 (create_from_point_cloud), else the caller's min_bound
    (create_from_point_cloud_within_bounds).  -> idx, colours, origin"""
    v = float(v)
    if not v > 0.0:
        raise ValueError("voxel_size <= 0")
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    if origin is None:
        lo = p.min(0) if len(p) else np.zeros(3)
        origin = lo - v * 0.5
        if len(p) and v * INT_MAX < (p.max(0) - lo).max():
            raise ValueError("voxel_size is too small")
    origin = np.asarray(origin, np.float64).reshape(3)
    f = cell(p, origin, v)
    if not in_range(f).all():
        raise ValueError("voxel_size is too small")          # the library's one range error
    key = keys_of(f.astype(np.int64))
    uniq, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    idx = np.stack([uniq >> (2 * AXIS_BITS), (uniq >> AXIS_BITS) & (AXIS_CELLS - 1), uniq & (AXIS_CELLS - 1)], 1).astype(np.int64)
    col = np.zeros((len(uniq), 3), np.float32)
    if colors is not None:
        acc = np.zeros((len(uniq), 3))
        np.add.at(acc, inv, np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64))          # unbuffered: ascending point index
        col = (acc / np.bincount(inv, minlength=len(uniq)).astype(np.float64)[:, None]).astype(np.float32)
    return idx, col, origin


def round_half_away(q):
    """std::round"""
    n = np.floor(abs(q))
    return int(np.sign(q)) * (int(n) + (1 if abs(q) - n >= 0.5 else 0))


def create_dense(origin, color, v, width, height, depth):
    n = [round_half_away(float(e) / float(v)) for e in (width, height, depth)]
    if min(n) < 0 or max(n) > AXIS_CELLS or n[0] * n[1] * n[2] > INT_MAX:
        raise ValueError("create_dense: dimensions out of range")
    g = np.stack(np.meshgrid(np.arange(n[0]), np.arange(n[1]), np.arange(n[2]), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    return g, np.repeat(np.asarray(color, np.float64).astype(np.float32).reshape(1, 3), len(g), 0), np.asarray(origin, np.float64).reshape(3)


# ---- geometry of a voxel ---------------------------------------------------------------------------------------------------------------
def centres(idx, origin, v):
    """c_k = origin_k + (g_k + 0.5) v: add, multiply, add"""
    return np.asarray(origin, np.float64).reshape(1, 3) + (np.asarray(idx, np.int64).reshape(-1, 3).astype(np.float64) + 0.5) * float(v)


def corners(idx, origin, v):
    """(M, 8, 3): c_k +- r with r = v 0.5"""
    c = centres(idx, origin, v)[:, None, :]
    r = float(v) * 0.5
    return np.where(CORNER_SIGNS[None, :, :], c + r, c - r)


def project(x, intrinsic, extrinsic):
    """x (..., 3) world points -> u, v, z; no test of the sign of z: IEEE division decides"""
    fx, fy, cx, cy = (float(t) for t in intrinsic)
    E = np.asarray(extrinsic, np.float64).reshape(4, 4)
    X, Y, z = ac1(E, x[..., 0], x[..., 1], x[..., 2])
    with np.errstate(all="ignore"):
        u = (fx * X + cx * z) / z
        v = (fy * Y + cy * z) / z
    return u, v, z


def sample(image, u, v):
    """Open3D's FloatValueAt on a float32 (H, W) image -> within, d (d is meaningless where not within)"""
    a = np.asarray(image, np.float32)
    H, W = a.shape
    assert W >= 2 and H >= 2
    with np.errstate(invalid="ignore"):
        within = (u >= 0.0) & (u <= float(W - 1)) & (v >= 0.0) & (v <= float(H - 1))
    us, vs = np.where(within, u, 0.0), np.where(within, v, 0.0)
    ui = np.maximum(np.minimum(us.astype(np.int64), W - 2), 0)
    vi = np.maximum(np.minimum(vs.astype(np.int64), H - 2), 0)
    pu, pv = us - ui.astype(np.float64), vs - vi.astype(np.float64)
    a = a.astype(np.float64)
    a00, a01, a10, a11 = a[vi, ui], a[vi + 1, ui], a[vi, ui + 1], a[vi + 1, ui + 1]
    with np.errstate(invalid="ignore"):
        d = (a00 * (1.0 - pv) + a01 * pv) * (1.0 - pu) + (a10 * (1.0 - pv) + a11 * pv) * pu
    return within, d


def corner_keeps(image, u, v, z, mode, keep_outside, keep_unmeasured=False):
    within, d = sample(image, u, v)
    with np.errstate(invalid="ignore"):
        measured = within & (d > 0.0)
        hit = measured & (z >= d) if mode == "depth" else measured
    keep = hit | (~within & bool(keep_outside))
    if keep_unmeasured:
        keep = keep | (within & ~measured)
    return keep


def carve(idx, origin, v, image, intrinsic, extrinsic, mode="depth", keep_outside=False, keep_unmeasured=False):
    """survivors of ONE float32 (H, W) image: bool (M,), True = some corner keeps the voxel"""
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    if len(idx) == 0:
        return np.zeros(0, bool)
    u, w, z = project(corners(idx, origin, v), intrinsic, extrinsic)
    return corner_keeps(image, u, w, z, mode, keep_outside, keep_unmeasured).any(1)


def carve_all(idx, origin, v, images, intrinsic, extrinsics, mode="depth", keep_outside=False, keep_unmeasured=False):
    """survivors of every image, as an index array into idx"""
    alive = np.ones(len(idx), bool)
    for im, E in zip(images, extrinsics):
        alive &= carve(idx, origin, v, im, intrinsic, E, mode, keep_outside, keep_unmeasured)
    return np.flatnonzero(alive)


def mask_from_u8(mask):
    """a uint8 / bool mask read as 0 / 1"""
    return (np.asarray(mask) != 0).astype(np.float32)


# ---- inclusion and bounds --------------------------------------------------------------------------------------------------------------
def included(idx, origin, v, queries):
    f = cell(queries, origin, v)
    ok = in_range(f)
    out = np.zeros(len(f), bool)
    have = set(keys_of(idx).tolist())
    k = keys_of(f[ok].astype(np.int64))
    out[np.flatnonzero(ok)] = [int(t) in have for t in k]
    return out


def bounds(idx, origin, v):
    origin = np.asarray(origin, np.float64).reshape(3)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    if len(idx) == 0:
        return origin.copy(), origin.copy()
    return origin + idx.min(0).astype(np.float64) * float(v), origin + (idx.max(0).astype(np.float64) + 1.0) * float(v)

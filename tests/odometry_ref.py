"""Host reference for the image operators and the RGB-D odometry (kpx_odometry.hip): a NumPy restatement of arithmetic contract AC11
(DESIGN.md 3), itself a recollection of Open3D's Image.cpp, Odometry.cpp and RGBDOdometryJacobian.cpp.  This file is the pinned
statement of the semantics: if a comparison with a real Open3D finds a difference, this file and kpx_odometry.hip change together.

Everything a DECISION depends on (filters, pyramids, the intensity normalisation, correspondences) is restated operation for operation
-- float64 from plain multiplies and adds in the kernel's order, float32 where the kernel rounds -- and is compared bit for bit.  The
27 sums of an iteration are formed here in correspondence order and on the device by a fixed tree: they, and the poses that follow
from them, agree within the spread this file shows over permuted orders.

  filters     separable, horizontal pass then vertical pass, border pixel repeated, fp64 accumulation over the taps in ascending
              order, one rounding to float32 per pass
  pyramid     level i = 2 x 2 mean (float32 (((a + b) + c) + d) / 4) of level i - 1, Gaussian3-filtered first when asked
  preprocess  depth < depth_min, > depth_max or <= 0 -> NaN; Gaussian3 on intensity and depth; each intensity image times 0.5 / (mean
              over the full-resolution correspondences at odo_init), the means from 128-bit fixed-point sums (order-free)
  correspond  q = d (K R K^-1)(u, v, 1) + K t, z' = q_z > 0, (u_t, v_t) = trunc(q_xy / z' + 0.5) inside, target depth finite,
              |z' - d_t| <= depth_diff_max; per target pixel the smallest float32(z'), then the smallest source index
  iteration   rows of the colour / hybrid term, J^T J x = -J^T r by LDL^T with the rank test 1e-12, T <- [Rz Ry Rx | t](x) T
  result      information matrix from the full-resolution correspondences at the final pose
"""
import numpy as np

from fgr_ref import euler_update, fixed_sum, solve6_ldlt_ranked

GAUSSIAN3, GAUSSIAN5, GAUSSIAN7, SOBEL3DX, SOBEL3DY = range(5)
_G3 = [0.25, 0.5, 0.25]
_G5 = [0.0625, 0.25, 0.375, 0.25, 0.0625]
_G7 = [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]
_DIFF = [-1.0, 0.0, 1.0]
_SMOOTH = [1.0, 2.0, 1.0]
TAPS = {GAUSSIAN3: (_G3, _G3), GAUSSIAN5: (_G5, _G5), GAUSSIAN7: (_G7, _G7), SOBEL3DX: (_DIFF, _SMOOTH), SOBEL3DY: (_SMOOTH, _DIFF)}   # (along x, along y)
LAMBDA = 0.968
SOBEL_SCALE = 0.125
COLOR, HYBRID = 0, 1


class Option:
    def __init__(self, iterations=(20, 10, 5), depth_diff_max=0.03, depth_min=0.0, depth_max=4.0):
        self.iterations, self.depth_diff_max, self.depth_min, self.depth_max = list(iterations), depth_diff_max, depth_min, depth_max


class Margins:
    """the two decision margins over every correspondence search made while it is passed along"""

    def __init__(self):
        self.rounding, self.depth_diff = np.inf, np.inf


# ---- image operators ---------------------------------------------------------------------------------------------------------------
def filter_pass(img, taps, horizontal):
    a = np.asarray(img, dtype=np.float32).astype(np.float64)
    n = a.shape[1] if horizontal else a.shape[0]
    acc = np.zeros_like(a)
    with np.errstate(invalid="ignore"):
        for k, w in enumerate(taps):
            idx = np.clip(np.arange(n) + k - len(taps) // 2, 0, n - 1)
            acc = acc + (a[:, idx] if horizontal else a[idx, :]) * w
        return acc.astype(np.float32)


def image_filter(img, kind):
    tx, ty = TAPS[kind]
    return filter_pass(filter_pass(img, tx, True), ty, False)


def downsample(img):
    a = np.asarray(img, dtype=np.float32)
    h2, w2 = a.shape[0] // 2, a.shape[1] // 2
    a = a[:2 * h2, :2 * w2]
    with np.errstate(invalid="ignore"):
        return (((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2]) + a[1::2, 1::2]) / np.float32(4.0)


def create_pyramid(img, levels, with_gaussian_filter=True):
    out = [np.asarray(img, dtype=np.float32)]
    for _ in range(1, levels):
        out.append(downsample(image_filter(out[-1], GAUSSIAN3) if with_gaussian_filter else out[-1]))
    return out


def filter_pyramid(pyramid, kind):
    return [image_filter(p, kind) for p in pyramid]


def preprocess_depth(depth, opt):
    d = np.array(depth, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        d[(d.astype(np.float64) < opt.depth_min) | (d.astype(np.float64) > opt.depth_max) | (d <= 0)] = np.nan
    return d


# ---- correspondences ---------------------------------------------------------------------------------------------------------------
def _mat3_mul(a, b):
    return [[(a[i][0] * b[0][k] + a[i][1] * b[1][k]) + a[i][2] * b[2][k] for k in range(3)] for i in range(3)]


def projection(K4, T):
    """M = (K R) K^-1 and K t with c_ij = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j, as the kernel's thread 0 forms them"""
    fx, fy, cx, cy = (float(x) for x in K4)
    T = np.asarray(T, dtype=np.float64)
    K = [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]
    Ki = [[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]]
    R = [[float(T[i, k]) for k in range(3)] for i in range(3)]
    M = _mat3_mul(_mat3_mul(K, R), Ki)
    Kt = [(K[i][0] * float(T[0, 3]) + K[i][1] * float(T[1, 3])) + K[i][2] * float(T[2, 3]) for i in range(3)]
    return M, Kt


def correspondence(K4, T, depth_s, depth_t, depth_diff_max, margins=None):
    """-> int32 (n, 4) rows (u_s, v_s, u_t, v_t), ascending in (v_t, u_t)"""
    Ds, Dt = np.asarray(depth_s, dtype=np.float32), np.asarray(depth_t, dtype=np.float32)
    H, W = Ds.shape
    M, Kt = projection(K4, T)
    v, u = (a.astype(np.float64) for a in np.mgrid[0:H, 0:W])
    d = Ds.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = [d * ((M[i][0] * u + M[i][1] * v) + M[i][2]) + Kt[i] for i in range(3)]
        valid = np.isfinite(Ds) & (q[2] > 0.0)
        fu, fv = q[0] / q[2] + 0.5, q[1] / q[2] + 0.5
        inside = valid & (fu > -1.0) & (fu < W) & (fv > -1.0) & (fv < H)
        ut = np.where(inside, np.trunc(np.where(inside, fu, 0.0)), 0).astype(np.int64)
        vt = np.where(inside, np.trunc(np.where(inside, fv, 0.0)), 0).astype(np.int64)
        dt = Dt[vt, ut]
        cand = inside & np.isfinite(dt)
        diff = np.abs(q[2] - dt.astype(np.float64))
        ok = cand & (diff <= depth_diff_max)
        if margins is not None:
            near = valid & np.isfinite(fu) & np.isfinite(fv) & (fu > -2.0) & (fu < W + 1.0) & (fv > -2.0) & (fv < H + 1.0)
            if near.any():
                margins.rounding = min(margins.rounding, float(np.abs(fu[near] - np.rint(fu[near])).min()), float(np.abs(fv[near] - np.rint(fv[near])).min()))
            if cand.any():
                margins.depth_diff = min(margins.depth_diff, float(np.abs(diff[cand] - depth_diff_max).min()))
    spx = np.flatnonzero(ok.reshape(-1))
    tpx = (vt.reshape(-1)[spx] * W + ut.reshape(-1)[spx])
    zf = q[2].reshape(-1)[spx].astype(np.float32).view(np.uint32).astype(np.uint64)
    keys = (zf << np.uint64(32)) | spx.astype(np.uint64)
    best = np.full(H * W, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(best, tpx, keys)
    t = np.flatnonzero(best != np.iinfo(np.uint64).max)
    s = (best[t] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.stack([s % W, s // W, t % W, t // W], 1).astype(np.int32)


def correspondence_brute(K4, T, depth_s, depth_t, depth_diff_max):
    """the same set by a plain loop and a sort by (target, float32 z', source): written differently on purpose"""
    Ds, Dt = np.asarray(depth_s, dtype=np.float32), np.asarray(depth_t, dtype=np.float32)
    H, W = Ds.shape
    M, Kt = projection(K4, T)
    cands = []
    for vs in range(H):
        for us in range(W):
            d = float(Ds[vs, us])
            if not np.isfinite(d):
                continue
            q = [d * ((M[i][0] * us + M[i][1] * vs) + M[i][2]) + Kt[i] for i in range(3)]
            if not q[2] > 0.0:
                continue
            fu, fv = q[0] / q[2] + 0.5, q[1] / q[2] + 0.5
            if not (np.isfinite(fu) and np.isfinite(fv)) or abs(fu) > 1e9 or abs(fv) > 1e9:
                continue
            ut, vt = int(fu), int(fv)                    # int() truncates towards zero, like the C cast
            if not (0 <= ut < W and 0 <= vt < H) or fu <= -1.0 or fv <= -1.0:
                continue
            dt = float(Dt[vt, ut])
            if not np.isfinite(dt) or not abs(q[2] - dt) <= depth_diff_max:
                continue
            cands.append((vt * W + ut, float(np.float32(q[2])), vs * W + us))
    cands.sort()
    rows, seen = [], set()
    for t, _, s in cands:
        if t not in seen:
            seen.add(t)
            rows.append((s % W, s // W, t % W, t // W))
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


# ---- one iteration -----------------------------------------------------------------------------------------------------------------
def _rows(J, r, w):
    """(n, 28): upper triangle of (w J)^T (w J) by rows, (w J)^T (w r), (w r)^2 per correspondence"""
    Jw = [w * j for j in J]
    rw = w * r
    cols = [Jw[i] * Jw[c] for i in range(6) for c in range(i, 6)] + [Jw[i] * rw for i in range(6)] + [rw * rw]
    return np.stack(cols, 1)


def _xyz(u, v, z, K4):
    fx, fy, cx, cy = (float(x) for x in K4)
    return ((u.astype(np.float64) - cx) * z) / fx, ((v.astype(np.float64) - cy) * z) / fy, z


def _grad(img, vt, ut):
    g = np.asarray(img, dtype=np.float32)[vt, ut]
    return np.where(np.isfinite(g), SOBEL_SCALE * g.astype(np.float64), 0.0)


def iteration(Is, Ds, It, Dt, dIx, dIy, dDx, dDy, K4, T, jacobian, depth_diff_max, perm_seed=None, margins=None):
    """-> sums (28,), count, solved, T_new (the given T when not solved)"""
    T = np.asarray(T, dtype=np.float64)
    fx, fy = float(K4[0]), float(K4[1])
    c = correspondence(K4, T, Ds, Dt, depth_diff_max, margins)
    if perm_seed is not None:
        c = c[np.random.default_rng(perm_seed).permutation(len(c))]
    if len(c) == 0:
        return np.zeros(28), 0, False, T
    us, vs, ut, vt = (c[:, k].astype(np.int64) for k in range(4))
    x, y, z = _xyz(us, vs, np.asarray(Ds, dtype=np.float32)[vs, us].astype(np.float64), K4)
    p = [((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)]
    invz = 1.0 / p[2]
    c0, c1 = (_grad(dIx, vt, ut) * fx) * invz, (_grad(dIy, vt, ut) * fy) * invz
    c2 = (-(c0 * p[0] + c1 * p[1])) * invz
    rp = np.asarray(It, dtype=np.float32)[vt, ut].astype(np.float64) - np.asarray(Is, dtype=np.float32)[vs, us].astype(np.float64)
    Jp = [-p[2] * c1 + p[1] * c2, p[2] * c0 - p[0] * c2, -p[1] * c0 + p[0] * c1, c0, c1, c2]
    if jacobian == COLOR:
        rows = _rows(Jp, rp, 1.0)
    else:
        d0, d1 = (_grad(dDx, vt, ut) * fx) * invz, (_grad(dDy, vt, ut) * fy) * invz
        d2 = (-(d0 * p[0] + d1 * p[1])) * invz
        rg = np.asarray(Dt, dtype=np.float32)[vt, ut].astype(np.float64) - p[2]
        Jg = [(-p[2] * d1 + p[1] * d2) - p[1], (p[2] * d0 - p[0] * d2) + p[0], -p[1] * d0 + p[0] * d1, d0, d1, d2 - 1.0]
        rows = _rows(Jp, rp, float(np.sqrt(1.0 - LAMBDA))) + _rows(Jg, rg, float(np.sqrt(LAMBDA)))
    sums = np.add.reduce(rows, axis=0)
    if not np.all(np.isfinite(sums)):
        return sums, len(c), False, T
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(sums[k])
            k += 1
    xs = solve6_ldlt_ranked(A, [-float(s) for s in sums[21:27]])
    if xs is None:
        return sums, len(c), False, T
    U = euler_update(xs)
    Tn = np.eye(4)
    for i in range(3):
        for j in range(4):
            a = (U[i, 0] * T[0, j] + U[i, 1] * T[1, j]) + U[i, 2] * T[2, j]
            Tn[i, j] = a + U[i, 3] if j == 3 else a
    return sums, len(c), True, Tn


def information(K4, T, Ds, Dt, depth_diff_max, perm_seed=None, margins=None):
    c = correspondence(K4, T, Ds, Dt, depth_diff_max, margins)
    if perm_seed is not None:
        c = c[np.random.default_rng(perm_seed).permutation(len(c))]
    G = np.zeros((6, 6))
    if len(c):
        ut, vt = c[:, 2].astype(np.int64), c[:, 3].astype(np.int64)
        x, y, z = _xyz(ut, vt, np.asarray(Dt, dtype=np.float32)[vt, ut].astype(np.float64), K4)
        o, l = np.zeros_like(x), np.ones_like(x)
        rows = _rows([o, z, -y, l, o, o], o, 1.0) + _rows([-z, o, x, o, l, o], o, 1.0) + _rows([y, -x, o, o, o, l], o, 1.0)
        sums = np.add.reduce(rows, axis=0)
        k = 0
        for i in range(6):
            for j in range(i, 6):
                G[i, j] = G[j, i] = sums[k]
                k += 1
    return G, len(c)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def level_camera(K4, level):
    return tuple(float(x) / float(1 << level) for x in K4)


def prepare(color_s, depth_s, color_t, depth_t, K4, odo_init, opt, margins=None):
    """-> per level (Is, Ds, It, Dt, dIx, dIy, dDx, dDy): the preprocessed, normalised pyramids and the target's Sobel pyramids"""
    Is, It = image_filter(color_s, GAUSSIAN3), image_filter(color_t, GAUSSIAN3)
    Ds, Dt = image_filter(preprocess_depth(depth_s, opt), GAUSSIAN3), image_filter(preprocess_depth(depth_t, opt), GAUSSIAN3)
    c = correspondence(K4, odo_init, Ds, Dt, opt.depth_diff_max, margins)
    if len(c):
        ms = fixed_sum(Is[c[:, 1], c[:, 0]]) / float(len(c))
        mt = fixed_sum(It[c[:, 3], c[:, 2]]) / float(len(c))
        if ms > 0.0 and mt > 0.0:
            Is = (Is.astype(np.float64) * (0.5 / ms)).astype(np.float32)
            It = (It.astype(np.float64) * (0.5 / mt)).astype(np.float32)
    n = len(opt.iterations)
    pIs, pIt = create_pyramid(Is, n, True), create_pyramid(It, n, True)
    pDs, pDt = create_pyramid(Ds, n, False), create_pyramid(Dt, n, False)
    return [(pIs[l], pDs[l], pIt[l], pDt[l], image_filter(pIt[l], SOBEL3DX), image_filter(pIt[l], SOBEL3DY), image_filter(pDt[l], SOBEL3DX),
             image_filter(pDt[l], SOBEL3DY)) for l in range(n)]


def odometry(color_s, depth_s, color_t, depth_t, K4, odo_init=None, jacobian=HYBRID, opt=None, perm_seed=None, margins=None):
    """compute_rgbd_odometry on float32 intensity / depth images -> (success, T (4, 4), information (6, 6))"""
    opt = Option() if opt is None else opt
    T = np.eye(4) if odo_init is None else np.array(odo_init, dtype=np.float64)
    levels = prepare(color_s, depth_s, color_t, depth_t, K4, T, opt, margins)
    n, step = len(levels), 0
    for l in range(n - 1, -1, -1):
        Kl = level_camera(K4, l)
        for _ in range(opt.iterations[n - 1 - l]):
            step += 1
            _, _, solved, T = iteration(*levels[l], Kl, T, jacobian, opt.depth_diff_max, None if perm_seed is None else perm_seed + step, margins)
            if not solved:
                return False, np.eye(4), np.eye(6)
    G, _ = information(K4, T, levels[0][1], levels[0][3], opt.depth_diff_max, None if perm_seed is None else perm_seed + step + 1, margins)
    return True, T, G


def sums_difference(a, b):
    """largest |difference| of two sets of sums relative to the largest |entry| of the second (1 when that is 0)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = float(np.abs(b).max()) if b.size else 0.0
    return float(np.abs(a - b).max() / (m if m > 0 else 1.0)) if b.size else 0.0

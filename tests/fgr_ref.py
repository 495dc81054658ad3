"""Host reference for Fast Global Registration (Zhou, Park, Koltun 2016): a float64 NumPy restatement of Open3D's
FastGlobalRegistration.cpp as include/kinectpx.h and DESIGN.md 5.10 state it.  This file is the pinned statement of the semantics:
if a comparison with a real Open3D finds a difference, this file and kpx_fgr.hip change together.

Stages (all on the float32-rounded coordinates, arithmetic in float64, no fused multiply-add):
  tuple_test   100 nc trials; trial t draws three correspondences with replacement from Philox-4x32-10, counter (0, t, 2, 0), key =
               the 64-bit seed, pick_q = (out[q] * nc) >> 32; it passes when l_k * tuple_scale < m_k < l_k / tuple_scale for the edges
               0-1, 1-2, 2-0 (l on the source, m on the target; strict); the first maximum_tuple_count passing trials, in trial order,
               give their three pairs each.
  normalise    the means of the WHOLE clouds (128-bit fixed-point sums as kpx_fixed.h: order-free), scale = the largest |p - mean|
               over both clouds; use_absolute_scale: scale_global = 1, par0 = scale, else scale_global = scale, par0 = 1.  A scale that is
               not positive (every point on its mean) is taken as 1 with par0 = 1.
  optimise     T = I; per round the 16 distinct sums of the weighted 6x6 system (weight s = (par / (r.r + par))^2), LDL^T with the
               rank test |D_j| > 1e-12 |A_jj| (solve6_ldlt_ranked), delta = [Rz(x2) Ry(x1) Rx(x0) | x3..5], T = delta T; a failed
               solve gives delta = I; then par /= division_factor if decrease_mu, itr % 4 == 0 and par > maximum_correspondence_distance.
  result       T maps target -> source in normalised coordinates; t' = -R m_t + t scale_global + m_s; the rigid inverse is returned.
               No correspondence or iteration_number == 0: the identity.
"""
import numpy as np

BATCH = 32768                 # kFgrBatch: trials per launch (the output does not depend on it)
TRIALS_PER_CORRES = 100
RANK_TOL = 1e-12              # kFgrRankTol
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on arrays of counters -> four uint64 arrays holding 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def tuple_picks(nc, seed, t0, t1):
    """the three correspondence indices of trials t0 .. t1 - 1 -> int64 (t1 - t0, 3)"""
    t = np.arange(t0, t1, dtype=np.uint64)
    out = philox4x32_10(0, t, 2, 0, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return np.stack([(out[q] * np.uint64(nc)) >> np.uint64(32) for q in range(3)], 1).astype(np.int64)


def _edge(p, u, v):
    d = p[:, u] - p[:, v]
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def tuple_flags(src, tgt, corres, tuple_scale, seed, t0, t1):
    """pass flag and picks of trials t0 .. t1 - 1"""
    s = np.asarray(src, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    g = np.asarray(tgt, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    corres = np.asarray(corres).reshape(-1, 2)
    picks = tuple_picks(len(corres), seed, t0, t1)
    sp, tp = s[corres[picks, 0]], g[corres[picks, 1]]             # (trials, 3, 3)
    ok = np.ones(len(picks), dtype=bool)
    for u, v in ((0, 1), (1, 2), (2, 0)):
        l, m = _edge(sp, u, v), _edge(tp, u, v)
        ok &= (l * tuple_scale < m) & (m < l / tuple_scale)
    return ok, picks


def tuple_test(src, tgt, corres, tuple_scale=0.95, maximum_tuple_count=1000, seed=0, batch=BATCH):
    """-> int32 (3 K, 2): the pairs of the first maximum_tuple_count passing trials.  `batch` only bounds the memory of a step."""
    corres = np.asarray(corres, dtype=np.int32).reshape(-1, 2)
    nc, out, found = len(corres), [], 0
    for t0 in range(0, TRIALS_PER_CORRES * nc, batch):
        if found >= maximum_tuple_count:
            break
        ok, picks = tuple_flags(src, tgt, corres, tuple_scale, seed, t0, min(t0 + batch, TRIALS_PER_CORRES * nc))
        take = picks[ok][:maximum_tuple_count - found]
        out.append(corres[take.reshape(-1)])
        found += len(take)
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 2), np.int32)


def fixed_sum(v):
    """sum of a float32 array as kpx_fixed.h forms it: every value truncated towards zero at 2^-64, added as integers, the 128-bit
    total converted as (double)hi + (double)lo * 2^-64 on the magnitude"""
    scaled = np.asarray(v, dtype=np.float32).astype(np.float64) * 2.0 ** 64          # a power of two: exact
    tot = sum(int(x) for x in scaled.tolist())                                    # int() truncates towards zero
    mag = abs(tot)
    val = float(mag >> 64) + float(mag & ((1 << 64) - 1)) * 2.0 ** -64
    return -val if tot < 0 else val


def normalise(src, tgt, use_absolute_scale=False):
    """-> m_s, m_t, scale, scale_global, par0"""
    s = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    g = np.asarray(tgt, dtype=np.float32).reshape(-1, 3)
    ms = np.array([fixed_sum(s[:, a]) / float(len(s)) for a in range(3)])
    mt = np.array([fixed_sum(g[:, a]) / float(len(g)) for a in range(3)])
    d2max = 0.0
    for p, m in ((s, ms), (g, mt)):
        d = p.astype(np.float64) - m
        d2max = max(d2max, float((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).max()))
    scale = float(np.sqrt(d2max))
    flat = not scale > 0.0
    return ms, mt, scale, (1.0 if use_absolute_scale or flat else scale), (scale if use_absolute_scale and not flat else 1.0)


def solve6_ldlt_ranked(A, b, rel=RANK_TOL):
    """kpx_linalg.h's LDL^T, operation for operation; None when a pivot fails |D_j| > 1e-300 or |D_j| > rel |A_jj|"""
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k] * D[k]
        D[j] = d
        if not abs(d) > 1e-300 or not abs(d) > rel * abs(A[j][j]):
            return None
        L[j][j] = 1.0
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v -= L[i][k] * L[j][k] * D[k]
            L[i][j] = v / d
    y = [0.0] * 6
    for i in range(6):
        v = b[i]
        for k in range(i):
            v -= L[i][k] * y[k]
        y[i] = v
    y = [y[i] / D[i] for i in range(6)]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k][i] * x[k]
        x[i] = v
    return x


def euler_update(x):
    """[Rz(x2) Ry(x1) Rx(x0) | x3..5] as a 4x4"""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3]],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def round_system(P, Q, T, par):
    """the 6x6 system of one round from the normalised points P (source) and Q (target) of the correspondences -> A (6, 6), b (6)"""
    qx = T[0, 0] * Q[:, 0] + T[0, 1] * Q[:, 1] + T[0, 2] * Q[:, 2] + T[0, 3]
    qy = T[1, 0] * Q[:, 0] + T[1, 1] * Q[:, 1] + T[1, 2] * Q[:, 2] + T[1, 3]
    qz = T[2, 0] * Q[:, 0] + T[2, 1] * Q[:, 1] + T[2, 2] * Q[:, 2] + T[2, 3]
    rx, ry, rz = P[:, 0] - qx, P[:, 1] - qy, P[:, 2] - qz
    w = par / (rx * rx + ry * ry + rz * rz + par)
    s = w * w
    S = [float(np.sum(v)) for v in (
        s * (qy * qy + qz * qz), s * (qx * qx + qz * qz), s * (qx * qx + qy * qy), s * (qx * qy), s * (qx * qz), s * (qy * qz),
        s * qx, s * qy, s * qz, s,
        s * (qz * ry - qy * rz), s * (qx * rz - qz * rx), s * (qy * rx - qx * ry), s * rx, s * ry, s * rz)]
    # J^T J = sum s J^T J over the rows (0, -qz, qy, -1, 0, 0), (qz, 0, -qx, 0, -1, 0), (-qy, qx, 0, 0, 0, -1); J^T r with r_x, r_y, r_z
    A = [[S[0], -S[3], -S[4], 0.0, -S[8], S[7]],
         [-S[3], S[1], -S[5], S[8], 0.0, -S[6]],
         [-S[4], -S[5], S[2], -S[7], S[6], 0.0],
         [0.0, S[8], -S[7], S[9], 0.0, 0.0],
         [-S[8], 0.0, S[6], 0.0, S[9], 0.0],
         [S[7], -S[6], 0.0, 0.0, 0.0, S[9]]]
    b = [-S[10], -S[11], -S[12], S[13], S[14], S[15]]
    return A, b


def optimize(src, tgt, corres, division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
             iteration_number=64):
    """-> dict(transformation (source -> target, the clouds' units), par, iterations, failed_solves, scale)"""
    s = np.asarray(src, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    g = np.asarray(tgt, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    corres = np.asarray(corres).reshape(-1, 2)
    if len(s) == 0 or len(g) == 0:
        return {"transformation": np.eye(4), "par": 1.0, "iterations": 0, "failed_solves": 0, "scale": 0.0}
    ms, mt, scale, sg, par = normalise(src, tgt, use_absolute_scale)
    rounds = iteration_number if len(corres) else 0
    P = (s[corres[:, 0]] - ms) / sg
    Q = (g[corres[:, 1]] - mt) / sg
    T, failed = np.eye(4), 0
    for itr in range(rounds):
        A, b = round_system(P, Q, T, par)
        x = solve6_ldlt_ranked(A, b)
        if x is None:
            failed += 1
        else:
            T = euler_update(x) @ T
            T[3] = [0.0, 0.0, 0.0, 1.0]
        if decrease_mu and itr % 4 == 0 and par > maximum_correspondence_distance:
            par = par / division_factor
    out = np.eye(4)
    if rounds > 0:
        R, t = T[:3, :3], T[:3, 3]
        tp = -(R @ mt) + t * sg + ms
        out[:3, :3] = R.T
        out[:3, 3] = -(R.T @ tp)
    return {"transformation": out, "par": float(par), "iterations": rounds, "failed_solves": failed, "scale": scale}


def optimize_permuted(src, tgt, corres, perm_seed, **options):
    """the optimisation with the correspondences in a permuted order (the sums are then formed in another order)"""
    corres = np.asarray(corres).reshape(-1, 2)
    return optimize(src, tgt, corres[np.random.default_rng(perm_seed).permutation(len(corres))], **options)


def permutation_spread(src, tgt, corres, n_perm=4, **options):
    """reference result and the largest difference of T over n_perm permuted runs: rotation entries absolute, translation relative to
    the cloud scale -> (result, spread)"""
    r0 = optimize(src, tgt, corres, **options)
    spread = 0.0
    for k in range(n_perm):
        spread = max(spread, transform_difference(optimize_permuted(src, tgt, corres, 1000 + k, **options)["transformation"],
                                                  r0["transformation"], r0["scale"]))
    return r0, spread


def transform_difference(Ta, Tb, scale):
    """largest |difference| of the rotation entries and of the translation relative to `scale` (1 when the scale is not positive)"""
    d = np.abs(np.asarray(Ta) - np.asarray(Tb))
    return float(max(d[:3, :3].max(), d[:3, 3].max() / (scale if scale > 0 else 1.0)))


def fgr(src, tgt, corres, tuple_test_on=True, tuple_scale=0.95, maximum_tuple_count=1000, seed=0, **options):
    """mutual correspondences in, transformation out: tuple test (when on and there is a correspondence), then the optimisation"""
    if tuple_test_on and len(corres):
        corres = tuple_test(src, tgt, corres, tuple_scale, maximum_tuple_count, seed)
    return optimize(src, tgt, corres, **options), corres

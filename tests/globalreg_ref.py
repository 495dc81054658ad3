"""Float64 references and path bookkeeping for global registration (rows a11-a13: FPFH, 33-D feature matching, RANSAC).

The constants restate kpx_fpfh.hip's and must be moved with the library's:
    kRansacBatch = 32768 hypotheses per batch; kSpec = 64 survivors validated speculatively before the one read-back;
    kMaxValidate = 512 survivors per further validation chunk; kFnnCols = 128 target columns per feature_nn stage and 64 query
    rows per block; the column split rule min(cdiv(1024, row_blocks), stages, 16), stages dealt to the splits round-robin."""
import numpy as np

RANSAC_BATCH = 32768
SPEC = 64
MAX_VALIDATE = 512
FNN_COLS = 128
FNN_ROWS = 64
FNN_MAX_SPLITS = 16


def cdiv(a, b):
    return -(-a // b)


def fnn_splits(na, nb):
    """feature_nn_splits: column splits (gridDim.y) of a (na, nb) feature_nn launch"""
    row_blocks, stages = cdiv(max(na, 1), FNN_ROWS), cdiv(max(nb, 1), FNN_COLS)
    return max(1, min(cdiv(1024, row_blocks), stages, FNN_MAX_SPLITS))


def fnn_place(j, na, nb):
    """where target column j lands: (split, stage, lane group column j % 16, 16-column tile within the stage)"""
    stage = j // FNN_COLS
    return stage % fnn_splits(na, nb), stage, j % 16, (j % FNN_COLS) // 16


def argmin_ref(fa, fb):
    """1-NN in 33-D, ties to the lowest target index, with no rounding at all: for integer-valued features of small magnitude every
    partial sum is an integer below 2^53, so the float64 matrix product is exact in any order."""
    fa = np.asarray(fa, dtype=np.float64)
    fb = np.asarray(fb, dtype=np.float64)
    assert np.all(fa == np.round(fa)) and np.all(fb == np.round(fb)) and max(np.abs(fa).max(initial=0), np.abs(fb).max(initial=0)) < 2 ** 20
    nb2 = (fb * fb).sum(1)
    out = np.empty(len(fa), dtype=np.int32)
    for r0 in range(0, len(fa), 4096):
        a = fa[r0:r0 + 4096]
        d = (a * a).sum(1)[:, None] - 2.0 * (a @ fb.T) + nb2[None, :]
        out[r0:r0 + 4096] = np.argmin(d, 1)                   # first minimum: the lowest index among ties
    return out


def nn_dist_excess(fa, fb, idx):
    """float64 (direct differences) distance of the returned neighbour minus the float64 minimum, and the rounding bound of the
    K = 36 fma chain (|a|^2 + sum a_k (-2 b_k) + |b|^2, 36 roundings of terms no larger than (|a| + |b|)^2)"""
    fa = np.asarray(fa, dtype=np.float64)
    fb = np.asarray(fb, dtype=np.float64)
    exc, bound = np.empty(len(fa)), np.empty(len(fa))
    nb = np.sqrt((fb * fb).sum(1))
    for i in range(len(fa)):
        d = ((fb - fa[i]) ** 2).sum(1)
        exc[i] = d[idx[i]] - d.min()
        bound[i] = 2 * 40 * np.finfo(np.float64).eps * (np.linalg.norm(fa[i]) + nb.max()) ** 2
    return exc, bound


def ransac_chunk(k):
    """validation chunk of the in-batch survivor index k: 0 = the speculative chunk (kSpec), 1.. = the chunks of kMaxValidate"""
    return 0 if k < SPEC else 1 + (k - SPEC) // MAX_VALIDATE


# ---- FPFH: which pairs sit on a bin edge ---------------------------------------------------------------------------------
def pair_bins(p1, n1, p2, n2):
    """the three binned coordinates 11 (f0 + pi) / 2 pi, 11 (f1 + 1) / 2, 11 (f2 + 1) / 2 of Open3D's ComputePairFeatures, float64,
    vectorised over pairs (rows of p1, n1, p2, n2)"""
    p1, n1, p2, n2 = (np.asarray(x, dtype=np.float64) for x in (p1, n1, p2, n2))
    dp = p2 - p1
    f3 = np.sqrt((dp * dp).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        a1 = (n1 * dp).sum(1) / f3
        a2 = (n2 * dp).sum(1) / f3
    swap = np.abs(a1) < np.abs(a2)
    a = np.where(swap[:, None], n2, n1)
    b = np.where(swap[:, None], n1, n2)
    dp = np.where(swap[:, None], -dp, dp)
    f2 = np.where(swap, -a2, a1)
    v = np.cross(dp, a)
    vn = np.sqrt((v * v).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = v / vn[:, None]
    w = np.cross(a, v)
    f1 = (v * b).sum(1)
    f0 = np.arctan2((w * b).sum(1), (a * b).sum(1))
    zero = (f3 == 0.0) | (vn == 0.0)
    f = np.stack([f0, f1, f2], 1)
    f[zero] = 0.0
    return np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) * 0.5, 11.0 * (f[:, 2] + 1.0) * 0.5], 1)


def fpfh_edge_flags(pts, nrm, nbr, cnt, tol=1e-12):
    """flags[i, f] = number of pairs (i, nbr[i, t]), t >= 1, whose binned coordinate of feature f lies within tol of an inner bin
    edge (1 .. 10; the outer edges clamp to the same bin on both sides).  nbr / cnt: the oracle's neighbour lists."""
    pts = np.asarray(pts, dtype=np.float32).astype(np.float64)
    nrm = np.asarray(nrm, dtype=np.float32).astype(np.float64)
    n, k = nbr.shape
    flags = np.zeros((n, 3), dtype=np.int64)
    ii, tt = np.nonzero((np.arange(k)[None, :] >= 1) & (np.arange(k)[None, :] < cnt[:, None]))
    if len(ii) == 0:
        return flags
    jj = nbr[ii, tt]
    x = pair_bins(pts[ii], nrm[ii], pts[jj], nrm[jj])
    e = np.round(x)
    near = (np.abs(x - e) <= tol * np.maximum(1.0, np.abs(x))) & (e >= 1) & (e <= 10)
    for f in range(3):
        np.add.at(flags[:, f], ii, near[:, f].astype(np.int64))
    return flags


def check_fpfh(got, want, flags, nbr, cnt, d2, rtol=1e-9):
    """got (GPU) against want (oracle): rows untouched by a flagged pair (neither the row's own pairs nor any weighted neighbour's)
    within rtol with no allowance; touched rows keep their per-feature sums, and each feature block differs (L1) by no more than one
    bin move of every flagged pair can cause.  Returns the number of touched rows; raises AssertionError otherwise."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    n, k = nbr.shape
    assert got.shape == want.shape == (n, 33)
    inc = np.where(cnt > 1, 100.0 / np.maximum(cnt - 1, 1), 0.0)
    own = 2.0 * inc[:, None] * flags                              # L1 change of the row's SPFH block per feature
    bound = own.copy()
    touched = flags.sum(1) > 0
    for i in range(n):
        m = cnt[i]
        if m <= 1:
            continue
        j = nbr[i, 1:m]
        d = d2[i, 1:m]
        ok = d != 0.0
        j, d = j[ok], d[ok]
        if len(j) == 0:
            continue
        s = (100.0 * (cnt[j] > 1) / d).sum()
        if s == 0.0:
            continue
        bound[i] += ((100.0 / s) / d) @ own[j]                   # weighted neighbours' SPFH moves, after normalisation
        touched[i] |= bool(flags[j].sum() > 0)
    scale = np.abs(want).max(1, keepdims=True) + 1.0
    close = np.abs(got - want) <= rtol * scale
    bad = ~close.all(1)
    assert not np.any(bad & ~touched), "rows without a flagged pair differ: %s" % np.nonzero(bad & ~touched)[0][:10]
    gs, ws = got.reshape(n, 3, 11).sum(2), want.reshape(n, 3, 11).sum(2)
    assert np.allclose(gs, ws, rtol=rtol, atol=rtol), "per-feature sums differ"
    l1 = np.abs(got - want).reshape(n, 3, 11).sum(2)
    assert np.all(l1 <= bound * (1 + 1e-9) + rtol * scale), "a touched row differs by more than its flagged pairs allow"
    return int(touched.sum())


# ---- RANSAC: synthetic correspondence sets and the path a run takes --------------------------------------------------------
def _rot(ax, ang):
    ax = np.asarray(ax, dtype=np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


MOTION1 = np.eye(4)
MOTION1[:3, :3], MOTION1[:3, 3] = _rot([0.3, 1, 0.2], 0.4), [120, -40, 300]
MOTION2 = np.eye(4)
MOTION2[:3, :3], MOTION2[:3, 3] = _rot([1, 0.1, -0.3], -0.9), [-900, 500, 200]


def corres_scene(base, n, f1, f2, nc, seed):
    """source = n points of `base`; target = the source under MOTION1, followed by a tenth of the source under MOTION2 (a repetitive
    structure).  Correspondences: round(f1 nc) true pairs, round(f2 nc) pairs consistent under MOTION2, the rest random; shuffled.
    -> src, tgt (float32), corres (int32 (nc, 2))"""
    rng = np.random.default_rng(seed)
    src = base[rng.choice(len(base), n, replace=False)].astype(np.float32)
    G = rng.choice(n, max(n // 10, 1), replace=False)
    s64 = src.astype(np.float64)
    tgt = np.concatenate([s64 @ MOTION1[:3, :3].T + MOTION1[:3, 3], s64[G] @ MOTION2[:3, :3].T + MOTION2[:3, 3]]).astype(np.float32)
    k1, k2 = int(round(f1 * nc)), int(round(f2 * nc))
    a = rng.choice(n, k1, replace=False)
    b = rng.choice(len(G), k2, replace=k2 > len(G))
    r = np.stack([rng.integers(0, n, nc - k1 - k2), rng.integers(0, len(tgt), nc - k1 - k2)], 1)
    corr = np.concatenate([np.stack([a, a], 1), np.stack([G[b], n + b], 1), r]).astype(np.int32)
    return src, tgt, np.ascontiguousarray(corr[rng.permutation(len(corr))])


def ransac_path(O, src, tgt, corr, max_dist, max_iter, conf, seed):
    """The oracle's run and the path the product's batched loop takes for it.  Survivors of batch b (hypotheses that pass every
    checker) = the validations of confidence-1.0 runs (no exit) up to the batch's end, differenced.  The run stops at the in-batch
    survivor index `stop_k` of batch `stop_batch` (the first survivor at or beyond est_k; None: no survivor there, the batch loop
    ends on its own)."""
    T, st = O.ransac_corres(src, tgt, corr, max_dist, 3, 0.95, max_iter, conf, seed)
    I, V = st["iterations"], st["validations"]
    run = cdiv(I, RANSAC_BATCH) if I > 0 else 0
    surv, prev = [], 0
    for b in range(run):
        if conf == 1.0 and b == run - 1 and min(max_iter, RANSAC_BATCH * (b + 1)) == I:
            surv.append(V - prev)                                  # this run itself
            break
        _, s1 = O.ransac_corres(src, tgt, corr, max_dist, 3, 0.95, min(max_iter, RANSAC_BATCH * (b + 1)), 1.0, seed)
        surv.append(s1["validations"] - prev)
        prev = s1["validations"]
    cum = np.cumsum(surv) if surv else np.zeros(0, dtype=np.int64)
    stop_batch = next((b for b in range(run) if cum[b] > V), None)
    stop_k = None if stop_batch is None else V - (int(cum[stop_batch - 1]) if stop_batch else 0)
    return T, st, dict(survivors=surv, exit=I < max_iter, stop_batch=stop_batch, stop_k=stop_k,
                       stop_chunk=None if stop_k is None else ransac_chunk(stop_k))

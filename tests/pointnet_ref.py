"""Reference statements of the PointNet joint regressor (AC18), independent of the library:
  - the UNFOLDED network in float64 (NumPy, and torch CPU with conv1d / batch_norm / linear / bmm),
  - the folded network (batch normalisation folded into the layer in front of it) evaluated in float64 -- the reference every float32
    result is judged against -- and in float32 in several summation orders: NumPy as given, random consistent permutations of every
    hidden channel axis (the same function, another order), torch CPU,
  - the deviation rule: tau = 4 x the worst float32 restatement's deviation from the float64 evaluation, relative to the array's scale.
Layer numbering as in include/kinectpx.h: 0..5 tnet(3), 6..7, 8..13 tnet(32), 14..19."""
import functools

import numpy as np

EPS = 1e-3                         # Keras' BatchNormalization default
MARGIN = 4.0
N_PERMUTATIONS = 5
STAGES = ("T3", "T32", "g1", "g2", "g3", "joints")


def layer_shapes(J):
    """(c_in, c_out, has batch normalisation, is a Conv1D) in network order"""
    tnet = lambda f: [(f, 32, True, True), (32, 64, True, True), (64, 512, True, True), (512, 256, True, False), (256, 128, True, False),
                      (128, f * f, False, False)]
    return tnet(3) + [(3, 32, True, True), (32, 32, True, True)] + tnet(32) + [(32, 32, True, True), (32, 64, True, True), (64, 512, True, True),
                                                                              (512, 256, True, False), (256, 128, True, False), (128, 3 * J, False, False)]


def make_weights(J, seed):
    """seeded stand-ins for trained weights in Keras' get_weights() order (108 arrays): Glorot-uniform kernels, biases / beta / mean ~ N(0,
    0.1), gamma / variance ~ U(0.5, 1.5); the T-nets' last Dense gets a N(0, 0.02) kernel and the identity bias (Keras' zero kernel would
    leave the T-nets unexercised)."""
    rng = np.random.default_rng(seed)
    w = []
    for l, (ci, co, bn, conv) in enumerate(layer_shapes(J)):
        shape = (1, ci, co) if conv else (ci, co)
        if l in (5, 13):
            f = int(round(np.sqrt(co)))
            w += [rng.normal(0, 0.02, shape).astype(np.float32), np.eye(f, dtype=np.float32).reshape(-1)]
            continue
        lim = np.sqrt(6.0 / (ci + co))
        w += [rng.uniform(-lim, lim, shape).astype(np.float32), rng.normal(0, 0.1, co).astype(np.float32)]
        if bn:
            w += [rng.uniform(0.5, 1.5, co).astype(np.float32), rng.normal(0, 0.1, co).astype(np.float32), rng.normal(0, 0.1, co).astype(np.float32),
                  rng.uniform(0.5, 1.5, co).astype(np.float32)]
    return w


def split_weights(weights):
    """108 arrays -> per layer a dict(K (c_in, c_out) f64, b, and gamma, beta, mean, var where the layer has batch normalisation)"""
    J = np.asarray(weights[-1]).size // 3
    out, i = [], 0
    for ci, co, bn, _ in layer_shapes(J):
        d = dict(K=np.asarray(weights[i], np.float64).reshape(ci, co), b=np.asarray(weights[i + 1], np.float64))
        if bn:
            d.update(gamma=np.asarray(weights[i + 2], np.float64), beta=np.asarray(weights[i + 3], np.float64), mean=np.asarray(weights[i + 4], np.float64),
                     var=np.asarray(weights[i + 5], np.float64))
        out.append(d)
        i += 6 if bn else 2
    assert i == len(weights) == 108
    return out


def fold(weights, eps=EPS, rounded=True):
    """s = gamma / sqrt(var + eps), W' = K s, b' = (b - mean) s + beta in float64; rounded: to float32 (the model), else left in float64"""
    out = []
    for d in split_weights(weights):
        W, b = d["K"], d["b"]
        if "gamma" in d:
            s = d["gamma"] / np.sqrt(d["var"] + eps)
            W, b = W * s, (b - d["mean"]) * s + d["beta"]
        out.append((W.astype(np.float32), b.astype(np.float32)) if rounded else (W, b))
    return out


def _relu(v):
    return np.maximum(v, 0)


def _stages(T3, T32, g1, g2, g3, y):
    return dict(T3=T3, T32=T32, g1=g1, g2=g2, g3=g3, joints=y)


def forward_unfolded(weights, x, eps=EPS):
    """the network as Keras builds it, layer by layer, in float64: relu(BN(x K + b)), BN on the moving statistics"""
    L = split_weights(weights)
    x = np.asarray(x, np.float64)
    B = x.shape[0]

    def block(h, d, act=True):
        y = h @ d["K"] + d["b"]
        if "gamma" in d:
            y = d["gamma"] * (y - d["mean"]) / np.sqrt(d["var"] + eps) + d["beta"]
        return _relu(y) if act else y

    def tnet(h, l0, f):
        a = block(block(block(h, L[l0]), L[l0 + 1]), L[l0 + 2])
        g = a.max(axis=1)
        t = block(block(block(g, L[l0 + 3]), L[l0 + 4]), L[l0 + 5], act=False)
        return g, t.reshape(B, f, f)

    g1, T3 = tnet(x, 0, 3)
    f = block(block(np.einsum("bnk,bkj->bnj", x, T3), L[6]), L[7])
    g2, T32 = tnet(f, 8, 32)
    a = block(block(block(np.einsum("bnk,bkj->bnj", f, T32), L[14]), L[15]), L[16])
    g3 = a.max(axis=1)
    y = block(block(block(g3, L[17]), L[18]), L[19], act=False)
    return _stages(T3, T32, g1, g2, g3, y)


_HIDDEN = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 18)          # layers whose output channels the next layer sums over


def forward_folded(folded, x, dtype=np.float64, perm_seed=None, transpose_T=False):
    """the folded network (y = relu(x W + b)) with every product and sum in `dtype`.  perm_seed: the output channels of every hidden layer,
    and the columns of T3 and T32, are permuted, with the rows of whatever consumes them -- the same function in another summation order;
    the stage outputs come back in natural order.  transpose_T: the T-net matrices applied transposed (a negative control)."""
    L = [(np.asarray(W, dtype), np.asarray(b, dtype)) for W, b in folded]
    x = np.asarray(x, dtype)
    B = x.shape[0]
    P = {}
    Pa, Pb = np.arange(3), np.arange(32)
    if perm_seed is not None:
        rng = np.random.default_rng(perm_seed)
        for l in _HIDDEN:
            P[l] = rng.permutation(L[l][0].shape[1])
            L[l] = (L[l][0][:, P[l]], L[l][1][P[l]])
            L[l + 1] = (L[l + 1][0][P[l], :], L[l + 1][1])
        Pa, Pb = rng.permutation(3), rng.permutation(32)
        L[6] = (L[6][0][Pa, :], L[6][1])
        L[14] = (L[14][0][Pb, :], L[14][1])
    P7 = P.get(7, np.arange(32))

    def dense(h, l, act=True):
        y = h @ L[l][0] + L[l][1]
        return _relu(y) if act else y

    def natural(g, l):
        if l not in P:
            return g
        out = np.empty_like(g)
        out[:, P[l]] = g
        return out

    def tnet(h, l0, f):
        a = dense(dense(dense(h, l0), l0 + 1), l0 + 2)
        g = a.max(axis=1)
        t = dense(dense(dense(g, l0 + 3), l0 + 4), l0 + 5, act=False)
        return natural(g, l0 + 2), t.reshape(B, f, f)

    use = (lambda T: T.transpose(0, 2, 1)) if transpose_T else (lambda T: T)
    g1, T3 = tnet(x, 0, 3)
    f = dense(dense(np.matmul(x, np.ascontiguousarray(use(T3)[:, :, Pa])), 6), 7)
    g2, T32 = tnet(f, 8, 32)
    a = dense(dense(dense(np.matmul(f, np.ascontiguousarray(use(T32)[:, P7, :][:, :, Pb])), 14), 15), 16)
    g3 = natural(a.max(axis=1), 16)
    y = dense(dense(dense(a.max(axis=1), 17), 18), 19, act=False)
    assert y.dtype == dtype
    return _stages(T3, T32, g1, g2, g3, y)


def forward_torch32(folded, x):
    """the folded network on torch CPU float32 (another library's kernels and summation order)"""
    import torch
    L = [(torch.from_numpy(np.asarray(W, np.float32)), torch.from_numpy(np.asarray(b, np.float32))) for W, b in folded]
    x = torch.from_numpy(np.array(x, np.float32))
    B = x.shape[0]
    dense = lambda h, l, act=True: torch.relu(torch.matmul(h, L[l][0]) + L[l][1]) if act else torch.matmul(h, L[l][0]) + L[l][1]

    def tnet(h, l0, f):
        g = dense(dense(dense(h, l0), l0 + 1), l0 + 2).amax(dim=1)
        return g, dense(dense(dense(g, l0 + 3), l0 + 4), l0 + 5, act=False).reshape(B, f, f)

    g1, T3 = tnet(x, 0, 3)
    f = dense(dense(torch.bmm(x, T3), 6), 7)
    g2, T32 = tnet(f, 8, 32)
    g3 = dense(dense(dense(torch.bmm(f, T32), 14), 15), 16).amax(dim=1)
    y = dense(dense(dense(g3, 17), 18), 19, act=False)
    return {k: v.numpy() for k, v in _stages(T3, T32, g1, g2, g3, y).items()}


def forward_torch64_unfolded(weights, x, eps=EPS):
    """the unfolded network on torch CPU float64 with the framework's own layers: conv1d, batch_norm(training=False), linear, bmm"""
    import torch
    import torch.nn.functional as F
    L = [{k: torch.from_numpy(v) for k, v in d.items()} for d in split_weights(weights)]
    x = torch.from_numpy(np.array(x, np.float64))
    B = x.shape[0]

    def bn(y, d):
        return F.batch_norm(y, d["mean"], d["var"], d["gamma"], d["beta"], training=False, eps=eps)

    def conv(h, d):                                   # h (B, C, N)
        return torch.relu(bn(F.conv1d(h, d["K"].t().unsqueeze(-1).contiguous(), d["b"]), d))

    def dense(h, d, act=True):
        y = F.linear(h, d["K"].t().contiguous(), d["b"])
        return torch.relu(bn(y, d)) if act else y

    def tnet(h, l0, f):
        g = conv(conv(conv(h, L[l0]), L[l0 + 1]), L[l0 + 2]).amax(dim=2)
        return g, dense(dense(dense(g, L[l0 + 3]), L[l0 + 4]), L[l0 + 5], act=False).reshape(B, f, f)

    g1, T3 = tnet(x.transpose(1, 2), 0, 3)
    f = conv(conv(torch.bmm(x, T3).transpose(1, 2), L[6]), L[7])
    g2, T32 = tnet(f, 8, 32)
    g3 = conv(conv(conv(torch.bmm(f.transpose(1, 2), T32).transpose(1, 2), L[14]), L[15]), L[16]).amax(dim=2)
    y = dense(dense(dense(g3, L[17]), L[18]), L[19], act=False)
    return {k: v.numpy() for k, v in _stages(T3, T32, g1, g2, g3, y).items()}


def restatements32(folded, x):
    """the float32 restatements: NumPy as given, N_PERMUTATIONS permuted orders, torch CPU"""
    outs = [forward_folded(folded, x, np.float32)]
    outs += [forward_folded(folded, x, np.float32, perm_seed=1000 + q) for q in range(N_PERMUTATIONS)]
    outs.append(forward_torch32(folded, x))
    return outs


def rel_dev(got, ref):
    """max |got - ref| / max |ref|; an all-zero ref: 0 when got is all zero too, else inf"""
    ref = np.asarray(ref, np.float64)
    err, scale = float(np.abs(np.asarray(got, np.float64) - ref).max()), float(np.abs(ref).max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def reference(folded, x):
    """-> (y64: the float64 evaluation per stage, tau per stage: MARGIN x the worst float32 restatement's rel_dev)"""
    y64 = forward_folded(folded, x, np.float64)
    outs = restatements32(folded, x)
    tau = {k: MARGIN * max(rel_dev(o[k], y64[k]) for o in outs) for k in STAGES}
    return y64, tau


# ---- test inputs ------------------------------------------------------------------------------------------------------------------------------
UNIT, MILLIMETRE = "unit", "millimetre"


def make_clouds(B, N, scale, seed):
    """B clouds of N points around a centre away from the origin: a body-sized blob in metres-like units (spread 0.3 around a centre at
    distance ~1.2) or in millimetres (spread 250 around (600, -400, 3000))"""
    rng = np.random.default_rng(seed)
    if scale == UNIT:
        c = np.array([0.6, -0.4, 1.0]) + rng.normal(0, 0.05, (B, 1, 3))
        return (c + rng.normal(0, 0.3, (B, N, 3))).astype(np.float32)
    c = np.array([600.0, -400.0, 3000.0]) + rng.normal(0, 50.0, (B, 1, 3))
    return (c + rng.normal(0, 250.0, (B, N, 3))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def model(J, seed=7):
    """(weights, folded) of the seeded test model for J joints, computed once"""
    w = make_weights(J, seed)
    return w, fold(w)


@functools.lru_cache(maxsize=None)
def case(B, N, J, scale, seed=0):
    """(x, y64, tau) of one test case, computed once and shared; the arrays must be left unchanged"""
    x = make_clouds(B, N, scale, 100 * seed + 7 * B + N)
    y64, tau = reference(model(J)[1], x)
    x.setflags(write=False)
    return x, y64, tau

"""The normative restatement of AC19: one training step of the reference's models/pointnet.py as model.fit runs it, on
torch CPU autograd, independent of the library.
  - step(): train-mode forward (batch statistics, biased variance, epsilon 1e-3), dropout by given keep masks, loss = mean squared error +
    (OrthogonalRegularizer(T3) + OrthogonalRegularizer(T32)) / B, gradients of the 74 trainable arrays; float64 or float32; `perm`
    evaluates the same function with the points of every cloud in another order (another summation order); `pool_index` forces the three
    max-pool selections (a gather instead of a maximum), because a float32 run may pick another point on a near tie and then moves a whole
    channel's gradient (measured: up to 7 % of a layer's scale at B = 16, N = 63).
  - the deviation rule of AC18 per LAYER: dev_l = max |g - g64| over the layer's trainable arrays / the largest |g64| among them;
    tau_l = 4 x the worst dev_l among the float32 restatements (as given, two point permutations), never measured on the device.
  - adam(): NumPy float64.  dropout_masks(): the host mirror of AC19's counter-based generator.
Keras behaviour restated from memory (no TensorFlow here): this file is the normative statement of it."""
import functools

import numpy as np
import torch

from tests import pointnet_ref as R

EPS = 1e-3
KEEP = 0.7
MARGIN = 4.0
BN_LAYERS = [l for l in range(20) if l not in (5, 13, 19)]
CAP = 2.0 ** -8                     # the input condition: a case whose float32 restatements wobble more than this per layer is not used


def _mix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    return x ^ (x >> 16)


def dropout_masks(seed, step, B):
    """keep masks (B, 256), (B, 128): keep iff (h >> 8) < floor(0.7 2^24), h = mix(mix(mix(mix(seed) ^ step) ^ layer) ^ (512 row + channel))"""
    out = []
    for layer, width in enumerate((256, 128)):
        base = _mix(_mix(_mix(seed & 0xFFFFFFFF) ^ (step & 0xFFFFFFFF)) ^ layer)
        m = np.empty((B, width), bool)
        for b in range(B):
            for c in range(width):
                m[b, c] = (_mix(base ^ ((512 * b + c) & 0xFFFFFFFF)) >> 8) < 11744051
        out.append(m)
    return out


def regulariser(t, f):
    """OrthogonalRegularizer.__call__ as the reference writes it"""
    x = t.reshape(-1, f, f)
    xxt = torch.tensordot(x, x, dims=([2], [2])).reshape(-1, f, f)
    return (0.001 * (xxt - torch.eye(f, dtype=t.dtype)) ** 2).sum()


def params_of(weights, dtype):
    """108 Keras arrays -> per layer dict K (c_in, c_out), b, and gamma, beta where the layer has batch normalisation, as leaf tensors"""
    out = []
    for d in R.split_weights(weights):
        out.append({k: torch.tensor(np.asarray(d[k], np.float64), dtype=dtype, requires_grad=True) for k in ("K", "b", "gamma", "beta") if k in d})
    return out


def step(weights, x, y, masks=None, pool_index=None, dtype=torch.float64, perm=None):
    """-> dict: loss, mse, reg (floats), grads (20 lists of float64 arrays: kernel, bias[, gamma, beta]), T3, T32, g1..g3, i1..i3, out,
    pre3 (the three (B, N, 512) activations in front of the pools, float64 runs without perm only), stats {layer: (mean, var)}"""
    P = params_of(weights, dtype)
    x = torch.tensor(np.asarray(x, np.float64), dtype=dtype)
    y = torch.tensor(np.asarray(y, np.float64), dtype=dtype)
    B, N = x.shape[0], x.shape[1]
    inv = None
    if perm is not None:
        perm = torch.as_tensor(np.asarray(perm))
        x = x[:, perm]
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(N)
    stats, pools, pre = {}, [], []

    def lay(h, l):
        p = P[l]
        z = h @ p["K"] + p["b"]
        if "gamma" not in p:
            return z
        ax = tuple(range(z.dim() - 1))
        m, v = z.mean(ax), z.var(ax, unbiased=False)
        stats[l] = (m.detach().double().numpy(), v.detach().double().numpy())
        return torch.relu(p["gamma"] * (z - m) / torch.sqrt(v + EPS) + p["beta"])

    def pool(h):
        pre.append(h)
        if pool_index is None:
            v, i = h.max(1)
        else:
            i = torch.as_tensor(np.asarray(pool_index[len(pools)], np.int64))
            if inv is not None:
                i = inv[i]
            v = torch.gather(h, 1, i[:, None, :]).squeeze(1)
        pools.append((v, i))
        return v

    def tnet(h, l0, f):
        a = lay(lay(lay(h, l0), l0 + 1), l0 + 2)
        t = lay(lay(lay(pool(a), l0 + 3), l0 + 4), l0 + 5)
        return torch.bmm(h, t.reshape(B, f, f)), t, regulariser(t, f)

    h, T3, r3 = tnet(x, 0, 3)
    h = lay(lay(h, 6), 7)
    h, T32, r32 = tnet(h, 8, 32)
    h = pool(lay(lay(lay(h, 14), 15), 16))
    h = lay(h, 17)
    if masks is not None:
        h = h * torch.tensor(masks[0], dtype=dtype) * (1.0 / KEEP)
    h = lay(h, 18)
    if masks is not None:
        h = h * torch.tensor(masks[1], dtype=dtype) * (1.0 / KEEP)
    out = lay(h, 19)
    mse = ((out - y) ** 2).mean()
    reg = (r3 + r32) / B
    loss = mse + reg
    flat = [p[k] for p in P for k in ("K", "b", "gamma", "beta") if k in p]
    g = torch.autograd.grad(loss, flat, allow_unused=True)
    grads, i = [], 0
    for p in P:
        grads.append([(g[i + q] if g[i + q] is not None else torch.zeros_like(flat[i + q])).double().numpy() for q in range(len(p))])
        i += len(p)
    res = dict(loss=float(loss.detach()), mse=float(mse.detach()), reg=float(reg.detach()), grads=grads, stats=stats, out=out.detach().double().numpy(),
               T3=T3.detach().double().numpy().reshape(B, 3, 3), T32=T32.detach().double().numpy().reshape(B, 32, 32))
    for q, (v, i) in enumerate(pools):
        res[f"g{q + 1}"], res[f"i{q + 1}"] = v.detach().double().numpy(), i.numpy()
    if perm is None and dtype == torch.float64:
        res["pre3"] = [h.detach().numpy() for h in pre]
    return res


def layer_dev(grads, grads64):
    """per layer: max |g - g64| over the layer's arrays / the largest |g64| among them (0 / 0 = 0)"""
    out = []
    for g, r in zip(grads, grads64):
        scale = max(float(np.abs(a).max()) for a in r)
        err = max(float(np.abs(np.asarray(a, np.float64) - b).max()) for a, b in zip(g, r))
        out.append(0.0 if err == 0.0 else (err / scale if scale > 0 else float("inf")))
    return out


def reference(weights, x, y, masks, pool_index):
    """-> (the float64 step with the given selections, tau per layer, tau of the loss: MARGIN x the float32 restatements' worst deviation)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)               # one summation order per restatement, whatever the machine's core count
    try:
        r64 = step(weights, x, y, masks, pool_index)
        N = np.asarray(x).shape[1]
        rng = np.random.default_rng(N)
        runs = [step(weights, x, y, masks, pool_index, torch.float32)]
        runs += [step(weights, x, y, masks, pool_index, torch.float32, perm=rng.permutation(N)) for _ in range(2)]
    finally:
        torch.set_num_threads(threads)
    tau = [MARGIN * max(d) for d in zip(*[layer_dev(r["grads"], r64["grads"]) for r in runs])]
    tau_loss = MARGIN * max(abs(r["loss"] - r64["loss"]) for r in runs) / abs(r64["loss"])
    return r64, tau, tau_loss


def adam(w, g, m, v, lr=0.001, b1=0.9, b2=0.999, eps=1e-7, t=1):
    """Keras' Adam in float64 -> (w, m, v)"""
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return w - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(v) + eps), m, v


# ---- test inputs --------------------------------------------------------------------------------------------------------------------------------
CASES = [(16, 1), (16, 63), (16, 64), (16, 65), (17, 130), (32, 200)]
SMALL = [(1, 70), (2, 65), (5, 130)]
JOINTS = (1, 3)
SEED = 7
CASE_SEED = {(32, 200): 12}         # seeds under which a case meets the input condition (tests/test_pointnet_train_cpu.py checks all of them)


def seed_of(B, N):
    return CASE_SEED.get((B, N), SEED)


@functools.lru_cache(maxsize=None)
def train_weights(J, seed=SEED):
    """pointnet_ref.make_weights (non-zero transform kernels, so the T-net paths carry gradient) with an eighth of the gammas negative:
    the pooled point of such a channel is its smallest pre-activation"""
    w = [np.array(a) for a in R.make_weights(J, seed)]
    rng = np.random.default_rng(seed + 1)
    i = 0
    for ci, co, bn, _ in R.layer_shapes(J):
        if bn:
            w[i + 2] = (w[i + 2] * np.where(rng.random(co) < 0.125, -1.0, 1.0)).astype(np.float32)
        i += 6 if bn else 2
    for a in w:
        a.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def case(B, N, J, seed=None):
    """(weights, x (B, N, 3) f32, y (B, 3 J) f32) of one test case, read-only"""
    seed = seed_of(B, N) if seed is None else seed
    x = R.make_clouds(B, N, R.UNIT, 100 * seed + 7 * B + N)
    y = np.random.default_rng(1000 * seed + 31 * B + N).normal(0, 0.3, (B, 3 * J)).astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return train_weights(J, seed), x, y


@functools.lru_cache(maxsize=None)
def masks_of(B, N, step_no=0):
    """the keep masks of the case's step: seed = the case's seed"""
    return dropout_masks(seed_of(B, N), step_no, B)


# ---- the timing baseline (tools/bench_kernels.py --pointnet-train; not shipped) ---------------------------------------------------------------------
def torch_modules(weights, device):
    """the same model as train-mode torch modules on `device`: Conv1d(kernel 1) / Linear + BatchNorm1d(eps 1e-3, momentum 1: the running
    statistics become the batch's) + ReLU, Dropout(0.3), bmm for the T-nets -> (net, loss_fn); net(x) -> (out, T3, T32),
    loss_fn(out, T3, T32, y) = the mean squared error + the two regularisers / B"""
    nn = torch.nn
    it = iter(weights)

    def block(conv, bn=True):
        k = np.asarray(next(it))
        k = k.reshape(k.shape[-2], k.shape[-1])
        lin = nn.Conv1d(k.shape[0], k.shape[1], 1) if conv else nn.Linear(k.shape[0], k.shape[1])
        lin.weight.data = torch.as_tensor(k.T.copy()).reshape(lin.weight.shape)
        lin.bias.data = torch.as_tensor(np.array(next(it)))
        if not bn:
            return lin
        norm = nn.BatchNorm1d(k.shape[1], eps=EPS, momentum=1.0)
        norm.weight.data, norm.bias.data = torch.as_tensor(np.array(next(it))), torch.as_tensor(np.array(next(it)))
        norm.running_mean.data, norm.running_var.data = torch.as_tensor(np.array(next(it))), torch.as_tensor(np.array(next(it)))
        return nn.Sequential(lin, norm, nn.ReLU())

    class TNet(nn.Module):
        def __init__(self, f):
            super().__init__()
            self.f = f
            self.convs = nn.Sequential(block(True), block(True), block(True))
            self.head = nn.Sequential(block(False), block(False), block(False, bn=False))

        def forward(self, h):                                # h (B, f, N)
            t = self.head(self.convs(h).amax(dim=2))
            return torch.bmm(h.transpose(1, 2), t.reshape(-1, self.f, self.f)).transpose(1, 2), t

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.t3 = TNet(3)
            self.front = nn.Sequential(block(True), block(True))
            self.t32 = TNet(32)
            self.trunk = nn.Sequential(block(True), block(True), block(True))
            self.head = nn.Sequential(block(False), nn.Dropout(0.3), block(False), nn.Dropout(0.3), block(False, bn=False))

        def forward(self, x):                                # x (B, N, 3)
            h, T3 = self.t3(x.transpose(1, 2))
            h, T32 = self.t32(self.front(h))
            return self.head(self.trunk(h).amax(dim=2)), T3, T32

    net = Net().to(device).train()
    assert next(it, None) is None
    eyes = {f: torch.eye(f, device=device) for f in (3, 32)}

    def loss_fn(out, T3, T32, y):
        reg = 0.0
        for t, f in ((T3, 3), (T32, 32)):
            x = t.reshape(-1, f, f)
            reg = reg + (0.001 * (torch.tensordot(x, x, dims=([2], [2])).reshape(-1, f, f) - eyes[f]) ** 2).sum()
        return ((out - y) ** 2).mean() + reg / out.shape[0]

    return net, loss_fn

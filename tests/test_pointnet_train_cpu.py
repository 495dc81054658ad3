"""CPU suite of PointNet training (AC19): the restatement tests/pointnet_train_ref.py is checked against finite differences
and hand expansions, the host pieces of the feature (Adam's formula, the dropout generator, the parameter buffer, names and defaults, the
argument checks of the C entries) against it, and the GPU suite's input condition is checked here so that a bad seed fails without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import pointnet_ref as R
from tests import pointnet_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("kpx_pointnet_train_floats", "kpx_pointnet_train_workspace_bytes", "kpx_pointnet_grad", "kpx_adam_step", "kpx_pointnet_train_step")


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------------------------
def _perturbed(weights, direction, h):
    """weights + h direction on the 74 trainable arrays (direction: 20 lists in the order of step()'s grads)"""
    out, i = [np.array(a, np.float64) for a in weights], 0
    for l, d in enumerate(direction):
        for q, a in enumerate(d):
            out[i + q] = out[i + q] + h * a.reshape(out[i + q].shape)
        i += 6 if l in T.BN_LAYERS else 2
    return out


def test_float64_restatement_passes_finite_differences_with_forced_selections():
    """J = 1, N = 4, B = 16: central differences along one random direction per layer and along three over all layers.  The loss is
    piecewise smooth (ReLU): a step of 1e-5 along a unit-variance direction already crosses kinks (measured: 10 % off at h = 1e-5, 1e-4 off
    at 1e-6, 3e-10 at 1e-7), so h = 1e-7, where rounding is ~1e-16 loss / h = 4e-9 absolute.  The bound, 1e-6 of sum |g_i d_i|, is a
    hundred times that and fails any wrong term."""
    w, x, y = T.case(16, 4, 1)
    masks = T.masks_of(16, 4)
    base = T.step(w, x, y, masks)
    pi = [base["i1"], base["i2"], base["i3"]]
    forced = T.step(w, x, y, masks, pi)
    assert abs(forced["loss"] - base["loss"]) <= 1e-14 * abs(base["loss"])
    rng = np.random.default_rng(0)
    h = 1e-7
    dirs = []
    for l in range(20):
        dirs.append([[rng.normal(size=a.shape) if k == l else np.zeros_like(a) for a in g] for k, g in enumerate(base["grads"])])
    dirs += [[[rng.normal(size=a.shape) for a in g] for g in base["grads"]] for _ in range(3)]
    for d in dirs:
        gd = sum(float((a * b).sum()) for g, dd in zip(forced["grads"], d) for a, b in zip(g, dd))
        size = sum(float(np.abs(a * b).sum()) for g, dd in zip(forced["grads"], d) for a, b in zip(g, dd))
        fd = (T.step(_perturbed(w, d, h), x, y, masks, pi)["loss"] - T.step(_perturbed(w, d, -h), x, y, masks, pi)["loss"]) / (2 * h)
        print(f"directional derivative {gd:.9e}, finite difference {fd:.9e}, size {size:.3e}")
        assert abs(fd - gd) <= 1e-6 * size


def test_regulariser_is_the_textbook_one_for_one_cloud_and_the_quirk_for_two():
    rng = np.random.default_rng(1)
    for f in (3, 32):
        t = rng.normal(0, 0.3, (1, f * f))
        M = t.reshape(f, f)
        want = 0.001 * ((M @ M.T - np.eye(f)) ** 2).sum()
        assert abs(float(T.regulariser(torch.tensor(t), f)) - want) <= 1e-12 * want
    B, f = 2, 3
    t = rng.normal(0, 0.5, (B, f * f))
    X = t.reshape(B, f, f)
    want = 0.0
    for b in range(B):
        for r in range(f):
            for b2 in range(B):
                for r2 in range(f):
                    chunk_row = ((b * f + r) * B + b2) % f          # (B, f, B, f) cut into f x f chunks: the row inside its chunk
                    want += 0.001 * (X[b, r] @ X[b2, r2] - (1.0 if chunk_row == r2 else 0.0)) ** 2
    assert abs(float(T.regulariser(torch.tensor(t), f)) - want) <= 1e-12 * want
    textbook = sum(0.001 * ((X[b] @ X[b].T - np.eye(f)) ** 2).sum() for b in range(B))
    assert abs(want - textbook) > 1e-3 * textbook                   # it is not the per-cloud sum


def test_momentum_zero_makes_the_moving_statistics_the_batch_statistics():
    w, x, y = T.case(16, 63, 3)
    r = T.step(w, x, y)
    d0 = R.split_weights(w)[0]
    z = np.asarray(x, np.float64) @ d0["K"] + d0["b"]
    assert np.abs(r["stats"][0][0] - z.mean((0, 1))).max() <= 1e-13 and np.abs(r["stats"][0][1] - z.var((0, 1))).max() <= 1e-13
    assert sorted(r["stats"]) == T.BN_LAYERS


def test_adam_against_the_closed_form_over_three_steps():
    """a constant gradient g: m_t = g (1 - b1^t), v_t = g^2 (1 - b2^t), so step t moves w by lr g s / (|g| s + eps), s = sqrt(1 - b2^t)"""
    g = np.array([0.0, 1e-12, -3e-4, 0.5, -7.0])
    w, m, v = np.zeros(5), np.zeros(5), np.zeros(5)
    want = np.zeros(5)
    for t in (1, 2, 3):
        w, m, v = T.adam(w, g, m, v, lr=0.005, t=t)
        s = np.sqrt(1 - 0.999 ** t)
        want = want - 0.005 * g * s / (np.abs(g) * s + 1e-7)
        assert np.abs(w - want).max() <= 1e-15
    assert w[0] == 0.0


# ---- 2. dropout ----------------------------------------------------------------------------------------------------------------------------------------
def test_dropout_generator_keep_fraction_and_the_two_host_mirrors():
    from kinectpy_amd import ops
    for seed, step in ((0, 0), (7, 3), (2 ** 40 + 5, 2 ** 33 + 1)):
        a, b = ops.pointnet_dropout_masks(seed, step, 64), T.dropout_masks(seed, step, 64)
        for m, r, width in zip(a, b, (256, 128)):
            assert m.shape == (64, width) and m.dtype == bool and np.array_equal(m, r)
            assert abs(m.mean() - 0.7) <= 5 * np.sqrt(0.21 / m.size)
    big = ops.pointnet_dropout_masks(1, 1, 4096)
    for m in big:
        assert abs(m.mean() - 0.7) <= 5 * np.sqrt(0.21 / m.size)
        assert abs(m.mean(0) - 0.7).max() <= 5 * np.sqrt(0.21 / 4096) and abs(m[:1024].mean(1) - 0.7).max() <= 5 * np.sqrt(0.21 / m.shape[1])
    assert not np.array_equal(ops.pointnet_dropout_masks(1, 1, 8)[0], ops.pointnet_dropout_masks(1, 2, 8)[0])
    assert not np.array_equal(ops.pointnet_dropout_masks(1, 1, 8)[0], ops.pointnet_dropout_masks(2, 1, 8)[0])


# ---- 3. the input condition of the GPU suite -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, N", T.CASES)
def test_gpu_cases_meet_the_input_condition(B, N):
    """the float32 restatements' own deviation (tau / 4) stays below 2^-8 of every layer's scale, with the float64 run's selections"""
    for J in T.JOINTS:
        w, x, y = T.case(B, N, J)
        for masks in (None, T.masks_of(B, N)):
            free = T.step(w, x, y, masks)
            _, tau, tau_loss = T.reference(w, x, y, masks, [free["i1"], free["i2"], free["i3"]])
            print(f"B={B} N={N} J={J} dropout={masks is not None}: worst tau / 4 = {max(tau) / 4:.3e}, loss {tau_loss / 4:.3e}")
            assert max(tau) / T.MARGIN <= T.CAP


def test_the_fixed_batch_of_the_learning_test_learns_on_the_cpu():
    """fit's GPU test asks for a last loss below a quarter of the first: the restatement with Adam (lr 0.005, 60 steps) on that batch
    goes 3.95 -> 0.61 in float64, under a fifth, so a quarter leaves a margin"""
    w, x, y = T.case(16, 64, 3)
    w = [np.array(a, np.float64) for a in w]
    idx = [i for i, name in enumerate(_trainable_flags()) if name]
    m, v = [np.zeros_like(w[i]) for i in idx], [np.zeros_like(w[i]) for i in idx]
    losses = []
    for t in range(1, 61):
        r = T.step(w, x, y, T.dropout_masks(0, t - 1, 16))
        losses.append(r["loss"])
        flat = [a for g in r["grads"] for a in g]
        for q, i in enumerate(idx):
            w[i], m[q], v[q] = T.adam(w[i], flat[q].reshape(w[i].shape), m[q], v[q], lr=0.005, t=t)
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0] / 5


def _trainable_flags():
    out = []
    for l in range(20):
        out += [True, True, True, True, False, False] if l in T.BN_LAYERS else [True, True]
    return out


# ---- 4. the surface ----------------------------------------------------------------------------------------------------------------------------------------
def test_names_defaults_and_what_is_not_built():
    import inspect
    from kinectpy_amd import ops
    from kinectpy_amd.models import pointnet as P
    for name in ("pointnet_train_pack", "pointnet_train_unpack", "pointnet_grad", "adam_step", "pointnet_train_step", "pointnet_dropout_masks"):
        assert callable(getattr(ops, name)), name
    a = P.Adam()
    assert (a.learning_rate, a.beta_1, a.beta_2, a.epsilon) == (0.001, 0.9, 0.999, 1e-7)
    sig = inspect.signature(P.PointNet.fit).parameters
    assert [(k, sig[k].default) for k in ("batch_size", "epochs", "validation_data", "shuffle", "callbacks", "seed")] == [
        ("batch_size", 16), ("epochs", 1), ("validation_data", None), ("shuffle", False), ("callbacks", ()), ("seed", 0)]
    assert inspect.signature(P.EarlyStopping).parameters["monitor"].default == "val_loss"
    assert inspect.signature(P.ModelCheckpoint).parameters["save_best_only"].default is True
    m = P.create_pointnet(64, 3)
    assert m.compile(optimizer=P.Adam(learning_rate=0.005)) is m and m.optimizer.learning_rate == 0.005
    for bad in ("mean_absolute_error", "huber", None):
        with pytest.raises(ValueError, match="not built"):
            m.compile(loss=bad)
    with pytest.raises(ValueError):
        m.compile(optimizer="sgd")
    with pytest.raises(ValueError):
        P.Adam(beta_1=1.0)
    with pytest.raises(RuntimeError, match="compiled"):
        P.create_pointnet(64, 3).train_on_batch(np.zeros((2, 64, 3), np.float32), np.zeros((2, 9), np.float32))
    with pytest.raises(ValueError):
        m.train_on_batch(np.zeros((2, 63, 3), np.float32), np.zeros((2, 9), np.float32))
    with pytest.raises(ValueError):
        m.train_on_batch(np.zeros((2, 64, 3), np.float32), np.zeros((2, 8), np.float32))


def test_parameter_buffer_round_trip_and_layout():
    from kinectpy_amd import ops
    from kinectpy_amd.models.pointnet import weight_shapes
    for J in (1, 3, 341):
        w = R.make_weights(J, 3)
        slots, trainable, total = ops.pointnet_train_layout(J)
        assert len(slots) == 108 and [s for _, s in slots] == weight_shapes(J)
        assert all(off % 64 == 0 for off, _ in slots) and trainable % 64 == 0 and total % 64 == 0
        moving = [off for (off, _), t in zip(slots, _trainable_flags()) if not t]
        assert min(moving) == trainable and max(off for (off, _), t in zip(slots, _trainable_flags()) if t) < trainable
        buf = ops.pointnet_train_pack_host(w)
        assert buf.dtype == np.float32 and buf.shape == (total,)
        back = ops.pointnet_train_unpack(buf, J)
        assert all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(w, back))
        assert ops._pn_train_joints_of(total) == J
    with pytest.raises(ValueError, match="108"):
        ops.pointnet_train_pack_host(w[:-1])
    with pytest.raises(ValueError, match="array 3 "):
        ops.pointnet_train_pack_host(w[:3] + [np.zeros(31, np.float32)] + w[4:])
    with pytest.raises(ValueError):
        ops.pointnet_train_unpack(buf[:-64], 341)
    with pytest.raises(ValueError, match="not a PointNet training"):
        ops._pn_train_joints_of(total + 64)


def test_callbacks_on_a_stub_model(tmp_path):
    from kinectpy_amd.models import pointnet as P

    class Stub:
        def __init__(self):
            self.optimizer, self.stop_training, self.saved = P.Adam(0.01), False, []

        def save_weights(self, path):
            self.saved.append(path)

    s = Stub()
    sched = P.LearningRateScheduler(lambda epoch, lr: lr * 0.5 if epoch else lr)
    sched.on_epoch_begin(s, 0)
    assert s.optimizer.learning_rate == 0.01
    sched.on_epoch_begin(s, 1)
    assert s.optimizer.learning_rate == 0.005
    stop = P.EarlyStopping(patience=2)
    for epoch, v in enumerate([3.0, 2.0, 2.5, 2.0, 1.0]):
        stop.on_epoch_end(s, epoch, {"val_loss": v})
        if s.stop_training:
            break
    assert s.stop_training and stop.stopped_epoch == 3 and stop.best == 2.0
    with pytest.raises(ValueError, match="val_loss"):
        P.EarlyStopping().on_epoch_end(s, 0, {"loss": 1.0})
    ck = P.ModelCheckpoint(str(tmp_path / "w{epoch}.npz"))
    for epoch, v in enumerate([3.0, 4.0, 2.0]):
        ck.on_epoch_end(s, epoch, {"val_loss": v})
    assert s.saved == [str(tmp_path / "w1.npz"), str(tmp_path / "w3.npz")]


# ---- 5. the ABI --------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_in_header_and_signatures():
    from kinectpy_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kinectpx.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.load()


def test_c_entries_reject_bad_arguments_on_the_host(lib):
    """nothing here reaches a device: this suite runs without one"""
    from kinectpy_amd import ops
    d = C.c_void_p(4096)
    err = lambda: lib.kpx_last_error()
    tr, total = C.c_int64(0), C.c_int64(0)
    for J in (1, 3, 341):
        assert lib.kpx_pointnet_train_floats(J, C.byref(total), C.byref(tr)) == 0
        assert (tr.value, total.value) == ops.pointnet_train_layout(J)[1:]
    assert lib.kpx_pointnet_train_floats(0, None, None) == -1 and lib.kpx_pointnet_train_floats(342, None, None) == -1 and b"1024" in err()
    f3 = ops.pointnet_train_layout(3)[2]

    def grad(params=d, floats=f3, x=d, y=d, B=2, N=64, J=3, loss=d, g=d, ws=d, wsz=1 << 40):
        return lib.kpx_pointnet_grad(params, floats, x, y, B, N, J, 0, 0, 1, loss, g, *([None] * 9), ws, wsz, None)

    for k in ("params", "x", "y", "loss", "g", "ws"):
        assert grad(**{k: None}) == -1 and b"null pointer" in err(), k
    assert grad(N=0) == -1 and b"at least one point" in err()
    assert grad(B=0, N=0) == -1
    assert grad(J=0) == -1 and b"joints" in err()
    assert grad(J=342) == -1 and b"1024" in err()
    assert grad(B=-1) == -1
    assert grad(B=2 ** 15, N=2 ** 16) == -3 and b"2^31" in err()
    assert grad(floats=f3 + 64) == -1 and b"parameter buffer" in err()
    assert grad(params=C.c_void_p(4100)) == -1 and b"aligned" in err()
    assert grad(wsz=16) == -2 and b"workspace too small" in err()
    assert grad(B=0, x=None, y=None, loss=None, g=None, ws=None, wsz=0) == 0                  # an empty batch is a no-op
    q = lib.kpx_pointnet_train_workspace_bytes
    assert 0 < q(1, 64, 3) < q(16, 64, 3) < q(16, 1024, 3) and q(16, 64, 3) <= q(16, 64, 32)
    assert q(2, 0, 3) == 0 and q(2, 64, 342) == 0 and q(2 ** 15, 2 ** 16, 3) == 0 and q(-1, 64, 3) == 0
    adam = lambda w=d, g=d, m=d, v=d, n=10, b1=0.9, b2=0.999, t=1: lib.kpx_adam_step(w, g, m, v, n, 0.001, b1, b2, 1e-7, t, None)
    for k in ("w", "g", "m", "v"):
        assert adam(**{k: None}) == -1 and b"null pointer" in err(), k
    assert adam(n=-1) == -1 and adam(t=0) == -1 and adam(b1=1.0) == -1 and adam(b2=-0.1) == -1
    assert adam(n=0, w=None, g=None, m=None, v=None) == 0
    step = lambda B=2, N=64, ws=d, wsz=1 << 40: lib.kpx_pointnet_train_step(d, f3, d, d, B, N, 3, 0, 0, 1, d, d, d, d, 0.001, 0.9, 0.999, 1e-7, 1, ws, wsz, None)
    assert step(N=0) == -1 and step(B=2 ** 15, N=2 ** 16) == -3 and step(wsz=16) == -2

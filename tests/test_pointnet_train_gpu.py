"""GPU suite of PointNet training (AC19).  Gradients and loss are judged by the deviation rule of
tests/pointnet_train_ref.py: per layer, max |g_gpu - g64| <= tau x the layer's scale, tau = 4 x the worst float32 CPU restatement, with the
float64 reference and the restatements gathering at the DEVICE's pooled points (a near tie picked differently moves a whole channel's
gradient); that those points are valid maxima is a test of its own.  Sizes: N on both sides of the 64-point tile, more than one tile, B
not a multiple of the 16-row head chunks, B above them; every case's device run and reference are computed once and shared.

Measured on MI355X: see DESIGN.md 5.20."""
import functools

import numpy as np
import pytest
import torch

from tests import pointnet_train_ref as T

pytestmark = pytest.mark.gpu


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def layers_of(flat, J):
    """a vector in the trainable layout -> 20 lists (kernel, bias[, gamma, beta]) as step()'s grads"""
    from kinectpy_amd import ops
    slots, out, k = ops.pointnet_train_layout(J)[0], [], 0
    for l in range(20):
        n = 6 if l in T.BN_LAYERS else 2
        out.append([flat[off:off + int(np.prod(shape))].reshape(shape[-2:] if len(shape) == 3 else shape) for off, shape in slots[k:k + min(n, 4)]])
        k += n
    return out


@functools.lru_cache(maxsize=None)
def device_run(B, N, J, drop):
    from kinectpy_amd import ops
    w, x, y = T.case(B, N, J)
    params = ops.pointnet_train_pack(w)
    loss, grad, st = ops.pointnet_grad(params, np.array(x), np.array(y), seed=T.seed_of(B, N), step=0, training_dropout=drop, want_stages=True)
    return dict(loss=loss.cpu().numpy(), grad=grad.cpu().numpy(), params=params.cpu().numpy(), **{k: v.cpu().numpy() for k, v in st.items()})


@functools.lru_cache(maxsize=None)
def judged(B, N, J, drop):
    """(device run, float64 reference at the device's pooled points, tau per layer, tau of the loss)"""
    got = device_run(B, N, J, drop)
    w, x, y = T.case(B, N, J)
    r64, tau, tau_loss = T.reference(w, x, y, T.masks_of(B, N) if drop else None, [got["i1"], got["i2"], got["i3"]])
    return got, r64, tau, tau_loss


def check_gradients(B, N, J, drop):
    got, r64, tau, tau_loss = judged(B, N, J, drop)
    assert np.isfinite(got["grad"]).all() and np.isfinite(got["loss"]).all()
    dev = T.layer_dev(layers_of(got["grad"], J), r64["grads"])
    for l in range(20):
        print(f"B={B} N={N} J={J} dropout={drop} layer {l}: deviation {dev[l]:.3e} of scale, tau {tau[l]:.3e}")
    dl = abs(float(got["loss"][0]) - r64["loss"]) / abs(r64["loss"])
    print(f"loss {got['loss'][0]:.7f} against {r64['loss']:.7f}: deviation {dl:.3e}, tau {tau_loss:.3e}")
    for l in range(20):
        assert dev[l] <= tau[l], (l, dev[l], tau[l])
    assert dl <= tau_loss
    assert abs(float(got["loss"][1]) + float(got["loss"][2]) - float(got["loss"][0])) <= 2e-7 * abs(float(got["loss"][0]))
    assert abs(float(got["loss"][2]) - r64["reg"]) <= max(tau_loss * abs(r64["loss"]), 1e-6 * abs(r64["reg"]))
    return got, r64


# ---- the pooled points ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", T.JOINTS)
@pytest.mark.parametrize("B, N", T.CASES)
def test_pooled_points_are_float64_maxima_and_the_lowest_on_ties(B, N, J):
    """the float64 activation at the device's point is within the float32 restatement's own deviation (x 4) of the float64 maximum; where
    the float64 maximum is attained more than once the device reports the lowest such point"""
    got = device_run(B, N, J, False)
    w, x, y = T.case(B, N, J)
    free = T.step(w, x, y)
    free32 = T.step(w, x, y, dtype=torch.float32)
    for q in range(3):
        a, idx = free["pre3"][q], got[f"i{q + 1}"].astype(np.int64)
        assert idx.min() >= 0 and idx.max() < N
        top = a.max(1)
        tol = T.MARGIN * np.abs(free32[f"g{q + 1}"] - free[f"g{q + 1}"]).max()
        miss = (top - np.take_along_axis(a, idx[:, None, :], 1)[:, 0]).max()
        print(f"B={B} N={N} J={J} pool {q}: worst miss {miss:.3e}, tolerance {tol:.3e}, points differing from float64's {(idx != a.argmax(1)).sum()}")
        assert miss <= tol
        tied = (a == top[:, None, :]).sum(1) > 1
        assert np.array_equal(idx[tied], a.argmax(1)[tied])
        dev = np.abs(got[f"g{q + 1}"] - free[f"g{q + 1}"]).max()
        assert dev <= tol, (q, dev, tol)


# ---- gradients and loss --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("J", T.JOINTS)
@pytest.mark.parametrize("B, N", T.CASES)
def test_gradients_and_loss_within_tau(B, N, J, drop):
    check_gradients(B, N, J, drop)


@pytest.mark.parametrize("B, N", T.SMALL)
def test_small_batches_are_finite_and_within_tau(B, N):
    """B N below one 64-point tile's worth of clouds, one-row batch normalisation, the regulariser's quirk at B = 2"""
    got, r64 = check_gradients(B, N, 3, True)
    if B == 1:
        g = layers_of(got["grad"], 3)
        for l in (3, 4, 11, 12, 17, 18):                 # behind a one-row batch normalisation: x - mean = 0, dz = 0
            assert not g[l][0].any() and not g[l][1].any() and not g[l][2].any(), l
        for l in (0, 1, 2, 6, 7, 8, 9, 10, 14, 15, 16):  # ... and nothing reaches the trunks
            assert all(not a.any() for a in g[l]), l


# ---- moving statistics ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, N", [(16, 65), (17, 130)])
def test_moving_statistics_are_the_batch_statistics(B, N):
    from kinectpy_amd import ops
    got, r64, _, _ = judged(B, N, 3, True)
    w, x, y = T.case(B, N, 3)
    r32 = T.step(w, x, y, T.masks_of(B, N), [got["i1"], got["i2"], got["i3"]], torch.float32)
    un = ops.pointnet_train_unpack(got["params"], 3)
    k = 0
    for l in range(20):
        if l in T.BN_LAYERS:
            for q in (0, 1):
                ref, scale = r64["stats"][l][q], np.abs(r64["stats"][l][q]).max()
                tol = T.MARGIN * np.abs(r32["stats"][l][q] - ref).max() / scale
                dev = np.abs(un[k + 4 + q] - ref).max() / scale
                print(f"layer {l} {'mean' if q == 0 else 'variance'}: deviation {dev:.3e}, tolerance {tol:.3e}")
                assert dev <= tol
            for q in range(4):                           # the trainable arrays are not touched by pointnet_grad
                assert np.array_equal(un[k + q], np.asarray(w[k + q], np.float32))
        k += 6 if l in T.BN_LAYERS else 2


def test_predict_after_train_on_batch_is_the_forward_on_get_weights():
    from kinectpy_amd import ops
    from kinectpy_amd.models.pointnet import Adam, create_pointnet
    w, x, y = T.case(16, 64, 3)
    m = create_pointnet(64, 3)
    m.set_weights(w)
    before = _bits(m.predict(np.array(x)))
    m.compile(optimizer=Adam(0.005))
    loss = m.train_on_batch(np.array(x), np.array(y))
    assert np.isfinite(float(loss))
    after = m.predict(np.array(x))
    trained = m.get_weights()
    assert not np.array_equal(_bits(after), before) and not np.array_equal(trained[0], w[0])
    assert np.array_equal(_bits(after), _bits(ops.pointnet_forward(ops.pointnet_pack(ops.pointnet_fold(trained)), np.array(x))))
    got = device_run(16, 64, 3, True)                    # the moving statistics are the first step's batch statistics
    un = ops.pointnet_train_unpack(got["params"], 3)
    assert np.array_equal(trained[4], un[4]) and np.array_equal(trained[5], un[5])
    t = m._train["t"]
    m.set_weights(trained)                               # set_weights starts the optimiser again
    assert m._train is None and t == 1


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------------------------
def _ulps(a, ref64):
    r = ref64.astype(np.float32)
    return np.abs(a.astype(np.float64) - r.astype(np.float64)) / np.spacing(np.abs(r)).astype(np.float64)


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 100003])
def test_adam_step_within_two_ulp_of_the_float64_formula(count, t):
    from kinectpy_amd import ops
    rng = np.random.default_rng(count + t)
    w = rng.normal(0, 1, count).astype(np.float32)
    g = (rng.normal(0, 1, count) * 10.0 ** rng.integers(-12, 1, count)).astype(np.float32)
    g[::7] = 0.0
    g[3::11] = 1e-30
    m = (rng.normal(0, 0.1, count) * (t > 1)).astype(np.float32)
    v = (rng.random(count) * 0.01 * (t > 1)).astype(np.float32)
    dw, dm, dv = (torch.as_tensor(a).cuda() for a in (w, m, v))
    ops.adam_step(dw, torch.as_tensor(g).cuda(), dm, dv, learning_rate=0.005, t=t)
    rw, rm, rv = T.adam(w, g, m, v, lr=0.005, t=t)
    for name, a, r in (("w", dw, rw), ("m", dm, rm), ("v", dv, rv)):
        u = _ulps(a.cpu().numpy(), r)
        print(f"count {count} t {t} {name}: worst {u.max():.2f} ulp")
        assert u.max() <= 2.0, name


# ---- composition, determinism, a poisoned workspace -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, N", [(16, 65), (5, 130)])
def test_train_step_is_grad_then_adam_twice_the_same_bits_whatever_the_workspace_held(B, N):
    from kinectpy_amd import _lib, ops
    w, x, y = T.case(B, N, 3)
    x, y = torch.as_tensor(np.array(x)).cuda(), torch.as_tensor(np.array(y)).cuda()
    n = ops.pointnet_train_layout(3)[1]
    seed = T.seed_of(B, N)

    def two_calls():
        p = ops.pointnet_train_pack(w)
        m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        loss, grad = ops.pointnet_grad(p, x, y, seed=seed, step=3)
        ops.adam_step(p[:n], grad, m, v, learning_rate=0.005, t=1)
        return [_bits(a) for a in (loss, grad, p, m, v)]

    def one_call():
        p = ops.pointnet_train_pack(w)
        m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        loss, grad = ops.pointnet_train_step(p, x, y, m, v, learning_rate=0.005, t=1, seed=seed, step=3)
        return [_bits(a) for a in (loss, grad, p, m, v)]

    a, b = two_calls(), one_call()
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert np.array_equal(device_run(B, N, 3, True)["grad"].view(np.uint32), _bits(ops.pointnet_grad(ops.pointnet_train_pack(w), x, y, seed=seed, step=0)[1]))
    for poison in (0xFF, 0x7F):                          # NaN patterns, then large finite values
        _lib.workspace(1)                                # the calling stream's scratch exists
        for ws in _lib._ws.values():
            if ws.buf is not None:
                ws.buf.fill_(poison)
        c = one_call()
        assert all(np.array_equal(p, q) for p, q in zip(a, c)), hex(poison)


def test_empty_batch_and_argument_errors():
    from kinectpy_amd import _lib, ops
    p = ops.pointnet_train_pack(T.train_weights(3))
    loss, grad = ops.pointnet_grad(p, torch.empty((0, 64, 3), device="cuda"), torch.empty((0, 9), device="cuda"))
    assert loss.cpu().tolist() == [0.0, 0.0, 0.0] and not grad.any()
    with pytest.raises(_lib.KinectPxError, match="at least one point"):
        ops.pointnet_grad(p, torch.empty((2, 0, 3), device="cuda"), torch.empty((2, 9), device="cuda"))
    with pytest.raises(ValueError):
        ops.pointnet_grad(p, torch.empty((2, 5, 3), device="cuda"), torch.empty((2, 8), device="cuda"))
    with pytest.raises(ValueError, match="not a PointNet training"):
        ops.pointnet_grad(p[:-64].contiguous(), torch.empty((2, 5, 3), device="cuda"), torch.empty((2, 9), device="cuda"))


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_fit_on_one_batch_learns_and_the_callbacks_act(tmp_path):
    from kinectpy_amd.metrics.metric import percentual_correct_keypoints
    from kinectpy_amd.models.pointnet import Adam, EarlyStopping, LearningRateScheduler, ModelCheckpoint, create_pointnet
    w, x, y = T.case(16, 64, 3)
    x, y = np.array(x), np.array(y)
    m = create_pointnet(64, 3)
    m.set_weights(w)
    m.compile(optimizer=Adam(learning_rate=0.005), metrics=[percentual_correct_keypoints(0.5)])
    h = m.fit(x, y, batch_size=16, epochs=60)
    print(f"loss {h['loss'][0]:.4f} -> {h['loss'][-1]:.4f}")
    assert len(h["loss"]) == 60 and h["loss"][-1] < h["loss"][0] / 4
    assert len(h["percentual_correct_keypoints_0.5"]) == 60 and 0.0 <= h["percentual_correct_keypoints_0.5"][-1] <= 1.0
    # a short last batch is trained as it is: 16 samples in batches of 6 are three steps an epoch, the last on 4 samples.  (A last batch
    # of ONE sample is trained too, but momentum 0 then leaves zero moving variances in the heads and validation blows up, as in Keras.)
    t0 = m._train["t"]
    h = m.fit(x, y, batch_size=6, epochs=2, validation_data=(x[:7], y[:7]), shuffle=True, seed=3)
    assert m._train["t"] == t0 + 6 and set(h) == {"loss", "val_loss", "percentual_correct_keypoints_0.5", "val_percentual_correct_keypoints_0.5"}
    assert all(np.isfinite(v) for v in h["val_loss"])
    # LearningRateScheduler changes the step size: with rate 0 nothing moves
    before = m.get_weights()
    m.fit(x, y, epochs=1, callbacks=[LearningRateScheduler(lambda epoch, lr: 0.0)])
    after = m.get_weights()
    assert m.optimizer.learning_rate == 0.0 and all(np.array_equal(a, b) for a, b in zip(before[:4], after[:4]))
    m.optimizer.learning_rate = 0.005
    # EarlyStopping stops at the first epoch whose val_loss is no new best (patience 1).  With rate 0 the weights stand still and val_loss
    # only wobbles with the dropout masks behind the main head's batch statistics, so ten epochs without a stop would need ten successive
    # improvements; ModelCheckpoint has written the best epoch, and load_weights reads it
    stop = EarlyStopping(monitor="val_loss", patience=1)
    ck = ModelCheckpoint(str(tmp_path / "best.npz"), save_best_only=True)
    m.optimizer.learning_rate = 0.0
    h = m.fit(x, y, epochs=10, validation_data=(x, y), callbacks=[stop, ck])
    v = h["val_loss"]
    expect = next(e for e in range(1, len(v) + 1) if e == len(v) or not v[e] < min(v[:e]))
    assert len(v) < 10 and len(v) == expect + 1 and stop.stopped_epoch == expect and ck.best == min(v)
    other = create_pointnet(64, 3)
    other.load_weights(str(tmp_path / "best.npz"))
    assert all(np.array_equal(a, b) for a, b in zip(other.get_weights()[:4], m.get_weights()[:4]))
    assert torch.isfinite(other.predict(x)).all()

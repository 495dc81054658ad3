"""Host mirror of the reference's models/pointnet.py: create_pointnet(number_of_points, number_of_joints) returns a PointNet whose
weights are laid out as Keras' model.get_weights() of the reference model (108 arrays).
  inference: predict is the fused MI355X path (kpx_pointnet_forward; arithmetic contract AC18): batch normalisation on
      its moving statistics, dropout the identity.
  training:  compile(loss="mean_squared_error", optimizer=Adam(...), metrics=[...]), train_on_batch and fit run train.py's loop on the
      device (kpx_pointnet_train_step; AC19): batch statistics, Dropout(0.3), mean squared error plus the two
      OrthogonalRegularizer terms, Adam; LearningRateScheduler, EarlyStopping and ModelCheckpoint are the three callbacks train.py uses.
      Not built: other optimisers and losses, weight decay, mixed precision, the KinectDataset readers, the yacs configs, wandb.

predict_joints chains sampler -> normaliser -> forward -> inverse map on the device, as evaluate.py does around the Keras model.
"""
import numpy as np
import torch

from .. import ops

_BN = ("kernel", "bias", "gamma", "beta", "moving_mean", "moving_variance")


def _block_names():
    tnet = lambda t: [f"{t}/conv1", f"{t}/conv2", f"{t}/conv3", f"{t}/dense1", f"{t}/dense2", f"{t}/transform"]
    return tnet("tnet3") + ["conv1", "conv2"] + tnet("tnet32") + ["conv3", "conv4", "conv5", "dense1", "dense2", "joints"]


def weight_names():
    """names of the 108 arrays in Keras' get_weights() order (the keys save_weights writes)"""
    names = []
    for block, (_, _, bn) in zip(_block_names(), ops.POINTNET_LAYERS):
        names += [f"{block}/{q}" for q in (_BN if bn else _BN[:2])]
    return names


def weight_shapes(number_of_joints):
    """shapes of the 108 arrays: Conv1D kernels (1, c_in, c_out), Dense kernels (c_in, c_out), vectors (c_out,)"""
    shapes = []
    for block, (ci, co, bn) in zip(_block_names(), ops.pointnet_layer_shapes(number_of_joints)):
        shapes.append((1, ci, co) if "conv" in block else (ci, co))
        shapes += [(co,)] * (5 if bn else 1)
    return shapes


class Adam:
    """keras.optimizers.Adam's hyper-parameters (the update itself is ops.adam_step)"""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = float(learning_rate), float(beta_1), float(beta_2), float(epsilon)
        if not (0.0 <= self.beta_1 < 1.0 and 0.0 <= self.beta_2 < 1.0):
            raise ValueError("Adam: beta_1 and beta_2 must lie in [0, 1)")


class LearningRateScheduler:
    """keras.callbacks.LearningRateScheduler: schedule(epoch, lr) -> lr, applied when an epoch begins"""

    def __init__(self, schedule):
        self.schedule = schedule

    def on_epoch_begin(self, model, epoch):
        model.optimizer.learning_rate = float(self.schedule(epoch, model.optimizer.learning_rate))

    def on_epoch_end(self, model, epoch, logs):
        pass


class EarlyStopping:
    """keras.callbacks.EarlyStopping: stops after `patience` epochs without an improvement (a decrease) of `monitor`"""

    def __init__(self, monitor="val_loss", patience=0):
        self.monitor, self.patience = monitor, int(patience)
        self.best, self.wait, self.stopped_epoch = None, 0, None

    def on_epoch_begin(self, model, epoch):
        pass

    def on_epoch_end(self, model, epoch, logs):
        if self.monitor not in logs:
            raise ValueError(f"EarlyStopping: {self.monitor!r} is not among the epoch's logs {sorted(logs)}")
        value = logs[self.monitor]
        if self.best is None or value < self.best:
            self.best, self.wait = value, 0
            return
        self.wait += 1
        if self.wait >= self.patience:
            self.stopped_epoch, model.stop_training = epoch, True


class ModelCheckpoint:
    """keras.callbacks.ModelCheckpoint for weights: model.save_weights(filepath) (.npz) at the end of an epoch -- with save_best_only,
    only when `monitor` improved.  filepath may contain {epoch}."""

    def __init__(self, filepath, monitor="val_loss", save_best_only=True):
        self.filepath, self.monitor, self.save_best_only, self.best = str(filepath), monitor, bool(save_best_only), None

    def on_epoch_begin(self, model, epoch):
        pass

    def on_epoch_end(self, model, epoch, logs):
        if self.save_best_only:
            if self.monitor not in logs:
                raise ValueError(f"ModelCheckpoint: {self.monitor!r} is not among the epoch's logs {sorted(logs)}")
            if self.best is not None and not logs[self.monitor] < self.best:
                return
            self.best = logs[self.monitor]
        model.save_weights(self.filepath.format(epoch=epoch + 1))


class PointNet:
    """The reference's Keras model: set_weights / get_weights / load_weights / save_weights / predict, and compile / train_on_batch / fit."""

    name = "pointnet"

    def __init__(self, number_of_points, number_of_joints, seed=0):
        number_of_points, number_of_joints = int(number_of_points), int(number_of_joints)
        if number_of_points < 1:
            raise ValueError("create_pointnet: number_of_points must be positive")
        if not 1 <= number_of_joints or 3 * number_of_joints > ops.POINTNET_MAX_OUT:
            raise ValueError(f"create_pointnet: number_of_joints must be in [1, {ops.POINTNET_MAX_OUT // 3}]")
        self.number_of_points, self.number_of_joints = number_of_points, number_of_joints
        self._packed = None
        # Keras' initial state: Glorot-uniform kernels, zero biases, unit gamma and variance, zero beta and mean; the T-nets' last
        # Dense starts as the identity transform (zero kernel, identity bias)
        rng = np.random.default_rng(seed)
        w = []
        for name, shape in zip(weight_names(), weight_shapes(number_of_joints)):
            kind = name.rsplit("/", 1)[1]
            if kind == "kernel":
                if name.endswith("transform/kernel"):
                    w.append(np.zeros(shape, np.float32))
                else:
                    limit = np.sqrt(6.0 / (shape[-2] + shape[-1]))
                    w.append(rng.uniform(-limit, limit, shape).astype(np.float32))
            elif kind == "bias" and "transform" in name:
                w.append(np.eye(int(round(np.sqrt(shape[0]))), dtype=np.float32).reshape(-1))
            else:
                w.append((np.ones if kind in ("gamma", "moving_variance") else np.zeros)(shape, np.float32))
        self._weights = w
        self._train = None               # device state of training: params, m, v, t (Adam's step count), step (dropout's counter)
        self._stale = False              # the trained parameters are ahead of self._weights
        self.optimizer, self.metrics, self.stop_training = None, [], False

    # ---- weights ------------------------------------------------------------------------------------------------------------------
    def _sync(self):
        if self._stale:
            self._weights, self._stale = ops.pointnet_train_unpack(self._train["params"], self.number_of_joints), False

    def get_weights(self):
        """the 108 arrays; after training, the trained ones with the last step's moving statistics"""
        self._sync()
        return [a.copy() for a in self._weights]

    def set_weights(self, weights):
        weights = list(weights)
        names, shapes = weight_names(), weight_shapes(self.number_of_joints)
        if len(weights) != len(names):
            raise ValueError(f"set_weights: expected {len(names)} arrays (Keras get_weights() of create_pointnet), got {len(weights)}")
        new = []
        for i, (a, name, shape) in enumerate(zip(weights, names, shapes)):
            a = np.asarray(a)
            if a.shape != shape:
                raise ValueError(f"set_weights: array {i} ({name}) has shape {a.shape}, expected {shape}")
            new.append(np.array(a, dtype=np.float32))
        self._weights, self._packed, self._train, self._stale = new, None, None, False          # the optimiser state starts again

    def save_weights(self, path):
        """one .npz with the arrays under their names (weight_names())"""
        self._sync()
        with open(path, "wb") as f:
            np.savez(f, **dict(zip(weight_names(), self._weights)))

    def load_weights(self, path):
        """a .npz written by save_weights, or np.savez(path, *keras_model.get_weights()) (keys arr_0 .. arr_107)"""
        with np.load(path) as z:
            names, keys = weight_names(), set(z.files)
            positional = [f"arr_{i}" for i in range(len(names))]
            if keys == set(names):
                order = names
            elif keys == set(positional):
                order = positional
            else:
                missing = [k for k in (names if any(k in keys for k in names) else positional) if k not in keys]
                raise ValueError(f"load_weights: {path}: {len(keys)} arrays, expected the {len(names)} of create_pointnet"
                                 + (f"; missing {missing[0]}" if missing else f"; unexpected {sorted(keys - set(names) - set(positional))[0]}"))
            self.set_weights([z[k] for k in order])

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def packed(self):
        """the folded, packed model on the device (built on first use, dropped by set_weights)"""
        self._sync()
        if self._packed is None:
            self._packed = ops.pointnet_pack(ops.pointnet_fold(self._weights))
        return self._packed

    def predict(self, x):
        """x (B, number_of_points, 3), a device tensor or NumPy -> joints f32 (B, 3 J) device tensor"""
        if not isinstance(x, torch.Tensor):
            x = np.asarray(x, dtype=np.float32)
        if x.ndim != 3 or tuple(x.shape[1:]) != (self.number_of_points, 3):
            raise ValueError(f"predict: expected (B, {self.number_of_points}, 3), got {tuple(x.shape)}")
        return ops.pointnet_forward(self.packed(), x)

    __call__ = predict

    # ---- training (AC19) ------------------------------------------------------------------------------------------
    def compile(self, loss="mean_squared_error", optimizer=None, metrics=None):
        """train.py's model.compile: the mean squared error (the T-nets' regularisers are part of the model), Adam, metrics as callables
        (y_true, y_pred) -> float such as metrics.metric.percentual_correct_keypoints(threshold)"""
        if loss != "mean_squared_error":
            raise ValueError(f"compile: loss {loss!r} is not built: only 'mean_squared_error'")
        optimizer = Adam() if optimizer is None else optimizer
        if not isinstance(optimizer, Adam):
            raise ValueError("compile: optimizer must be a models.pointnet.Adam")
        self.optimizer, self.metrics = optimizer, list(metrics or [])
        return self

    def _state(self):
        if self.optimizer is None:
            raise RuntimeError("the model must be compiled before it is trained: model.compile(optimizer=Adam(...))")
        if self._train is None:
            params = ops.pointnet_train_pack(self._weights)
            n = ops.pointnet_train_layout(self.number_of_joints)[1]
            self._train = dict(params=params, m=torch.zeros(n, dtype=torch.float32, device=params.device),
                               v=torch.zeros(n, dtype=torch.float32, device=params.device), t=0, step=0, seed=0)
        return self._train

    def _check_xy(self, who, x, y):
        x = x if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float32)
        y = y if isinstance(y, torch.Tensor) else np.asarray(y, dtype=np.float32)
        if x.ndim != 3 or tuple(x.shape[1:]) != (self.number_of_points, 3):
            raise ValueError(f"{who}: expected x (B, {self.number_of_points}, 3), got {tuple(x.shape)}")
        if y.ndim != 2 or tuple(y.shape) != (x.shape[0], 3 * self.number_of_joints):
            raise ValueError(f"{who}: expected y ({x.shape[0]}, {3 * self.number_of_joints}), got {tuple(y.shape)}")
        return x, y

    def _train_batch(self, x, y, want_out):
        s, o = self._state(), self.optimizer
        s["t"] += 1
        hyper = dict(learning_rate=o.learning_rate, beta_1=o.beta_1, beta_2=o.beta_2, epsilon=o.epsilon, t=s["t"])
        out = None
        if want_out:
            loss, grad, st = ops.pointnet_grad(s["params"], x, y, seed=s["seed"], step=s["step"], want_stages=True)
            ops.adam_step(s["params"][:grad.numel()], grad, s["m"], s["v"], **hyper)
            out = st["out"]
        else:
            loss, _ = ops.pointnet_train_step(s["params"], x, y, s["m"], s["v"], seed=s["seed"], step=s["step"], **hyper)
        s["step"] += 1
        self._packed, self._stale = None, True
        return loss, out

    def train_on_batch(self, x, y):
        """one step on the batch x (B, number_of_points, 3), y (B, 3 J) -> the loss (mean squared error + regulariser) as a device scalar"""
        x, y = self._check_xy("train_on_batch", x, y)
        return self._train_batch(x, y, False)[0][0]

    def _validate(self, x, y, batch_size):
        """inference-mode loss and metrics: the mean squared error plus the regulariser of the inference-mode T3 and T32"""
        total, n, preds = 0.0, int(x.shape[0]), []
        for i in range(0, n, batch_size):
            xb, yb = x[i:i + batch_size], ops._dev(y[i:i + batch_size], torch.float32)
            out, st = ops.pointnet_forward(self.packed(), xb, want_stages=True)
            reg = 0.0
            for T, f in ((st["T3"], 3), (st["T32"], 32)):
                X = T.reshape(-1, f)
                G = (X @ X.T).reshape(-1, f, f)
                reg = reg + 0.001 * ((G - torch.eye(f, dtype=G.dtype, device=G.device)) ** 2).sum()
            total += float(((out - yb) ** 2).mean() + reg / out.shape[0]) * out.shape[0]
            preds.append(out)
        pred = torch.cat(preds)
        logs = {"val_loss": total / n}
        for f in self.metrics:
            logs["val_" + f.__name__] = f(ops._dev(y, torch.float32), pred)
        return logs

    def fit(self, x, y, batch_size=16, epochs=1, validation_data=None, shuffle=False, callbacks=(), seed=0):
        """train.py's model.fit on arrays: batches of batch_size in order (shuffle: a permutation per epoch from `seed`), the short last batch
        trained as it is -> the history dict: per epoch "loss" (the mean of the batch losses weighted by their sizes), the metrics' names
        (on the training batches' train-mode outputs), and with validation_data = (x, y) "val_loss" and "val_<metric>"."""
        x, y = self._check_xy("fit", x, y)
        if validation_data is not None:
            vx, vy = self._check_xy("fit: validation_data", *validation_data)
        batch_size = int(batch_size)
        if batch_size < 1 or x.shape[0] < 1:
            raise ValueError("fit: batch_size and the number of samples must be positive")
        state = self._state()
        state["seed"] = int(seed)
        rng = np.random.default_rng(seed)
        n, history, self.stop_training = int(x.shape[0]), {}, False
        for epoch in range(int(epochs)):
            for cb in callbacks:
                cb.on_epoch_begin(self, epoch)
            order = rng.permutation(n) if shuffle else np.arange(n)
            losses, sizes, outs = [], [], []
            for i in range(0, n, batch_size):
                sel = order[i:i + batch_size]
                if shuffle:
                    sel_t = torch.as_tensor(sel, device=x.device) if isinstance(x, torch.Tensor) else sel
                    xb = x[sel_t]
                    yb = y[torch.as_tensor(sel, device=y.device)] if isinstance(y, torch.Tensor) else y[sel]
                else:
                    xb, yb = x[i:i + batch_size], y[i:i + batch_size]
                loss, out = self._train_batch(xb, yb, bool(self.metrics))
                losses.append(loss[0])
                sizes.append(len(sel))
                if out is not None:
                    outs.append((ops._dev(yb, torch.float32), out))
            w = torch.as_tensor(sizes, dtype=torch.float64, device=losses[0].device)
            logs = {"loss": float((torch.stack(losses).double() * w).sum() / w.sum())}
            for f in self.metrics:
                logs[f.__name__] = f(torch.cat([a for a, _ in outs]), torch.cat([b for _, b in outs]))
            if validation_data is not None:
                logs.update(self._validate(vx, vy, batch_size))
            for k, v in logs.items():
                history.setdefault(k, []).append(v)
            for cb in callbacks:
                cb.on_epoch_end(self, epoch, logs)
            if self.stop_training:
                break
        return history


def create_pointnet(number_of_points: int, number_of_joints: int):
    """models/pointnet.py create_pointnet: the classification path of PointNet regressing 3 number_of_joints coordinates"""
    return PointNet(number_of_points, number_of_joints)


def predict_joints(clouds, model, normalization="", sampler="farthest", start_index=0, seed=None):
    """clouds (a list of (n_i, 3) clouds, n_i >= model.number_of_points) -> joints f64 (B, 3 J) device tensor in the clouds' own frame:
    the fixed-size sample (ops.farthest_point_sample_batch, or ops.sample_points for sampler="random"), the normaliser of
    utils/normalization.py, the forward pass and the inverse map of the joints, without a host round trip.  normalization: "",
    "translation" or "obb_rotation_translation"; "obb_normalization" raises as evaluate.py does (its inverse map is not defined)."""
    if normalization == "obb_normalization":
        raise NotImplementedError("Needs to apply inverse mapping to evaluate")
    if normalization not in ("", "translation", "obb_rotation_translation"):
        raise ValueError(f"predict_joints: unknown normalization {normalization!r}")
    if sampler not in ("farthest", "random"):
        raise ValueError(f"predict_joints: unknown sampler {sampler!r}")
    N = model.number_of_points
    clouds = [ops._dev(c, torch.float32).reshape(-1, 3) for c in clouds]
    if not clouds:
        return torch.empty((0, 3 * model.number_of_joints), dtype=torch.float64, device=ops.L.device())
    if sampler == "farthest":
        sel, _ = ops.farthest_point_sample_batch(clouds, N, start_index)
        x = torch.stack([c[s.long()] for c, s in zip(clouds, sel)])
    else:
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        x = torch.stack([ops.sample_points(c, N, seed + i)[0] for i, c in enumerate(clouds)])
    if normalization == "":
        return model.predict(x).double()
    obb, _ = ops.obb_batch(x, check=False)
    xd = x.double()
    if normalization == "translation":
        y = model.predict(ops.normalize_batch(xd, obb, ops.NORM_TRANSLATE).float()).double()
        return (y.reshape(len(clouds), -1, 3) + obb[:, None, 9:12]).reshape(len(clouds), -1)
    from ..geometry import OrientedBoundingBox
    M = OrientedBoundingBox.get_rotation_matrix_from_yxz([0, 0, np.pi / 2])
    y = model.predict(ops.normalize_batch(xd, obb, ops.NORM_OBB_ROT_TRANS, M).float()).double()
    # y = (p - c) R M with R, M orthogonal: p = y (R M)^T + c
    RM = obb[:, :9].reshape(-1, 3, 3) @ torch.as_tensor(np.asarray(M, dtype=np.float64), device=obb.device)
    return (y.reshape(len(clouds), -1, 3) @ RM.transpose(1, 2) + obb[:, None, 9:12]).reshape(len(clouds), -1)

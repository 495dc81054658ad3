"""Host mirror of the reference's models/pointnet.py for inference: create_pointnet(number_of_points, number_of_joints) returns a
PointNet whose weights are laid out as Keras' model.get_weights() of the reference model (108 arrays) and whose forward pass is the
fused MI355X path (kpx_pointnet_forward; arithmetic contract AC18).  Batch normalisation runs on its moving
statistics and dropout is the identity; training stays outside this package.

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


class PointNet:
    """The reference's Keras model as far as inference goes: set_weights / get_weights / load_weights / save_weights / predict."""

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

    # ---- weights ------------------------------------------------------------------------------------------------------------------
    def get_weights(self):
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
        self._weights, self._packed = new, None

    def save_weights(self, path):
        """one .npz with the arrays under their names (weight_names())"""
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

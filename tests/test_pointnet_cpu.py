"""CPU suite of the PointNet joint regressor (AC18): the reference statements of tests/pointnet_ref.py judged against
torch's own layers and against each other, negative controls that give the deviation rule its teeth, the weight files, the argument
errors the C entries answer on the host, and the metrics' float32 tie rule.  Nothing here needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import pointnet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("kpx_pointnet_workspace_bytes", "kpx_pointnet_forward", "kpx_joint_metrics")
SMALL = [(1, 1, 1), (2, 17, 3), (5, 65, 32), (2, 200, 3)]                  # (B, N, J)
SCALES = (R.UNIT, R.MILLIMETRE)


# ---- 1. the unfolded float64 network against torch's layers and against the unrounded fold ---------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B, N, J", SMALL)
def test_unfolded_float64_agrees_with_torch_layers_and_with_the_unrounded_fold(B, N, J, scale):
    w = R.model(J)[0]
    x = R.case(B, N, J, scale)[0]
    mine = R.forward_unfolded(w, x)
    theirs = R.forward_torch64_unfolded(w, x)
    folded = R.forward_folded(R.fold(w, rounded=False), x, np.float64)
    for k in R.STAGES:
        assert mine[k].shape == theirs[k].shape == folded[k].shape
        assert R.rel_dev(mine[k], theirs[k]) <= 1e-12, k
        assert R.rel_dev(folded[k], mine[k]) <= 1e-12, k


def test_the_librarys_fold_is_the_references_bit_for_bit():
    from kinectpy_amd import ops
    w, folded = R.model(3)
    got = ops.pointnet_fold(w)
    assert len(got) == len(folded) == 20
    for (W, b), (Wr, br) in zip(got, folded):
        assert W.dtype == b.dtype == np.float32
        assert np.array_equal(W.view(np.uint32), Wr.view(np.uint32)) and np.array_equal(b.view(np.uint32), br.view(np.uint32))
    assert [(ci, co, bn) for ci, co, bn, _ in R.layer_shapes(3)] == ops.pointnet_layer_shapes(3)


# ---- 2. negative controls -------------------------------------------------------------------------------------------------------------------
def _miss(got, y64, tau):
    """per array: the deviation from the float64 reference in units of that array's tau"""
    return {k: R.rel_dev(got[k], y64[k]) / tau[k] for k in R.STAGES}


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B, N, J", SMALL)
def test_control_transposed_T_and_epsilon_miss_by_100_tau(B, N, J, scale):
    w, folded = R.model(J)
    x, y64, tau = R.case(B, N, J, scale)
    assert _miss(R.forward_folded(folded, x, np.float64, transpose_T=True), y64, tau)["joints"] >= 100
    assert _miss(R.forward_folded(R.fold(w, eps=1e-5), x, np.float64), y64, tau)["joints"] >= 100


@pytest.mark.parametrize("B, N, J", SMALL)
def test_control_one_bias_vector_times_1001_misses_by_100_tau_at_unit_scale(B, N, J):
    """unit coordinates only: at millimetre scale the activations are 10^3 times the biases and a relative change of a bias vanishes in
    the output scale.  The vector is the folded bias of layer 18 (256 -> 128)."""
    folded = list(R.model(J)[1])
    x, y64, tau = R.case(B, N, J, R.UNIT)
    folded[18] = (folded[18][0], folded[18][1] * np.float32(1.001))
    assert _miss(R.forward_folded(folded, x, np.float64), y64, tau)["joints"] >= 100


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B, J", [(1, 1), (2, 3), (5, 32)])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 65, 1000])
def test_control_one_extra_point_at_the_origin_misses_by_100_tau(B, N, J, scale):
    """what zero-filled rows of a partial tile would compute.  The control depends on the input: the clouds are centred away from the
    origin (checked here).  The rule is applied per array, so the control is caught where ANY array misses; the first maximum g1 sees the
    extra point directly and must miss in every case, the joints must miss at unit scale (at millimetre scale scale-relative effects
    shrink on the way to the output, as for the bias control)."""
    assert N % 64
    folded = R.model(J)[1]
    x, y64, tau = R.case(B, N, J, scale)
    assert np.linalg.norm(x.astype(np.float64).mean(axis=1), axis=1).min() > 2 * x.astype(np.float64).std(axis=1).max()
    miss = _miss(R.forward_folded(folded, np.concatenate([x, np.zeros((B, 1, 3), np.float32)], axis=1), np.float64), y64, tau)
    assert miss["g1"] >= 100 and max(miss.values()) >= 100
    if scale == R.UNIT:
        assert min(miss.values()) >= 100


# ---- 3. the reference is a function of the point SET --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_permuting_the_points_leaves_the_reference_unchanged(scale):
    folded = R.model(3)[1]
    x, y64, _ = R.case(2, 200, 3, scale)
    p = np.random.default_rng(5).permutation(200)
    again = R.forward_folded(folded, x[:, p], np.float64)
    for k in ("g1", "g2", "g3"):
        assert np.array_equal(again[k], y64[k]), k                        # a maximum of the same numbers
    for k in R.STAGES:
        assert R.rel_dev(again[k], y64[k]) <= 1e-12, k


def test_float32_restatements_spread_and_tau_is_of_float32_size():
    x, y64, tau = R.case(2, 200, 3, R.UNIT)
    outs = R.restatements32(R.model(3)[1], x)
    assert len(outs) >= 7
    devs = [R.rel_dev(o["joints"], y64["joints"]) for o in outs]
    assert len({d for d in devs}) > 1 and 0 < max(devs) < 1e-5
    assert tau["joints"] == R.MARGIN * max(devs)


# ---- 4. weights: files, counts, shapes ----------------------------------------------------------------------------------------------------------
def test_weights_round_trip_through_npz_in_both_key_styles(tmp_path):
    from kinectpy_amd.models.pointnet import PointNet, create_pointnet, weight_names, weight_shapes
    w = R.model(3)[0]
    m = create_pointnet(64, 3)
    assert isinstance(m, PointNet) and len(m.get_weights()) == 108 == len(weight_names()) == len(set(weight_names()))
    assert [a.shape for a in m.get_weights()] == weight_shapes(3) == [a.shape for a in w]
    # Keras' initial T-nets are the identity transform
    assert not m.get_weights()[30].any() and np.array_equal(m.get_weights()[31], np.eye(3, dtype=np.float32).reshape(-1))
    m.set_weights(w)
    named, positional = str(tmp_path / "named.npz"), str(tmp_path / "positional.npz")
    m.save_weights(named)
    np.savez(positional, *w)
    for path in (named, positional):
        m2 = create_pointnet(64, 3)
        m2.load_weights(path)
        assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(m2.get_weights(), w))
    assert sorted(np.load(named).files) == sorted(weight_names())


def test_weight_count_and_shape_errors_name_the_array(tmp_path):
    from kinectpy_amd import ops
    from kinectpy_amd.models.pointnet import create_pointnet
    w = R.model(3)[0]
    m = create_pointnet(64, 3)
    with pytest.raises(ValueError, match="108"):
        m.set_weights(w[:-1])
    bad = list(w)
    bad[13] = np.zeros((65,), np.float32)
    with pytest.raises(ValueError, match=r"array 13 \(tnet3/conv3/bias\)"):
        m.set_weights(bad)
    with pytest.raises(ValueError, match="array 13"):
        ops.pointnet_fold(bad)
    with pytest.raises(ValueError, match="108"):
        ops.pointnet_fold(w + [w[0]])
    short = str(tmp_path / "short.npz")
    np.savez(short, *w[:50])
    with pytest.raises(ValueError, match="arr_50"):
        m.load_weights(short)
    with pytest.raises(ValueError, match="joints"):                       # a model for another number of joints
        create_pointnet(64, 4).set_weights(w)
    with pytest.raises(ValueError):
        create_pointnet(64, 342)                                          # 3 J > 1024
    with pytest.raises(ValueError):
        create_pointnet(0, 3)


def test_names_and_the_public_surface():
    import inspect
    from kinectpy_amd import ops
    from kinectpy_amd.metrics import metric
    from kinectpy_amd.models import pointnet
    for name in ("pointnet_fold", "pointnet_pack", "pointnet_forward", "joint_metrics"):
        assert callable(getattr(ops, name))
    assert list(inspect.signature(pointnet.create_pointnet).parameters) == ["number_of_points", "number_of_joints"]
    assert list(inspect.signature(pointnet.predict_joints).parameters) == ["clouds", "model", "normalization", "sampler", "start_index", "seed"]
    assert inspect.signature(metric.percentual_correct_keypoints).parameters["threshold"].default == 150
    assert metric.percentual_correct_keypoints(150).__name__ == "percentual_correct_keypoints_150"
    assert metric.percentual_correct_keypoints(20).__name__ == "percentual_correct_keypoints_20"
    assert list(inspect.signature(metric.evaluate).parameters["thresholds"].default) == list(range(0, 210, 10))
    with pytest.raises(NotImplementedError):
        pointnet.predict_joints([], pointnet.create_pointnet(64, 3), normalization="obb_normalization")


def test_pack_layout_matches_the_header(monkeypatch):
    """every array at a multiple of 64 floats in layer order; the 64 -> 512 layers in the matrix instruction's operand order"""
    from kinectpy_amd import ops
    folded = R.model(3)[1]
    got = {}
    monkeypatch.setattr(ops, "_dev", lambda a, dtype: got.setdefault("buf", np.asarray(a)))
    buf = ops.pointnet_pack(folded)
    off = 0
    for l, (W, b) in enumerate(folded):
        n = W.size
        seg = buf[off:off + n]
        if l in (2, 10, 16):
            c, q, lane, e = np.meshgrid(np.arange(16), np.arange(8), np.arange(64), np.arange(4), indexing="ij")
            assert np.array_equal(seg.reshape(16, 8, 64, 4), W[2 * (4 * q + e) + (lane >> 5), 32 * c + (lane & 31)])
        else:
            assert np.array_equal(seg, W.reshape(-1))
        off += -(-n // 64) * 64
        assert np.array_equal(buf[off:off + b.size], b)
        off += -(-b.size // 64) * 64
    assert off == buf.size and ops._pn_joints_of(buf.size) == 3


# ---- 5. the ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_in_header_and_signatures():
    from kinectpy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "kinectpx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    for name, value in (("KPX_POINTNET_MAX_OUT", 1024), ("KPX_METRICS_MAX_THRESHOLDS", 64), ("KPX_VERSION", 100)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name


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
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.kpx_version() == 100
    dummy = C.c_void_p(4096)
    err = lambda: lib.kpx_last_error()
    floats = lambda J: sum(-(-ci * co // 64) * 64 + -(-co // 64) * 64 for ci, co, _, _ in R.layer_shapes(J))
    f3 = floats(3)
    assert ops._pn_joints_of(f3) == 3 and ops._pn_joints_of(floats(341)) == 341
    fwd = lambda w, wf, p, B, N, J, out, ws=dummy, wsz=1 << 30: lib.kpx_pointnet_forward(w, wf, p, B, N, J, out, None, None, None, None, None, ws, wsz, None)
    assert fwd(None, f3, dummy, 2, 64, 3, dummy) == -1 and b"null pointer" in err()
    assert fwd(dummy, f3, None, 2, 64, 3, dummy) == -1 and b"null pointer" in err()
    assert fwd(dummy, f3, dummy, 2, 64, 3, None) == -1 and b"null pointer" in err()
    assert fwd(dummy, f3, dummy, 2, 64, 3, dummy, None, 0) == -1 and b"null pointer" in err()
    assert fwd(dummy, f3, dummy, 2, 0, 3, dummy) == -1 and b"at least one point" in err()
    assert fwd(dummy, f3, dummy, 0, 0, 3, dummy) == -1                                       # N = 0 is rejected whatever the batch
    assert fwd(dummy, f3, dummy, 2, 64, 0, dummy) == -1 and b"joints" in err()
    assert fwd(dummy, floats(341), dummy, 2, 64, 341, dummy, dummy, 16) == -2               # 3 J = 1023 is in range: the workspace is next
    assert fwd(dummy, f3, dummy, 2, 64, 342, dummy) == -1 and b"1024" in err()
    assert fwd(dummy, f3, dummy, -1, 64, 3, dummy) == -1
    assert fwd(dummy, f3, dummy, 2 ** 15, 2 ** 16, 3, dummy) == -3 and b"2^31" in err()
    assert fwd(dummy, f3, dummy, 1, 2 ** 31, 3, dummy) == -3
    assert fwd(dummy, f3 + 64, dummy, 2, 64, 3, dummy) == -1 and b"packed weights" in err()
    assert fwd(C.c_void_p(4100), f3, dummy, 2, 64, 3, dummy) == -1 and b"aligned" in err()
    assert fwd(dummy, f3, dummy, 2, 64, 3, dummy, dummy, 16) == -2 and b"workspace too small" in err()
    assert fwd(None, f3, None, 0, 64, 3, None, None, 0) == 0                                 # an empty batch is a no-op
    q = lib.kpx_pointnet_workspace_bytes
    assert 0 < q(1, 64, 3) <= q(32, 64, 3) and q(32, 64, 3) == q(32, 4096, 3)
    assert q(2, 0, 3) == 0 and q(2, 64, 342) == 0 and q(2 ** 15, 2 ** 16, 3) == 0 and q(-1, 64, 3) == 0
    thr = (C.c_double * 2)(10.0, 20.0)
    met = lib.kpx_joint_metrics
    assert met(None, dummy, 10, thr, 2, dummy, dummy, None) == -1 and b"null pointer" in err()
    assert met(dummy, dummy, 10, thr, 2, None, dummy, None) == -1
    assert met(dummy, dummy, 10, thr, 2, dummy, None, None) == -1
    assert met(dummy, dummy, 10, None, 2, dummy, dummy, None) == -1
    assert met(dummy, dummy, -1, thr, 2, dummy, dummy, None) == -1
    assert met(dummy, dummy, 10, thr, 65, dummy, dummy, None) == -1 and b"at most 64" in err()


# ---- 6. metrics: the float32 comparison on ties ------------------------------------------------------------------------------------------------------
def metrics_case(seed=3, B=7, J=5):
    """values whose float32 difference is EXACTLY a threshold, one ulp above and one ulp below, mixed with general ones"""
    rng = np.random.default_rng(seed)
    yt = rng.normal(0, 200, (B, 3 * J)).astype(np.float32)
    yp = (yt + rng.normal(0, 80, yt.shape)).astype(np.float32)
    yt[0, :6] = [0, 100, -50, 1000, 0.5, 0]
    yp[0, :6] = [150, -50, 100, 1150, 150.5, -150]                                           # |diff| == 150 exactly
    yp[1, :3] = yt[1, :3] + np.float32(10)
    yp[1, 3] = np.nextafter(np.float32(150), np.float32(np.inf))
    yp[1, 4] = np.nextafter(np.float32(150), np.float32(0))
    yt[1, 3:5] = 0
    yp[2, :2], yt[2, :2] = yt[2, :2], yt[2, :2]                                              # difference 0: inside threshold 0
    return yt, yp


def numpy_metrics(yt, yp, thresholds):
    """the reference's float32 comparison and evaluate.py's mean squared error, the latter summed in float64"""
    d = np.asarray(yp, np.float32) - np.asarray(yt, np.float32)
    counts = [int((np.abs(d) <= np.float32(t)).sum()) for t in thresholds]
    return counts, float((d.astype(np.float64) ** 2).sum()), d.size


def test_tie_rule_of_the_numpy_statement():
    """the statement the GPU metrics are compared with: a difference of exactly the threshold counts, one float32 ulp more does not, and
    the comparison happens in float32 (a threshold that is not a float32 is rounded first)"""
    yt, yp = metrics_case()
    (c150, c0), _, n = numpy_metrics(yt, yp, [150, 0])
    d = np.abs(yp - yt)
    assert (d == 150).sum() == 6 and c150 == (d <= 150).sum() and c150 < n
    assert d[1, 3] > 150 and d[1, 4] < 150 and np.float32(d[1, 3]) - np.float32(d[1, 4]) < 1e-4          # one ulp either side of the threshold
    assert c0 == (d == 0).sum() >= 2
    t = 0.1                                                              # fl32(0.1) > 0.1: a difference of fl32(0.1) passes only in float32
    a, b = np.zeros(1, np.float32), np.full(1, np.float32(0.1))
    assert numpy_metrics(a, b, [t])[0] == [1] and not (np.abs(b.astype(np.float64)) <= t).any()

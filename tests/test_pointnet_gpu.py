"""GPU suite of the PointNet joint regressor (AC18).  The fused forward and every stage output are judged by the deviation
rule of tests/pointnet_ref.py: tau = 4 x the worst of the CPU float32 restatements against the float64 evaluation of the same folded
float32 weights, never against the code under test.  Sizes put partial tiles on both sides of every tile width (16 / 32 / 64-point
tiles: N = 15..17, 63..65), several tiles per cloud (1000, 4096) and both launch shapes (few tiles: the last layer's channels split over
several waves; many: one wave per tile).  Every case's reference is computed once (pointnet_ref.case) and shared.

Measured on MI355X (deviation / scale of the joints; tau of the case): see DESIGN.md 5.19."""
import functools

import numpy as np
import pytest
import torch

from tests import pointnet_ref as R
from tests.test_pointnet_cpu import metrics_case, numpy_metrics

pytestmark = pytest.mark.gpu

NS = [1, 15, 16, 17, 63, 64, 65, 1000, 4096]
BJ = [(1, 1), (2, 3), (5, 32)]
SCALES = (R.UNIT, R.MILLIMETRE)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


@functools.lru_cache(maxsize=None)
def packed(J, variant=""):
    from kinectpy_amd import ops
    folded = list(R.model(J)[1])
    if variant == "dead":                        # the main trunk's last layer can never fire: its folded bias is -10^3
        folded[16] = (folded[16][0], np.full(512, -1e3, np.float32))
    return ops.pointnet_pack(folded), folded


def run(J, x, variant=""):
    from kinectpy_amd import ops
    y, st = ops.pointnet_forward(packed(J, variant)[0], torch.as_tensor(np.array(x)).cuda(), want_stages=True)          # (a copy: the cases are read-only)
    got = {k: v.cpu().numpy() for k, v in st.items()}
    got["joints"] = y.cpu().numpy()
    return got


def check(got, y64, tau, label):
    B = y64["joints"].shape[0]
    for k in R.STAGES:
        assert got[k].dtype == np.float32 and got[k].shape == y64[k].shape, k
        dev = R.rel_dev(got[k], y64[k])
        print(f"{label} {k}: deviation {dev:.3e} of scale, tau {tau[k]:.3e}")
        assert np.isfinite(got[k]).all() and dev <= tau[k], (label, k, dev, tau[k], B)


# ---- forward and every stage output under the rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B, J", BJ)
@pytest.mark.parametrize("N", NS)
def test_forward_and_stage_outputs_within_tau(N, B, J, scale):
    x, y64, tau = R.case(B, N, J, scale)
    check(run(J, x), y64, tau, f"N={N} B={B} J={J} {scale}")


def test_plain_forward_equals_the_staged_one_and_numpy_input_is_accepted():
    """without stage outputs the maxima live in the workspace: the same bits"""
    from kinectpy_amd import ops
    x = np.array(R.case(2, 65, 3, R.UNIT)[0])
    y, _ = ops.pointnet_forward(packed(3)[0], torch.as_tensor(x).cuda(), want_stages=True)
    assert np.array_equal(_bits(ops.pointnet_forward(packed(3)[0], x)), _bits(y))


# ---- special clouds -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 17, 64, 200])
def test_cloud_of_identical_points(N):
    x1 = R.case(2, 1, 3, R.UNIT)[0]
    x = np.ascontiguousarray(np.repeat(x1, N, axis=1))
    y64, tau = R.reference(packed(3)[1], x)
    got = run(3, x)
    check(got, y64, tau, f"identical N={N}")
    one = run(3, x1)
    for k in R.STAGES:                           # a maximum over copies of one point is that point's value: the same bits as N = 1
        assert np.array_equal(got[k].view(np.uint32), one[k].view(np.uint32)), k


@pytest.mark.parametrize("N", [17, 64, 1000])
def test_all_negative_preactivations_give_plus_zero_and_a_head_driven_by_biases(N):
    x = R.case(2, N, 3, R.UNIT)[0]
    folded = packed(3, "dead")[1]
    y64, tau = R.reference(folded, x)
    assert not y64["g3"].any()
    got = run(3, x, "dead")
    assert np.array_equal(got["g3"].view(np.uint32), np.zeros((2, 512), np.uint32))             # exactly +0, not -0
    bias_only = R.forward_folded(folded, x, np.float64)["joints"]
    h = np.maximum(folded[17][1].astype(np.float64), 0)
    h = np.maximum(h @ folded[18][0].astype(np.float64) + folded[18][1], 0)
    assert R.rel_dev(bias_only, np.broadcast_to(h @ folded[19][0].astype(np.float64) + folded[19][1], bias_only.shape)) <= 1e-12
    for k in ("T3", "T32", "g1", "g2", "joints"):
        assert R.rel_dev(got[k], y64[k]) <= tau[k], k
    assert np.array_equal(got["joints"][0].view(np.uint32), got["joints"][1].view(np.uint32))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("N", [17, 65])
def test_partial_tiles_do_not_see_a_point_at_the_origin(N, scale):
    """the padding trap: the cloud passes the rule against ITS reference, the cloud with one more point at the origin -- what zero-filled
    padding rows would compute -- lies at least 100 tau away in g1, and that cloud passes against its own reference in turn"""
    folded = packed(3)[1]
    x, y64, tau = R.case(2, N, 3, scale)
    xo = np.concatenate([x, np.zeros((2, 1, 3), np.float32)], axis=1)
    yo64, tauo = R.reference(folded, xo)
    assert R.rel_dev(yo64["g1"], y64["g1"]) >= 100 * tau["g1"]
    check(run(3, x), y64, tau, f"N={N} {scale}")
    check(run(3, xo), yo64, tauo, f"N={N}+origin {scale}")


def test_non_finite_coordinates_do_not_fault():
    """the result is unspecified; the call must return and the device must stay usable"""
    x = np.array(R.case(2, 65, 3, R.UNIT)[0])
    x[0, 3] = [np.nan, np.inf, -np.inf]
    x[1, 64, 0] = np.inf
    got = run(3, x)
    assert got["joints"].shape == (2, 9)
    x2, y64, tau = R.case(2, 65, 3, R.UNIT)
    check(run(3, x2), y64, tau, "after non-finite")


def test_empty_batch_and_argument_errors():
    from kinectpy_amd import _lib, ops
    y, st = ops.pointnet_forward(packed(3)[0], torch.empty((0, 64, 3), dtype=torch.float32, device="cuda"), want_stages=True)
    assert y.shape == (0, 9) and st["T32"].shape == (0, 32, 32)
    with pytest.raises(_lib.KinectPxError, match="at least one point"):
        ops.pointnet_forward(packed(3)[0], torch.empty((2, 0, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        ops.pointnet_forward(packed(3)[0], torch.empty((2, 5, 2), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="not a packed PointNet"):
        ops.pointnet_forward(packed(3)[0][:-64], torch.empty((2, 5, 3), dtype=torch.float32, device="cuda"))


# ---- batching -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 1000])
def test_two_calls_are_bit_identical_and_a_batch_equals_its_clouds_run_singly(N):
    x = R.case(5, N, 32, R.MILLIMETRE)[0]
    a, b = run(32, x), run(32, x)
    for k in R.STAGES:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for c in range(5):                           # B = 1 takes the split launch shape at N = 17 and at N = 1000: the same values
        one = run(32, x[c:c + 1])
        for k in R.STAGES:
            assert np.array_equal(one[k][0].view(np.uint32), a[k][c].view(np.uint32)), (k, c)


def test_model_predict_is_the_operator_on_the_folded_packed_weights():
    from kinectpy_amd import ops
    from kinectpy_amd.models.pointnet import create_pointnet
    x = np.array(R.case(2, 64, 3, R.UNIT)[0])
    m = create_pointnet(64, 3)
    m.set_weights(R.model(3)[0])
    want = ops.pointnet_forward(packed(3)[0], x)
    assert np.array_equal(_bits(m.predict(x)), _bits(want)) and np.array_equal(_bits(m(torch.as_tensor(np.array(x)).cuda())), _bits(want))
    assert m.predict(x).dtype == torch.float32 and m.predict(x).is_cuda
    with pytest.raises(ValueError):
        m.predict(x[:, :63])


# ---- metrics ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, J", [(7, 5), (1, 1), (3000, 32)])
def test_joint_metrics_counts_are_numpys_and_the_loss_within_1e12(B, J):
    from kinectpy_amd import ops
    from kinectpy_amd.metrics.metric import percentual_correct_keypoints
    yt, yp = metrics_case(seed=B, B=max(B, 3), J=max(J, 2))
    thresholds = list(range(0, 210, 10)) + [0.1]
    counts, total, n = ops.joint_metrics(yt, yp, thresholds)
    rc, rt, rn = numpy_metrics(yt, yp, thresholds)
    assert n == rn and counts.dtype == torch.int64 and counts.cpu().tolist() == rc
    assert abs(float(total.cpu()[0]) - rt) <= 1e-12 * rt
    again = ops.joint_metrics(yt, yp, thresholds)
    assert float(again[1].cpu()[0]) == float(total.cpu()[0])                                   # a fixed summation order
    f = percentual_correct_keypoints(150)
    assert f(yt, yp) == rc[15] / rn and f(torch.as_tensor(yt).cuda(), torch.as_tensor(yp).cuda()) == rc[15] / rn
    assert percentual_correct_keypoints()(yt, yp) == rc[15] / rn


def test_evaluate_reports_loss_and_pck_as_evaluate_py():
    from kinectpy_amd.metrics.metric import evaluate
    from kinectpy_amd.models.pointnet import create_pointnet
    x = np.array(R.case(5, 64, 32, R.UNIT)[0])
    m = create_pointnet(64, 32)
    m.set_weights(R.model(32)[0])
    pred = m.predict(x).cpu().numpy()
    y = (pred + np.random.default_rng(2).normal(0, 0.05, pred.shape)).astype(np.float32)
    thresholds = [0.0, 0.02, 0.05, 0.1, 150]
    out = evaluate(m, x, y, thresholds)
    rc, rt, rn = numpy_metrics(y, pred, thresholds)
    assert set(out) == {"loss", "pck"} and list(out["pck"]) == thresholds
    assert [out["pck"][t] for t in thresholds] == [c / rn for c in rc] and out["pck"][150] == 1.0
    assert abs(out["loss"] - rt / rn) <= 1e-12 * rt / rn
    assert list(evaluate(m, x, y)["pck"]) == list(range(0, 210, 10))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------
def test_predict_joints_translation_equals_the_chain_by_hand(base_cloud):
    from kinectpy_amd import ops
    from kinectpy_amd.models.pointnet import create_pointnet, predict_joints
    rng = np.random.default_rng(11)
    base = np.asarray(base_cloud, np.float32).reshape(-1, 3)
    clouds = [np.ascontiguousarray(base[rng.permutation(len(base))[:3000 + 500 * i]] + np.float32(40 * i)) for i in range(3)]
    m = create_pointnet(256, 3)
    m.set_weights(R.model(3)[0])
    got = predict_joints(clouds, m, normalization="translation", sampler="farthest", start_index=0)
    assert got.shape == (3, 9) and got.is_cuda
    # by hand: sample -> gather -> the translation normaliser -> forward -> centre added back
    sel, _ = ops.farthest_point_sample_batch(clouds, 256, 0)
    x = np.stack([c[s] for c, s in zip(clouds, sel.cpu().numpy())])
    obb, _ = ops.obb_batch(torch.as_tensor(x).cuda())
    xn = ops.normalize_batch(torch.as_tensor(x).cuda().double(), obb, ops.NORM_TRANSLATE).float()
    yn = ops.pointnet_forward(m.packed(), xn).cpu().numpy()
    y = yn.astype(np.float64).reshape(3, 3, 3) + obb.cpu().numpy()[:, None, 9:12]
    assert np.array_equal(got.cpu().numpy(), y.reshape(3, 9))
    y64, tau = R.reference(R.model(3)[1], xn.cpu().numpy())
    assert R.rel_dev(yn, y64["joints"]) <= tau["joints"]
    # the rotation normaliser's inverse map: normalising the returned joints again gives the forward's own output.  Two fp64 3x3 products
    # and a translation on values up to ~4e3 (the centres, in millimetres): 1e-9 absolute is generous by four orders and far below float32
    from kinectpy_amd.geometry import OrientedBoundingBox
    M = OrientedBoundingBox.get_rotation_matrix_from_yxz([0, 0, np.pi / 2])
    rot = predict_joints(clouds, m, normalization="obb_rotation_translation")
    assert rot.shape == (3, 9) and torch.isfinite(rot).all()
    xr = ops.normalize_batch(torch.as_tensor(x).cuda().double(), obb, ops.NORM_OBB_ROT_TRANS, M).float()
    yr = ops.pointnet_forward(m.packed(), xr).double().cpu().numpy()
    back = ops.normalize_batch(rot.reshape(3, 3, 3), obb, ops.NORM_OBB_ROT_TRANS, M).cpu().numpy().reshape(3, 9)
    assert np.abs(back - yr).max() <= 1e-9 * max(1.0, np.abs(yr).max())
    with pytest.raises(NotImplementedError):
        predict_joints(clouds, m, normalization="obb_normalization")
    rnd = predict_joints(clouds, m, normalization="translation", sampler="random", seed=5)
    assert np.array_equal(rnd.cpu().numpy(), predict_joints(clouds, m, normalization="translation", sampler="random", seed=5).cpu().numpy())

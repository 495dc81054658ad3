"""Host suite for ISS keypoints: the NumPy restatement (tests/iss_ref.py) on cases with known answers, the Python surface that
needs no GPU, and the exclusion caps of every input tests/test_iss_gpu.py uses."""
import inspect

import numpy as np
import pytest

from tests import iss_ref as R

NEXT1 = float(np.nextafter(1.0, 2.0))


def _sal(pts, r, **kw):
    pts = np.asarray(pts, dtype=np.float32)
    return R.saliency(pts, R.radius_pairs(pts, r), **kw)


def test_flat_integer_lattice_has_no_keypoints():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(9), [4], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    sal = _sal(g, 2.5)
    assert np.all(sal["count"][(g[:, 0] > 2) & (g[:, 0] < 9) & (g[:, 1] > 2) & (g[:, 1] < 6)] == 21)
    assert np.all(np.abs(np.nan_to_num(sal["e"][:, 0])) < 1e-12) and np.all(np.abs(sal["s"]) < 1e-12)
    assert len(R.iss_keypoints(g, 2.5, 2.5)["idx"]) == 0


def test_single_point_duplicates_and_too_few_points():
    assert _sal([[1, 2, 3]], 1.0, min_neighbors=0)["s"].tolist() == [0.0]
    dup = np.tile([[0.5, -1.0, 8.0]], (40, 1))
    sal = _sal(dup, 1.0)
    assert np.all(sal["count"] == 40) and np.all(sal["s"] == 0) and np.all(np.isnan(sal["e"]))
    assert len(R.iss_keypoints(dup)["idx"]) == 0 and len(R.iss_keypoints(np.zeros((0, 3)))["idx"]) == 0
    four = np.random.default_rng(0).normal(size=(4, 3))
    assert np.all(_sal(four, 100.0)["s"] == 0) and np.all(_sal(four, 100.0, min_neighbors=4, gamma_21=2.0, gamma_32=2.0)["s"] > 0)


def test_hand_computed_five_points():
    """(0,0,0), (+-2,0,0), (0,+-1,0) lifted by z = (0, 1, 1, 0, 0) / 2: means (0, 0, 0.2); C = diag(8/5, 2/5, 0.06)"""
    pts = np.array([[0, 0, 0], [2, 0, 0.5], [-2, 0, 0.5], [0, 1, 0], [0, -1, 0]], np.float32)
    sal = _sal(pts, 10.0)
    assert np.all(sal["count"] == 5)
    assert np.allclose(sal["e"], [[0.06, 0.4, 1.6]] * 5, rtol=0, atol=1e-15)
    assert np.allclose(sal["s"], 0.06, rtol=0, atol=1e-15) and np.all(sal["decided"])
    assert np.all(_sal(pts, 10.0, gamma_21=0.25)["s"] == 0) and np.all(_sal(pts, 10.0, gamma_32=0.15)["s"] == 0)
    assert np.all(_sal(pts, 10.0, gamma_21=0.25 + 1e-12)["s"] > 0)
    # strict radius: the centre sees the points at distance 1 only beyond r = 1
    assert _sal(pts, 1.0)["count"].tolist() == [1, 1, 1, 1, 1] and _sal(pts, NEXT1)["count"].tolist() == [3, 1, 1, 2, 2]
    # suppression: equal saliencies survive together, a larger neighbour suppresses, zeros and negatives never survive
    pairs = R.radius_pairs(pts, 10.0)
    assert R.nonmax(np.full(5, 0.06), 5, pairs, 5)[0].all() and not R.nonmax(np.full(5, 0.06), 5, pairs, 6)[0].any()
    keep, gap = R.nonmax(np.array([0.1, 0.3, 0.3, 0.0, -1.0]), 5, pairs, 1)
    assert keep.tolist() == [False, True, True, False, False] and gap.tolist() == [0.1, 0.0, 0.0, 0.1, 1.0]


def test_resolution_is_the_mean_second_distance():
    pts = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [3, 0, 0]], np.float32)
    assert R.resolution(pts) == (1 + 1 + 0 + 0) / 4 and R.resolution(pts[:1]) == 0.0


def test_feature_select_by_index_on_the_host():
    import torch
    from kinectpy_amd import o3d
    data = np.arange(7 * 33, dtype=np.float64).reshape(7, 33)
    fe = o3d.pipelines.registration.Feature(torch.as_tensor(data))
    assert np.array_equal(fe.select_by_index([4, 1]).data, data[[1, 4]].T)
    assert np.array_equal(fe.select_by_index(np.array([[4], [1], [4]])).data, data[[1, 4]].T)
    assert np.array_equal(fe.select_by_index([4, 1], invert=True).data, data[[0, 2, 3, 5, 6]].T)
    assert fe.select_by_index([]).num() == 0 and fe.select_by_index([], invert=True).num() == 7
    with pytest.raises(RuntimeError):
        fe.select_by_index([7])


def test_namespace_and_defaults():
    from kinectpy_amd import o3d, ops
    from kinectpy_amd.geometry import PointCloud
    want = [("salient_radius", 0.0), ("non_max_radius", 0.0), ("gamma_21", 0.975), ("gamma_32", 0.975), ("min_neighbors", 5)]
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    assert sig(o3d.geometry.keypoint.compute_iss_keypoints) == [("input", inspect._empty)] + want
    assert sig(ops.iss_keypoints)[:6] == [("pts", inspect._empty)] + want
    assert sig(PointCloud._iss_keypoint_indices) == [("self", inspect._empty)] + want
    assert sig(ops.iss_saliency) == [("pts", inspect._empty), ("salient_radius", inspect._empty)] + want[2:]
    assert sig(ops.iss_nonmax) == [("pts", inspect._empty), ("saliency", inspect._empty), ("non_max_radius", inspect._empty), ("min_neighbors", 5)]
    assert sig(o3d.pipelines.registration.Feature.select_by_index) == [("self", inspect._empty), ("indices", inspect._empty), ("invert", False)]


def test_keypoints_none_leaves_registration_as_it_was(monkeypatch):
    from kinectpy_amd.preprocessing import data, registration
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    assert sig(registration.execute_global_registration) == [("pcd_master", inspect._empty), ("pcd_sub", inspect._empty), ("voxel_size", 35),
                                                              ("ransac_n_trials", 15), ("seed", None)]
    assert registration.execute_global_registration.__kwdefaults__ == {"keypoints": None}          # keyword-only, behind the shown signature
    init = inspect.signature(data.DataProcessor.__init__).parameters
    assert init["keypoints"].default is None and init["keypoints"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(data.DataProcessor.in_memory).parameters["keypoints"].default is None
    assert inspect.signature(registration.execute_multiway_registration).parameters["keypoints"].default is None
    # behaviour: without keypoints the clouds and features of prepare_dataset reach the RANSAC untouched and no ISS call is made
    seen = []
    tokens = tuple(object() for _ in range(6))
    monkeypatch.setattr(registration, "prepare_dataset", lambda *a, **k: tokens)
    monkeypatch.setattr(registration, "_cut_to_keypoints", lambda *a, **k: pytest.fail("ISS called without keypoints"))

    class Result:
        fitness, transformation = 0.5, "T"
    monkeypatch.setattr(registration.o3d.pipelines.registration, "registration_ransac_based_on_feature_matching",
                        lambda *a, **k: seen.append((a[:4], k["seed"])) or Result())
    for kwargs in ({}, {"keypoints": None}, {"keypoints": False}):
        seen.clear()
        assert registration.execute_global_registration("m", "s", 35, 2, seed=7, **kwargs) == "T"
        assert seen == [((tokens[2], tokens[3], tokens[4], tokens[5]), 7), ((tokens[2], tokens[3], tokens[4], tokens[5]), 8)]
    # DataProcessor hands its option down
    calls = []
    monkeypatch.setattr(data, "execute_global_registration", lambda m, s, **k: calls.append(k) or np.eye(4))
    monkeypatch.setattr(data, "execute_point_to_plane_registration", lambda m, s, init, **k: init)
    data.DataProcessor.in_memory(2, seed=3).find_registration_transforms("m", ["s"])
    data.DataProcessor.in_memory(2, seed=3, keypoints=True).find_registration_transforms("m", ["s"])
    assert calls == [{"seed": 3, "keypoints": None}, {"seed": 3, "keypoints": True}]


@pytest.mark.parametrize("name,factor", R.PARITY_CASES)
def test_reference_alone_stays_within_the_exclusion_caps(base_cloud, name, factor):
    pts, r, pairs, ref = R.parity_reference(name, factor, base_cloud)
    dec = ref["decided"]
    assert (~dec).sum() <= 0.01 * len(pts)
    assert (dec & (ref["s"] == 0)).any() and (dec & (ref["s"] != 0)).any()
    if factor > 40:
        assert ref["count"].mean() > 1100
    elif factor < 1:
        assert 0.3 < ref["count"].mean() - 1 < 1.0
    else:
        assert 20 < ref["count"].mean() < 40


@pytest.mark.parametrize("shape,rs,rn,seed", [c + (6,) for c in R.SLAB_CASES[:1]] + [(R.SLAB_DEFAULT, 0.0, 0.0, 4)])
def test_end_to_end_inputs_keep_the_unsafe_cap(shape, rs, rn, seed):
    """(the 65860-point slab's reference takes several seconds: its cap is asserted where it is used, in tests/test_iss_gpu.py)"""
    pts = R.bumpy_slab(*shape, seed=seed)
    ref = R.iss_keypoints(pts, rs, rn)
    safe = R.safe_points(ref, pts)
    assert (~safe).sum() <= 0.02 * len(pts)
    assert (safe & ref["keep"]).any() and (safe & ~ref["keep"] & (ref["sal"]["s"] > 0)).any()

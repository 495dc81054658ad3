"""GPU suite of the normal orientation and the Euclidean minimum spanning tree (AC17): exact equality against the
serial reference tests/orient_ref.py for signs, flip flags, EMST rows and orientation-tree rows.  Coordinates on the 1/16 grid give
heavy d2 ties, normals on the 1/1024 grid give weight ties and exact dot products; on general float clouds the reference's fma makes
d2 exact too.  Every cloud's reference EMST and kNN rows are computed once and shared."""
import functools

import numpy as np
import pytest
import torch

from tests import orient_ref as R
from tests import search_ref

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def quantised_normals(rng, n):
    return (rng.integers(-1024, 1025, (n, 3)) / 1024.0).astype(np.float32)


# ---- elementwise ---------------------------------------------------------------------------------------------------------------------------
def elementwise_case(n, seed):
    """general float normals with zero normals, -0.0 components and (camera) points that coincide with the camera mixed in"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    cam = np.array([0.5, -1.25, 2.0])
    if n:
        nrm[rng.random(n) < 0.2] = 0.0
        nrm[rng.random(n) < 0.2, 1] = -0.0
        nrm[rng.random(n) < 0.1, :2] = 0.0
        p[rng.random(n) < 0.2] = cam.astype(np.float32)
        nrm[0], p[0] = 0.0, cam                            # zero normal at the camera: (0, 0, 1)
    return p, nrm, cam


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_elementwise_bit_for_bit(n):
    from kinectpy_amd import ops
    p, nrm, cam = elementwise_case(n, 10 + n)
    dev = lambda a: torch.as_tensor(a).cuda()
    got = ops.orient_normals(dev(nrm), "normalize").cpu().numpy()
    assert np.array_equal(_bits(got), _bits(R.normalize(nrm)))
    ref = (0.25, -1.0, 0.5)
    got = ops.orient_normals(dev(nrm), "direction", ref).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(R.align_with_direction(nrm, ref)))
    t = dev(nrm)
    got = ops.orient_normals(t, "camera", cam, dev(p))
    assert got.data_ptr() == t.data_ptr()                                  # in place
    got, want = got.cpu().numpy(), R.towards_camera(p, nrm, cam)
    zero = ~np.any(nrm.astype(np.float64) != 0, axis=1)
    assert np.array_equal(_bits(got[~zero]), _bits(want[~zero]))
    # the zero-normal branch r / |r|: one rounding to float32 of an fp64 value whose own error is far below a float32 ulp
    assert np.all(np.abs(got[zero].astype(np.float64) - want[zero]) <= np.spacing(np.abs(want[zero])))
    if n:
        assert zero[0] and np.array_equal(got[0], [0, 0, 1])


# ---- EMST and tangent plane ------------------------------------------------------------------------------------------------------------------
def _clouds():
    rng = np.random.default_rng(20)
    q = lambda n, lo, hi: search_ref.quantised(rng, n, lo, hi)
    c = {}
    for n in (1, 2, 3, 65):
        c[f"q{n}"] = q(n, -1, 1)
    c["q700"] = q(700, -2, 2)
    c["float300"] = rng.normal(size=(300, 3)).astype(np.float32)
    c["blobs"] = np.concatenate([q(150, -1, 1), q(150, -1, 1) + np.float32([40, 0, 0])])          # k-closed components: the unbounded search
    d = q(200, -1, 1)
    d[rng.integers(0, 200, 60)] = d[rng.integers(0, 200, 60)]                                       # duplicated points: d2 = 0, ordered by index
    c["dups"] = d
    line = np.zeros((500, 3), np.float32)
    line[:, 0] = np.arange(500) * 0.25                                                              # all ties, a tree of depth n
    c["line"] = line
    flat = q(300, -1, 1)
    flat[:, 2] = np.minimum(flat[:, 2], np.float32(0.5))                                            # the maximal z is shared: root rule
    c["flat"] = flat
    c["cube"] = R.cube(top_sign=-1.0)[0]
    return c


CLOUDS = _clouds()
KS = {"q1": [0, 1, 8], "q2": [0, 1, 2, 8], "q3": [0, 1, 2, 8], "q65": [0, 1, 2, 8, 33, 70], "q700": [0, 1, 2, 8, 33, 705], "float300": [1, 8, 33],
      "blobs": [2, 8, 33], "dups": [1, 2, 8], "line": [0, 2, 8], "flat": [2, 8], "cube": [2, 8]}
CASES = [(name, k) for name, ks in KS.items() for k in ks]


def normals_of(name):
    if name == "cube":
        return R.cube(top_sign=-1.0)[1]
    n = len(CLOUDS[name])
    nrm = quantised_normals(np.random.default_rng(len(name) + n), n)
    if name in ("q65", "dups", "flat"):
        nrm[3] = 0.0                                                                                # a zero normal: c == 0 with everybody (the host walk)
    return nrm


@functools.lru_cache(maxsize=None)
def ref_emst(name):
    p = CLOUDS[name]
    return R.emst(p) if len(p) > 1 else np.zeros((0, 2), np.int32)


@functools.lru_cache(maxsize=None)
def ref_rows(name):
    return R.knn_rows(CLOUDS[name], max(KS[name]))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name, k", CASES)
def test_emst_rows_equal_the_reference(name, k):
    from kinectpy_amd import ops
    p = CLOUDS[name]
    edges, stats = ops.emst(dev(p), k, want_stats=True)
    assert edges.dtype == torch.int32 and tuple(edges.shape) == (max(len(p) - 1, 0), 2)
    assert np.array_equal(edges.cpu().numpy(), ref_emst(name))
    if len(p) > 1 and k <= 1:                              # every point's row is used up in every round: the exact search alone
        assert stats["bounded_searches"] + stats["unbounded_searches"] >= len(p)
    if name == "blobs" and k < 150:
        assert stats["unbounded_searches"] > 0
    if len(p) > 1:
        assert 1 <= stats["emst_rounds"] <= int(np.ceil(np.log2(len(p)))) + 1


@pytest.mark.parametrize("name, k", CASES)
def test_tangent_plane_equals_the_reference(name, k):
    from kinectpy_amd import ops
    p, nrm = CLOUDS[name], normals_of(name)
    n = len(p)
    rows = ref_rows(name)[:, :min(k, n)]
    want, want_flips, want_tree = R.tangent_from_graph(p, nrm, ref_emst(name), rows)
    t = dev(nrm)
    got, flips, tree, stats = ops.orient_normals_tangent(dev(p), t, k, want_flips=True, want_tree=True, want_stats=True)
    assert got.data_ptr() == t.data_ptr()
    assert np.array_equal(tree.cpu().numpy(), want_tree)
    assert np.array_equal(flips.cpu().numpy(), want_flips)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    if name == "cube":
        assert stats["zero_edges"] > 0 and np.array_equal(want, R.cube(top_sign=1.0)[1])
    if name == "flat":
        assert np.sum(p[:, 2] == p[:, 2].max()) > 1 and got[R.root_of(p), 2].item() >= 0
    # the optional outputs are optional
    again = ops.orient_normals_tangent(dev(p), dev(nrm), k)
    assert again[1] is None and again[2] is None and np.array_equal(_bits(again[0].cpu().numpy()), _bits(want))


def test_large_float_cloud_against_scipy_and_its_own_graph():
    """beyond one block and through many rounds: about 20 000 points of a noisy sphere.  EMST: SciPy's minimum spanning tree over the
    Delaunay edges weighted by the reference d2 (pairwise distinct, so that tree is unique).  T and the signs: the reference's
    Kruskal and walk on the library's own EMST and search_knn rows, so that nothing here is O(n^2)."""
    from kinectpy_amd import ops
    n, k = 20011, 8
    p, nrm = R.noisy_sphere(n, 30)
    p = (p.astype(np.float64) * (1.0 + 0.05 * np.random.default_rng(31).normal(size=(n, 1)))).astype(np.float32)
    de = R.delaunay_edges(p)
    w = R.d2_pairs(p, de[:, 0], de[:, 1])
    assert len(np.unique(w)) == len(w)
    edges, stats = ops.emst(dev(p), k, want_stats=True)
    edges = edges.cpu().numpy()
    assert np.array_equal(edges, edges[np.lexsort((edges[:, 1], edges[:, 0]))])
    assert {(int(a), int(b)) for a, b in edges} == R.scipy_mst(n, de[:, 0], de[:, 1], w)
    assert stats["emst_rounds"] <= 16
    idx, _, cnt = ops.search_knn(ops.search_index(dev(p)), dev(p), k)
    assert int(cnt.min()) == k
    want, want_flips, want_tree = R.tangent_from_graph(p, nrm, edges, idx.cpu().numpy())
    got, flips, tree = ops.orient_normals_tangent(dev(p), dev(nrm), k, want_flips=True, want_tree=True)
    assert np.array_equal(tree.cpu().numpy(), want_tree)
    assert np.array_equal(flips.cpu().numpy(), want_flips)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    side = np.sign(R.dot(got.cpu().numpy(), p))
    assert np.mean(side == 1) > 0.999                      # what it is for: the sphere comes out outward


# ---- methods -----------------------------------------------------------------------------------------------------------------------------------
def _cloud(p, nrm=None):
    from kinectpy_amd.geometry import PointCloud
    pc = PointCloud(p)
    if nrm is not None:
        pc.normals = nrm
    return pc


def test_point_cloud_methods_end_to_end():
    p, nrm, cam = elementwise_case(1000, 40)
    got = lambda pc: np.asarray(pc.normals).astype(np.float32)
    pc = _cloud(p, nrm)
    assert pc.normalize_normals() is pc and np.array_equal(_bits(got(pc)), _bits(R.normalize(nrm)))
    pc = _cloud(p, nrm)
    assert pc.orient_normals_to_align_with_direction() is pc and np.array_equal(_bits(got(pc)), _bits(R.align_with_direction(nrm)))
    pc = _cloud(p, nrm)
    assert pc.orient_normals_to_align_with_direction((0, -1, 0)) is pc and np.array_equal(_bits(got(pc)), _bits(R.align_with_direction(nrm, (0, -1, 0))))
    some = np.any(nrm != 0, axis=1)
    pc = _cloud(p, nrm)
    assert pc.orient_normals_towards_camera_location(cam) is pc and np.array_equal(_bits(got(pc)[some]), _bits(R.towards_camera(p, nrm, cam)[some]))
    pc = _cloud(p, nrm)
    assert pc.orient_normals_towards_camera_location() is pc and np.array_equal(_bits(got(pc)[some]), _bits(R.towards_camera(p, nrm)[some]))
    name = "q700"
    pc = _cloud(CLOUDS[name], normals_of(name))
    want = R.tangent_from_graph(CLOUDS[name], normals_of(name), ref_emst(name), ref_rows(name)[:, :8])[0]
    assert pc.orient_normals_consistent_tangent_plane(8) is pc and np.array_equal(_bits(got(pc)), _bits(want))


def test_methods_raise_without_normals_and_for_unbuilt_parameters():
    from kinectpy_amd.geometry import PointCloud
    pc = _cloud(CLOUDS["q65"])
    for call in (pc.normalize_normals, pc.orient_normals_to_align_with_direction, pc.orient_normals_towards_camera_location,
                 lambda: pc.orient_normals_consistent_tangent_plane(8)):
        with pytest.raises(RuntimeError, match="no normals"):
            call()
    pc = _cloud(CLOUDS["q65"], normals_of("q65"))
    with pytest.raises(NotImplementedError):
        pc.orient_normals_consistent_tangent_plane(8, 1.0)
    with pytest.raises(NotImplementedError):
        pc.orient_normals_consistent_tangent_plane(8, 0.0, 0.9)
    with pytest.raises(RuntimeError):
        pc.orient_normals_consistent_tangent_plane(4097)
    with pytest.raises(RuntimeError):
        pc.orient_normals_consistent_tangent_plane(-1)
    empty = PointCloud()
    assert empty.normalize_normals() is empty and empty.orient_normals_to_align_with_direction() is empty
    assert empty.orient_normals_towards_camera_location() is empty and empty.orient_normals_consistent_tangent_plane(8) is empty


def test_fusion_helper_orients_every_cloud_to_its_own_sensor():
    from kinectpy_amd.preprocessing.fusion import orient_normals_to_sensors
    Ts = []
    for s in range(1, 3):
        T = np.eye(4)
        T[:3, 3] = [2.0 * s, -1.0, 0.5 * s]
        Ts.append(T)
    data = [elementwise_case(300 + s, 50 + s)[:2] for s in range(3)]
    pcds = [_cloud(p, nrm) for p, nrm in data]
    assert orient_normals_to_sensors(pcds, Ts) is pcds
    for (p, nrm), pc, T in zip(data, pcds, [np.eye(4)] + Ts):
        some = np.any(nrm != 0, axis=1)
        got = np.asarray(pc.normals).astype(np.float32)
        assert np.array_equal(_bits(got[some]), _bits(R.towards_camera(p, nrm, T[:3, 3])[some]))
    again = [_cloud(p, nrm) for p, nrm in data]
    orient_normals_to_sensors(again, [np.eye(4)] + Ts)                     # S transforms, the master's first
    assert all(np.array_equal(np.asarray(a.normals), np.asarray(b.normals), equal_nan=True) for a, b in zip(again, pcds))
    with pytest.raises(RuntimeError):
        orient_normals_to_sensors(pcds, Ts[:1])


def test_results_do_not_depend_on_the_run_or_on_the_row_width():
    from kinectpy_amd import ops
    p, nrm = CLOUDS["q700"], normals_of("q700")
    runs = [ops.orient_normals_tangent(dev(p), dev(nrm), 8, want_flips=True, want_tree=True) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # the EMST works from rows of any width: 8, 33, or none at all
    trees = [ops.emst(dev(p), k).cpu().numpy() for k in (8, 33, 0, 8)]
    assert all(np.array_equal(trees[0], t) for t in trees[1:])
    # the same rows reached as a wider search cut to 8: the graph, and so T, is the same
    idx33, _, _ = ops.search_knn(ops.search_index(dev(p)), dev(p), 33)
    want = R.tangent_from_graph(p, nrm, trees[0], idx33[:, :8].cpu().numpy())
    assert np.array_equal(runs[0][2].cpu().numpy(), want[2]) and np.array_equal(runs[0][1].cpu().numpy(), want[1])

"""No GPU: the registry of tests/object_state.py classifies every public method and property of the geometry classes, names nothing
that does not exist, and its sources and mutators reach every callable that returns or changes a cloud or a mesh."""
import numpy as np
import pytest
import torch

import object_state as S


@pytest.mark.parametrize("name", sorted(S.CLASSES))
def test_every_public_callable_is_classified_and_every_entry_names_one(name):
    cls, entries = S.CLASSES[name], S.CLASSIFIED[name]
    public = S.public_names(cls)
    assert len(public) >= 5, public
    missing = sorted(public - set(entries))
    assert not missing, f"{name}: public methods / properties without a classification in tests/object_state.py: {missing}"
    stale = sorted(set(entries) - public)
    assert not stale, f"{name}: classified names that the class does not have (any more): {stale}"
    assert set(entries.values()) <= set(S.KINDS)
    for n, kind in entries.items():
        attr = vars(cls).get(n, getattr(cls, n))
        if isinstance(attr, property):
            assert (kind == "mutates_self") == (attr.fset is not None), f"{name}.{n}: a property is classified by its setter"


def test_classes_and_classification_cover_each_other():
    assert sorted(S.CLASSES) == sorted(S.CLASSIFIED)
    assert set(S.ELSEWHERE) <= set(S.CLASSES)


@pytest.mark.parametrize("name, sources, mutators", [("PointCloud", S.CLOUD_SOURCES, S.CLOUD_MUTATORS), ("TriangleMesh", S.MESH_SOURCES, S.MESH_MUTATORS)])
def test_the_matrix_reaches_every_callable_that_returns_or_changes_an_object(name, sources, mutators):
    entries = S.CLASSIFIED[name]
    for group, kinds in ((sources, ("returns_new", "mutates_self")), (mutators, ("mutates_self",))):
        assert len({e.name for e in group}) == len(group), "two entries of one name"
        for e in group:
            assert e.uses and callable(e[2]), e.name
            for u in e.uses:
                assert u in entries or callable(S.HELPERS.get(u)), f"{e.name}: uses {u!r}, which names nothing"
                assert u not in entries or entries[u] in ("returns_new", "mutates_self"), (e.name, u, entries[u])
    used_s = {u for e in sources for u in e.uses}
    used_m = {u for e in mutators for u in e.uses}
    elsewhere = S.ELSEWHERE.get(name, {})
    assert set(elsewhere) <= set(entries)
    for n, kind in entries.items():
        if kind == "returns_new":
            assert n in used_s or n in elsewhere, f"{name}.{n} returns an object and no source obtains one from it"
        if kind == "mutates_self":
            assert n in used_m, f"{name}.{n} works in place and no mutator applies it"
    if name == "PointCloud":                                 # the helpers all take clouds
        for h in S.HELPERS:
            assert h in used_s | used_m, h


def test_elsewhere_names_tests_that_exist():
    import ast
    import os
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_object_state_gpu.py")).read())
    tests = {f.name for f in tree.body if isinstance(f, ast.FunctionDef)}
    for per_class in S.ELSEWHERE.values():
        assert set(per_class.values()) <= tests, set(per_class.values()) - tests


def test_matrix_cells_are_the_legal_pairs():
    cells = S.pairs(S.CLOUD_SOURCES, S.CLOUD_MUTATORS)
    assert "b.points = a.points -> transform" in cells and "e + a -> transform" in cells and "e += a -> transform" in cells
    assert "b.normals = a.normals -> normalize_normals" in cells and "b.normals = a.normals -> orient_normals_to_align_with_direction" in cells
    assert "PointCloud(a.points) -> normalize_normals" not in cells and "PointCloud(a.points) -> transform" in cells
    assert "m2.triangles = m1.triangles -> orient_triangles" in S.pairs(S.MESH_SOURCES, S.MESH_MUTATORS)


def test_fixtures_are_what_the_suite_says():
    h = S.cloud_arrays()
    assert h["points"].shape == (257, 3) and h["points"].dtype == np.float32 and len(np.unique(h["points"], axis=0)) == 257
    assert np.array_equal(h["points"], np.round(h["points"])) and (np.linalg.norm(h["normals"], axis=1) == 0).sum() == 3
    assert np.linalg.eigvalsh(h["covariances"]).min() > 0 and np.array_equal(h["covariances"], h["covariances"].transpose(0, 2, 1))
    m, f = S.mesh_arrays(), S.mesh_arrays(flipped=S.FLIPPED)
    assert m["vertices"].shape == (66, 3) and m["triangles"].shape == (128, 3)
    p = m["vertices"].astype(np.float64) - np.array([10.0, 20.0, 30.0])
    t = m["triangles"]
    signed = np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]]))
    assert (signed > 0).all(), "the mesh is wound outward"
    edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all(), "and closed"
    assert sorted(np.flatnonzero((f["triangles"] != t).any(1))) == sorted(S.FLIPPED)
    T = S.rigid()
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-15) and np.abs(T[:3, 3]).min() > 800.0


class _Holder:
    __module__ = "kinectpy_amd.fake"

    def __init__(self, t):
        self.buf = t


def test_reachability_and_overlap_on_host_tensors():
    class Obj:
        pass
    base = torch.zeros(64, dtype=torch.float32)
    a, b, c = Obj(), Obj(), Obj()
    a.x, a.more = base[:8], [None, (torch.ones(3),), {"k": _Holder(torch.ones(2))}]
    b.y = base[32:40]                                       # another view of a.x's storage: no common element, shared all the same
    c.z, c.empty = torch.zeros(8), torch.empty(0)
    assert sorted(S.tensors_of(a)) == ["more[1][0]", "more[2]['k'].buf", "x"]
    assert len(S.storage_of(a)) == 3 and len(S.storage_of(c)) == 1
    assert S.disjoint(a, c) and S.disjoint([a, b], c)
    with pytest.raises(AssertionError, match="shared storage"):
        S.disjoint(a, b)
    snap = S.snapshot(c)
    assert S.unchanged(c, snap)
    c.z[3] = -0.0                                           # equal as a number, another bit pattern
    with pytest.raises(AssertionError, match="z changed"):
        S.unchanged(c, snap)
    assert S.same(np.float32([np.nan]), np.float32([np.nan])) and not S.same(np.float32([0.0]), np.float64([0.0]))

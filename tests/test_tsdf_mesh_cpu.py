"""CPU suite of the mesh extraction (AC12): the marching-cubes case table judged by the properties a correct
table has (nothing here trusts the typed numbers), the serial restatement tests/tsdf_mesh_ref.py end to end on a sphere, the
header's copy of the table, the PLY reader / writer, the stated errors and the ABI's host-side answers."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import tsdf_mesh_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = range(256)


def corner_pos(c):
    return np.array(M.CORNERS[c], dtype=np.float64)


def midpoint(e):
    a, b = M.EDGE_CORNERS[e]
    return (corner_pos(a) + corner_pos(b)) / 2.0


def edge_faces(e):
    """the two faces (axis, side) of the cube that contain edge e"""
    a, b = M.EDGE_CORNERS[e]
    return {(k, M.CORNERS[a][k]) for k in range(3) if M.CORNERS[a][k] == M.CORNERS[b][k]}


def table_triangles(code):
    r = M.row(code)
    return [tuple(r[i:i + 3]) for i in range(0, len(r), 3)]


def directed_sides(code):
    """every directed side (edge index -> edge index) of the triangles of a row, in the table's own orientation"""
    return [(t[i], t[(i + 1) % 3]) for t in table_triangles(code) for i in range(3)]


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_edges_and_corners_are_consistent():
    """the first corner of an edge is the edge's lower voxel and the second lies one step along the edge's axis"""
    for e, (dx, dy, dz, a) in enumerate(M.EDGE_SHIFTS):
        c0, c1 = M.EDGE_CORNERS[e]
        assert M.CORNERS[c0] == (dx, dy, dz)
        step = [0, 0, 0]
        step[a] = 1
        assert M.CORNERS[c1] == (dx + step[0], dy + step[1], dz + step[2])


def test_spot_rows():
    assert M.row(0) == [] and M.row(255) == []
    assert M.row(1) == [0, 8, 3] and M.row(2) == [0, 1, 9] and M.row(3) == [1, 8, 3, 9, 8, 1] and M.row(254) == [0, 3, 8]


@pytest.mark.parametrize("code", CODES)
def test_a_row_uses_exactly_the_sign_changing_edges(code):
    assert sum(1 << e for e in set(M.row(code))) == M.edge_mask(code)


@pytest.mark.parametrize("code", CODES)
def test_b_row_shape(code):
    full = M.TRI_TABLE[code].tolist()
    r = M.row(code)
    assert len(full) == 16 and full[15] == -1
    assert len(r) % 3 == 0 and len(r) // 3 <= 5
    assert all(v == -1 for v in full[len(r):])
    assert all(0 <= v <= 11 for v in r)
    assert all(len(set(t)) == 3 for t in table_triangles(code))


@pytest.mark.parametrize("code", CODES)
def test_c_interior_sides_pair_up_and_face_sides_are_boundary(code):
    sides = directed_sides(code)
    for a, b in set((min(s), max(s)) for s in sides):
        fwd, back = sides.count((a, b)), sides.count((b, a))
        if edge_faces(a) & edge_faces(b):
            assert fwd + back == 1, (code, a, b)                 # lies in a face of the cube: the surface's boundary there
        else:
            assert fwd == 1 and back == 1, (code, a, b)          # interior: two triangles, opposite directions


def face_function():
    """(axis, side) -> {sign pattern of the face's four corners -> set of directed segments in the face}, both in coordinates of the
    face's plane (the axis dropped); asserts that the segments depend on the pattern alone"""
    drop = lambda p, k: tuple(int(2 * v) for i, v in enumerate(p) if i != k)          # doubled: midpoints stay integers
    out = {}
    for k, s in itertools.product(range(3), (0, 1)):
        fn = {}
        on_face = [c for c in range(8) if M.CORNERS[c][k] == s]
        for code in CODES:
            pattern = frozenset(drop(M.CORNERS[c], k) for c in on_face if (code >> c) & 1)
            segs = frozenset((drop(midpoint(a), k), drop(midpoint(b), k)) for a, b in directed_sides(code)
                             if (k, s) in edge_faces(a) & edge_faces(b))
            assert fn.setdefault(pattern, segs) == segs, (k, s, code)
        assert len(fn) == 16
        out[(k, s)] = fn
    return out


def test_d_no_cracks():
    """what a cube leaves on a face is a function of the face's corner signs, and the neighbouring cube, which sees the same face
    from the other side, leaves the same segments reversed: every segment on a shared face belongs to two triangles that traverse it
    in opposite directions"""
    fn = face_function()
    for k in range(3):
        for pattern, segs in fn[(k, 1)].items():
            assert fn[(k, 0)][pattern] == frozenset((b, a) for a, b in segs), (k, sorted(pattern))


@pytest.mark.parametrize("corner", range(8))
def test_e_single_corner_normal_points_away_from_the_negative_corner(corner):
    (t0, t1, t2), = table_triangles(1 << corner)
    v = np.stack([midpoint(t0), midpoint(t2), midpoint(t1)]).astype(np.float32)                 # the emitted order
    n = M.triangle_normals(v, np.array([[0, 1, 2]]), normalized=False)[0].astype(np.float64)
    assert np.dot(n, v.mean(0) - corner_pos(corner)) > 0.0


def test_header_table_equals_the_reference_copy():
    text = open(os.path.join(ROOT, "kinectpy_amd", "csrc", "kpx_mctables.h")).read()
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)
    body = text[text.index("{", text.index("kMcTriTable")):]
    nums = [int(v) for v in re.findall(r"-?\d+", body)]
    assert len(nums) == 256 * 16
    assert np.array_equal(np.array(nums, dtype=np.int8).reshape(256, 16), M.TRI_TABLE)


# ---- the restatement end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    f, w = M.sphere_volume()
    return M.extract_triangle_mesh(f, w, None, 16, 0.25, (-1.0, 2.0, 0.5))


def test_sphere_is_closed_oriented_and_of_genus_zero(sphere):
    v, _, t, keys = sphere
    assert len(v) and len(t) and t.min() == 0 and t.max() == len(v) - 1
    assert np.all((keys[1:, 0] > keys[:-1, 0]) | ((keys[1:, 0] == keys[:-1, 0]) & (keys[1:, 1] > keys[:-1, 1])))
    directed = [(int(tr[i]), int(tr[(i + 1) % 3])) for tr in t for i in range(3)]
    assert len(set(directed)) == len(directed)
    assert all((b, a) in set(directed) for a, b in directed)                      # every edge twice, in opposite directions
    E = len(directed) // 2
    assert len(v) - E + len(t) == 2
    p = v.astype(np.float64)
    vol = np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6.0
    assert vol > 0.0
    assert abs(vol - 4.0 / 3.0 * np.pi * (5.3 * 0.25) ** 3) < 0.05 * vol


def test_sphere_normals_and_area(sphere):
    v, _, t, _ = sphere
    centre = np.array([7.3, 8.1, 6.6]) * 0.25 + np.array([-1.0, 2.0, 0.5])
    tn = M.triangle_normals(v, t).astype(np.float64)
    assert np.all(np.einsum("ij,ij->i", tn, v[t].astype(np.float64).mean(1) - centre) > 0.0)          # outward
    vn = M.vertex_normals(v, t).astype(np.float64)
    assert np.all(np.einsum("ij,ij->i", vn, v.astype(np.float64) - centre) > 0.0)
    slow = np.zeros((len(v), 3))
    raw = M.triangle_normals(v, t, normalized=False)
    n64 = M._cross(v, t)
    assert np.array_equal(raw, n64.astype(np.float32))
    for i, tr in enumerate(t):                                                     # the literal loop the rounds restate
        for c in tr:
            slow[c] = slow[c] + n64[i]
    assert np.array_equal(M.vertex_normals(v, t, normalized=False), slow.astype(np.float32))
    area = M.surface_area(v, t)
    assert abs(area - 4.0 * np.pi * (5.3 * 0.25) ** 2) < 0.05 * area


def test_zero_normal_becomes_unit_z():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 5, 5]], dtype=np.float32)
    t = np.array([[0, 1, 2]], dtype=np.int32)
    assert np.array_equal(M.triangle_normals(v, t), [[0, 0, 1]])
    assert np.array_equal(M.vertex_normals(v, t), [[0, 0, 1]] * 4)
    assert np.array_equal(M.vertex_normals(v, t, normalized=False), np.zeros((4, 3)))


def test_inactive_cubes_and_signed_zero():
    """a corner of weight 0 silences its cubes; -0.0 and NaN are not negative"""
    f = np.full(8, 0.5, dtype=np.float32)
    f[0] = -0.5
    w = np.ones(8, dtype=np.float32)
    v, c, t, keys = M.extract_triangle_mesh(f, w, None, 2, 1.0, (0, 0, 0))
    assert len(v) == 3 and len(t) == 1 and keys.tolist() == [[0, 0], [0, 1], [0, 2]]
    assert np.array_equal(v, [[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0]])
    w[7] = 0.0
    assert len(M.extract_triangle_mesh(f, w, None, 2, 1.0, (0, 0, 0))[0]) == 0
    for zero in (-0.0, np.nan):
        f[0] = zero
        assert len(M.extract_triangle_mesh(f, np.ones(8, np.float32), None, 2, 1.0, (0, 0, 0))[0]) == 0
    assert all(len(a) == 0 for a in M.extract_triangle_mesh(np.zeros(1, np.float32), np.ones(1, np.float32), None, 1, 1.0, (0, 0, 0))[::2])


# ---- PLY --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ascii_", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip(ascii_, with_normals, with_colors):
    from kinectpy_amd import mesh_io
    rng = np.random.default_rng(5)
    v = rng.standard_normal((37, 3)).astype(np.float32).astype(np.float64) * 1e3
    v[0] = (0.1, -1e-300, 1.7976931348623157e308)
    n = rng.standard_normal((37, 3)) if with_normals else None
    c = rng.random((37, 3)) if with_colors else None
    t = rng.integers(0, 37, (50, 3)).astype(np.int32)
    raw = mesh_io.encode_ply(v, t, n, c, write_ascii=ascii_)
    assert raw.startswith(b"ply\nformat " + (b"ascii" if ascii_ else b"binary_little_endian") + b" 1.0\n")
    head = raw[:raw.index(b"end_header\n")].decode()
    assert "property double x" in head and "property list uchar uint vertex_indices" in head
    assert ("property double nx" in head) == with_normals and ("property uchar red" in head) == with_colors
    v2, t2, n2, c2 = mesh_io.decode_ply(raw)
    assert v2.dtype == np.float64 and np.array_equal(v2.view(np.uint64), v.view(np.uint64))
    assert t2.dtype == np.int32 and np.array_equal(t2, t)
    if with_normals:
        assert np.array_equal(n2.view(np.uint64), n.view(np.uint64))
    else:
        assert n2 is None
    if with_colors:
        assert np.array_equal(c2, np.clip(np.round(c * 255.0), 0, 255).astype(np.uint8) / 255.0)
    else:
        assert c2 is None


def test_ply_empty_mesh_and_other_formats(tmp_path):
    from kinectpy_amd import mesh_io
    v, t, n, c = mesh_io.decode_ply(mesh_io.encode_ply(np.zeros((0, 3)), np.zeros((0, 3), np.int32)))
    assert v.shape == (0, 3) and t.shape == (0, 3) and n is None and c is None
    for name in ("mesh.obj", "mesh.stl"):
        with pytest.raises(NotImplementedError, match="PLY"):
            mesh_io.write_triangle_mesh(str(tmp_path / name), None)
        with pytest.raises(NotImplementedError, match="PLY"):
            mesh_io.read_triangle_mesh(str(tmp_path / name))
    with pytest.raises(RuntimeError, match="range"):
        mesh_io.encode_ply(np.zeros((2, 3)), np.array([[0, 1, 2]], np.int32))


# ---- stated errors and the ABI ------------------------------------------------------------------------------------------------------
def test_extract_triangle_mesh_without_a_device_volume():
    from kinectpy_amd import o3d
    ns = o3d.pipelines.integration
    for who in (None, object()):
        with pytest.raises(NotImplementedError, match=r"UniformTSDFVolume\.extract_triangle_mesh: .*no CPU fallback"):
            ns.UniformTSDFVolume.extract_triangle_mesh(who)


def test_namespace_exports():
    from kinectpy_amd import geometry, mesh_io, o3d
    assert o3d.geometry.TriangleMesh is geometry.TriangleMesh and o3d.utility.Vector3iVector is geometry.Vector3iVector
    assert o3d.io.write_triangle_mesh is mesh_io.write_triangle_mesh and o3d.io.read_triangle_mesh is mesh_io.read_triangle_mesh
    a = np.asarray(o3d.utility.Vector3iVector([[0, 1, 2], [2, 1, 0]]))
    assert a.dtype == np.int32 and a.shape == (2, 3)
    with pytest.raises(RuntimeError):
        o3d.utility.Vector3iVector([[0, 1]])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from kinectpy_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.load()


def test_abi_symbols_and_host_side_answers(lib):
    for name in ("kpx_tsdf_mesh_workspace_bytes", "kpx_tsdf_mesh_count", "kpx_tsdf_mesh_fill", "kpx_mesh_normals_workspace_bytes",
                 "kpx_mesh_normals", "kpx_mesh_surface_area"):
        assert hasattr(lib, name), name
    assert lib.kpx_tsdf_mesh_workspace_bytes(0) == 0 and lib.kpx_tsdf_mesh_workspace_bytes(1025) == 0
    assert lib.kpx_tsdf_mesh_workspace_bytes(-3) == 0
    one, big = lib.kpx_tsdf_mesh_workspace_bytes(1), lib.kpx_tsdf_mesh_workspace_bytes(512)
    assert 0 < one < big
    assert big < 512 ** 3 * 2                                    # a code byte and half a byte of group records per voxel, not an index array
    assert lib.kpx_mesh_normals_workspace_bytes(-1, 5) == 0 and lib.kpx_mesh_normals_workspace_bytes(5, -1) == 0
    assert lib.kpx_mesh_normals_workspace_bytes(0, 0) > 0
    assert lib.kpx_mesh_normals_workspace_bytes(1000, 2000) > 2000 * 3 * 8
    assert lib.kpx_tsdf_mesh_count(None, 0, None, None, 0, None) == -1 and b"resolution" in lib.kpx_last_error()
    assert lib.kpx_tsdf_mesh_count(None, 8, None, None, 0, None) == -1 and b"null pointer" in lib.kpx_last_error()
    org = np.zeros(3)
    rc = lib.kpx_tsdf_mesh_fill(None, None, 8, C.c_double(0.0), org.ctypes.data_as(C.c_void_p), 1, 1, None, None, None, None, 0, None)
    assert rc == -1 and b"voxel_length" in lib.kpx_last_error()
    rc = lib.kpx_tsdf_mesh_fill(None, None, 8, C.c_double(1.0), org.ctypes.data_as(C.c_void_p), 1 << 31, 1, None, None, None, None, 0, None)
    assert rc == -3 and b"2^31" in lib.kpx_last_error()
    assert lib.kpx_mesh_normals(None, -1, None, 0, 1, None, None, None, 0, None) == -1
    assert lib.kpx_mesh_normals(None, 1 << 31, None, 0, 1, None, None, None, 0, None) == -3
    assert lib.kpx_mesh_normals(None, 0, None, 0, 1, None, None, None, 0, None) == 0             # nothing to do, nothing launched

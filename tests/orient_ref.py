"""Serial restatement of arithmetic contract AC17: normal orientation and the Euclidean minimum spanning tree.
fp64 on the float32 values; d2 = fma(dz, dz, fma(dy, dy, dx dx)) through tsdf_ref.fma (an exact fma), every other product and sum
rounded separately (NumPy never contracts); Kruskal under the stated total orders; Open3D's breadth-first walk with a queue."""
from collections import deque

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import minimum_spanning_tree
from scipy.spatial import Delaunay

from tests import tsdf_ref


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3))


def dot(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---- elementwise -------------------------------------------------------------------------------------------------------------------------
def normalize(normals):
    n = _f32(normals).copy()
    d = n.astype(np.float64)
    ln = np.sqrt(dot(d, d))
    ok = ln > 0
    n[ok] = (d[ok] / ln[ok, None]).astype(np.float32)
    return n


def _flip_where(n, towards, zero_value):
    d = n.astype(np.float64)
    zero = np.sqrt(dot(d, d)) == 0
    neg = ~zero & (dot(d, towards) < 0)
    out = n.copy()
    out[neg] = -n[neg]
    out[zero] = np.broadcast_to(zero_value, d.shape)[zero].astype(np.float32)
    return out


def align_with_direction(normals, ref=(0.0, 0.0, 1.0)):
    n = _f32(normals)
    ref = np.asarray(ref, np.float64).reshape(3)
    return _flip_where(n, np.broadcast_to(ref, (len(n), 3)), ref)


def towards_camera(points, normals, cam=(0.0, 0.0, 0.0)):
    """the zero-normal branch, r / |r|, is one more rounding of an fp64 value: compared within one float32 ulp"""
    p, n = _f32(points).astype(np.float64), _f32(normals)
    r = np.asarray(cam, np.float64).reshape(1, 3) - p
    rl = np.sqrt(dot(r, r))
    unit = np.where(rl[:, None] == 0, np.array([0.0, 0.0, 1.0]), r / np.where(rl == 0, 1.0, rl)[:, None])
    return _flip_where(n, r, unit)


# ---- trees ---------------------------------------------------------------------------------------------------------------------------------
def d2_pairs(points, a, b):
    """AC3 between points a[i] and b[i]"""
    p = _f32(points).astype(np.float64)
    d = p[np.asarray(a)] - p[np.asarray(b)]
    return tsdf_ref.fma(d[:, 2], d[:, 2], tsdf_ref.fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))


def kruskal(n, a, b, w):
    """minimum spanning forest of the edges {a[i] < b[i]} under the total order (w, a, b) -> int32 (m, 2) rows ascending in (a, b)"""
    a, b, w = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(w, np.float64)
    assert np.all(a < b) and not np.any(np.isnan(w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    for i in np.lexsort((b, a, w)):
        ra, rb = find(int(a[i])), find(int(b[i]))
        if ra != rb:
            parent[ra] = rb
            out.append((int(a[i]), int(b[i])))
            if len(out) == n - 1:
                break
    return np.asarray(sorted(out), dtype=np.int32).reshape(-1, 2)


def emst(points):
    """Kruskal on the complete graph under (d2, a, b)"""
    n = len(_f32(points))
    a, b = np.triu_indices(n, 1)
    return kruskal(n, a, b, d2_pairs(points, a, b))


def knn_rows(points, k):
    """(n, min(k, n)) indices of all points, the query included, ascending in (d2, index)"""
    p = _f32(points)
    n = len(p)
    i, j = np.divmod(np.arange(n * n), n)
    D = d2_pairs(p, i, j).reshape(n, n)
    return np.stack([np.lexsort((np.arange(n), D[v]))[:min(k, n)] for v in range(n)]).astype(np.int32).reshape(n, min(k, n))


def graph_edges(n, emst_edges, rows):
    """the Riemannian graph: the EMST plus {v, u}, u != v in v's row -> distinct (a < b) rows"""
    rows = np.asarray(rows, np.int64).reshape(n, -1)
    v = np.repeat(np.arange(n), rows.shape[1])
    u = rows.reshape(-1)
    keep = (u >= 0) & (u != v)
    pairs = np.concatenate([np.asarray(emst_edges, np.int64).reshape(-1, 2), np.stack([np.minimum(v, u)[keep], np.maximum(v, u)[keep]], -1)])
    return np.unique(pairs, axis=0)


def orientation_tree(normals, edges):
    nrm = _f32(normals).astype(np.float64)
    a, b = edges[:, 0], edges[:, 1]
    return kruskal(len(nrm), a, b, 1.0 - np.abs(dot(nrm[a], nrm[b])))


def root_of(points):
    return int(np.argmax(_f32(points)[:, 2]))              # the first of the maxima: the lowest index (-0.0 == 0.0)


def walk(points, normals, tree):
    """Open3D's breadth-first propagation over the tree from the root -> flips uint8 (n)"""
    p, nrm = _f32(points), _f32(normals).astype(np.float64)
    n = len(p)
    adj = [[] for _ in range(n)]
    for a, b in np.asarray(tree).reshape(-1, 2):
        adj[a].append(int(b))
        adj[b].append(int(a))
    r = root_of(p)
    sign = np.zeros(n, np.int64)
    sign[r] = -1 if nrm[r, 2] < 0 else 1
    queue = deque([r])
    while queue:
        a = queue.popleft()
        for b in adj[a]:
            if sign[b] == 0:
                c = dot(nrm[a], nrm[b])
                sign[b] = 1 if c == 0 else sign[a] * (1 if c > 0 else -1)
                queue.append(b)
    assert np.all(sign != 0), "the tree does not span the cloud"
    return (sign < 0).astype(np.uint8)


def apply_flips(normals, flips):
    n = _f32(normals).copy()
    f = np.asarray(flips).astype(bool)
    n[f] = -n[f]
    return n


def tangent_from_graph(points, normals, emst_edges, rows):
    """steps 3 to 5 on a given EMST and given kNN rows -> (oriented normals, flips, tree)"""
    n = len(_f32(points))
    tree = orientation_tree(normals, graph_edges(n, emst_edges, rows)) if n > 1 else np.zeros((0, 2), np.int32)
    flips = walk(points, normals, tree)
    return apply_flips(normals, flips), flips, tree


def tangent(points, normals, k):
    """orient_normals_consistent_tangent_plane(k) -> (oriented normals, flips, EMST, tree)"""
    n = len(_f32(points))
    e = emst(points) if n > 1 else np.zeros((0, 2), np.int32)
    rows = knn_rows(points, k) if k > 0 else np.zeros((n, 0), np.int32)
    out, flips, tree = tangent_from_graph(points, normals, e, rows)
    return out, flips, e, tree


# ---- SciPy, the judge of the trees --------------------------------------------------------------------------------------------------------
def scipy_mst(n, a, b, w):
    """SciPy's minimum spanning tree of the given edges -> set of (a < b); unique when the weights are pairwise distinct and positive"""
    assert len(np.unique(w)) == len(w) and np.all(w > 0)
    t = minimum_spanning_tree(coo_matrix((w, (a, b)), shape=(n, n)).tocsr()).tocoo()
    return {(int(min(i, j)), int(max(i, j))) for i, j in zip(t.row, t.col)}


def delaunay_edges(p):
    s = Delaunay(np.asarray(p, np.float64)).simplices
    e = np.concatenate([s[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    return np.unique(np.sort(e, axis=1), axis=0)


# ---- scenes shared by the CPU and GPU suites ----------------------------------------------------------------------------------------------
def noisy_sphere(n, seed, noise=0.15):
    """points on the unit sphere, their outward normals perturbed, half of them flipped"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    nrm = p + noise * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[rng.random(n) < 0.5] *= -1
    return p.astype(np.float32), nrm.astype(np.float32)


def cube(top_sign=-1.0, inward_face=None):
    """the interiors of the six faces of the axis-aligned cube [-1, 1]^3 on the 1/4 grid: 6 x 49 points with their faces' outward
    normals, but the top face times top_sign and the face `inward_face` (axis, side) inward.  Between two faces every dot product
    is exactly 0."""
    g = np.arange(-3, 4) / 4.0
    u, v = [x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij")]
    pts, nrm = [], []
    for axis in range(3):
        for side in (-1.0, 1.0):
            q = np.zeros((len(u), 3))
            q[:, axis] = side
            q[:, (axis + 1) % 3], q[:, (axis + 2) % 3] = u, v
            m = np.zeros((len(u), 3))
            m[:, axis] = side * (top_sign if (axis, side) == (2, 1.0) else 1.0) * (-1.0 if (axis, side) == inward_face else 1.0)
            pts.append(q)
            nrm.append(m)
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32)

"""The pinned statement of arithmetic contract AC13: TriangleMesh's adjacency, non-manifold edges,
connected triangles, ordered removal, smoothing and uniform sampling, restated serially in NumPy.  float64 throughout, every multiply
and add a separate NumPy or Python operation (neither fuses them), float32 only where the contract rounds.  Sums whose order the
contract fixes are taken in that order: per vertex over its ascending neighbours (round r adds every vertex's r-th neighbour, so each
vertex sees a serial sum), per cluster and per mesh over ascending triangles (Python loops).  Philox is tests/fgr_ref.py's."""
import itertools
import math

import numpy as np

import fgr_ref
import tsdf_mesh_ref as M

SAMPLE_TAG = 0x4D534D50           # 'MSMP': word 2 of the sampler's Philox counter
EPS_DIST = 1e-12                  # added to every edge length before the Laplacian weight's division


def _tri(triangles):
    return np.asarray(triangles, dtype=np.int64).reshape(-1, 3)


# ---- adjacency and edges ----------------------------------------------------------------------------------------------------------------
def adjacency(triangles, n_vertices):
    """-> (offsets int32 (V + 1,), neighbours int32): CSR rows N(v) = the ascending distinct u over the six ordered corner pairs (v, u)
    of every triangle"""
    t = _tri(triangles)
    v = t[:, (0, 1, 1, 2, 2, 0)].reshape(-1)
    u = t[:, (1, 0, 2, 1, 0, 2)].reshape(-1)
    keys = np.unique((v << 32) | u)
    offsets = np.searchsorted(keys >> 32, np.arange(n_vertices + 1), side="left")
    return offsets.astype(np.int32), (keys & 0xFFFFFFFF).astype(np.int32)


def edge_keys(triangles):
    """(T, 3) int64: min << 32 | max of the edges {t0,t1}, {t1,t2}, {t2,t0}"""
    t = _tri(triangles)
    a, b = t, t[:, (1, 2, 0)]
    return (np.minimum(a, b) << 32) | np.maximum(a, b)


def non_manifold_edges(triangles, allow_boundary_edges=True):
    """-> int32 (E, 2) ascending (min, max): the keys that occur more than twice, or (allow_boundary_edges False) not exactly twice"""
    keys, count = np.unique(edge_keys(triangles).reshape(-1), return_counts=True)
    bad = keys[count > 2] if allow_boundary_edges else keys[count != 2]
    return np.stack([bad >> 32, bad & 0xFFFFFFFF], 1).astype(np.int32).reshape(-1, 2)


# ---- connected triangles ------------------------------------------------------------------------------------------------------------------
def triangle_areas(vertices, triangles):
    """(T,) float64: half the norm of AC12's cross product"""
    return M._norm(M._cross(vertices, triangles)) * 0.5


def cluster_connected_triangles(vertices, triangles):
    """Open3D's breadth-first search from ascending seeds over "shares an edge key" -> (triangle_clusters int32 (T,),
    cluster_n_triangles int32 (C,), cluster_area float64 (C,)); the areas are added in ascending triangle index (Open3D: BFS order)"""
    keys = edge_keys(triangles)
    T = len(keys)
    flat = keys.reshape(-1)
    order = np.argsort(flat, kind="stable")
    run_of = np.empty(3 * T, dtype=np.int64)                   # the run of equal keys every (triangle, edge) entry belongs to
    starts = np.flatnonzero(np.concatenate([[True], flat[order][1:] != flat[order][:-1]])) if T else np.zeros(0, np.int64)
    run_of[order] = np.cumsum(np.concatenate([[True], flat[order][1:] != flat[order][:-1]])) - 1 if T else 0
    ends = np.append(starts[1:], 3 * T)
    members = [(order[s:e] // 3).tolist() for s, e in zip(starts.tolist(), ends.tolist())]
    runs = run_of.reshape(T, 3).tolist()
    label = [-1] * T
    done = [False] * len(members)
    n_clusters = 0
    for seed in range(T):
        if label[seed] >= 0:
            continue
        label[seed] = n_clusters
        queue = [seed]
        while queue:
            t = queue.pop()
            for r in runs[t]:
                if done[r]:
                    continue
                done[r] = True
                for m in members[r]:
                    if label[m] < 0:
                        label[m] = n_clusters
                        queue.append(m)
        n_clusters += 1
    label = np.asarray(label, dtype=np.int32).reshape(-1)
    count = np.bincount(label, minlength=n_clusters).astype(np.int32)
    area = [0.0] * n_clusters
    for c, a in zip(label.tolist(), triangle_areas(vertices, triangles).tolist()):
        area[c] = area[c] + a
    return label, count, np.asarray(area, dtype=np.float64)


# ---- removal --------------------------------------------------------------------------------------------------------------------------------
def remove_triangles(triangles, remove, triangle_normals=None):
    keep = ~np.asarray(remove, dtype=bool)
    return np.asarray(triangles)[keep], None if triangle_normals is None else np.asarray(triangle_normals)[keep]


def remove_vertices(vertices, triangles, remove, colors=None, normals=None, triangle_normals=None):
    """the kept vertices in order, renumbered by rank, with their colours and normals; the triangles whose three corners stay, in order,
    with their normals -> (vertices, colours, normals, triangles, triangle normals)"""
    keep = ~np.asarray(remove, dtype=bool)
    t = _tri(triangles)
    new = np.cumsum(keep) - 1
    tkeep = keep[t].all(1) if len(t) else np.zeros(0, dtype=bool)
    g = lambda a, k: None if a is None else np.asarray(a)[k]
    return np.asarray(vertices)[keep], g(colors, keep), g(normals, keep), new[t[tkeep]].astype(np.int32).reshape(-1, 3), g(triangle_normals, tkeep)


def referenced(triangles, n_vertices):
    f = np.zeros(n_vertices, dtype=bool)
    f[_tri(triangles).reshape(-1)] = True
    return f


def degenerate(triangles):
    t = _tri(triangles)
    return (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])


def index_mask(indices, n):
    i = np.asarray(indices, dtype=np.int64).reshape(-1)
    f = np.zeros(n, dtype=bool)
    f[i[(i >= 0) & (i < n)]] = True
    return f


# ---- smoothing --------------------------------------------------------------------------------------------------------------------------------
def _rounds(offsets):
    """for r = 0, 1, ...: (the vertices with more than r neighbours, the position of their r-th neighbour)"""
    off = np.asarray(offsets, dtype=np.int64)
    deg = np.diff(off)
    for r in range(int(deg.max()) if len(deg) else 0):
        who = np.flatnonzero(deg > r)
        yield who, off[who] + r


def _step(x, arrays, offsets, neighbours, lam):
    """one step on the float64 arrays; x: the vertices the weights come from (None: the simple filter)"""
    deg = np.diff(np.asarray(offsets, dtype=np.int64))
    nb = np.asarray(neighbours, dtype=np.int64)
    W = np.zeros(len(deg))
    s = [np.zeros_like(y) for y in arrays]
    with np.errstate(all="ignore"):
        for who, pos in _rounds(offsets):
            u = nb[pos]
            if x is not None:
                d = x[who] - x[u]
                dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                w = 1.0 / (dist + EPS_DIST)
                W[who] = W[who] + w
            for k, y in enumerate(arrays):
                s[k][who] = s[k][who] + (w[:, None] * y[u] if x is not None else y[u])
        out = []
        for k, y in enumerate(arrays):
            if x is None:
                out.append((y + s[k]) / (1 + deg).astype(np.float64)[:, None])
            else:
                safe = np.where(deg > 0, W, 1.0)
                out.append(np.where((deg > 0)[:, None], y + lam * (s[k] / safe[:, None] - y), y))
    return out


def smooth(vertices, triangles, method, iterations, lambda_filter=0.5, mu=-0.53, normals=None, colors=None, scope=(True, True, True)):
    """-> (vertices, normals | None, colours | None) float32; the arrays outside the scope (vertices, normals, colours) come back
    unchanged.  method: "simple" | "laplacian" | "taubin"."""
    if iterations < 0:
        raise ValueError("number_of_iterations must be non-negative")
    src = [vertices, normals, colors]
    f64 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    offsets, neighbours = adjacency(triangles, len(f64(vertices)))
    on = [a is not None and bool(o) for a, o in zip(src, scope)]
    work = [f64(a) for a, o in zip(src, on) if o]
    x0 = f64(vertices)
    lams = {"simple": [None], "laplacian": [lambda_filter], "taubin": [lambda_filter, mu]}[method]
    for _ in range(iterations):
        for lam in lams:
            x = None if method == "simple" else (work[0] if on[0] else x0)
            work = _step(x, work, offsets, neighbours, lam)
    done = iter(work)
    return tuple(M._f32(next(done)) if o else (None if a is None else np.asarray(a, dtype=np.float32)) for a, o in zip(src, on))


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------------
def llround(x):
    """C's llround for x >= 0: halves away from zero (x - floor(x) is exact)"""
    f = math.floor(x)
    return f + (1 if x - f >= 0.5 else 0)


def sample_counts(vertices, triangles, n_points):
    """-> (upto int64 (T,): the points [upto[t - 1], upto[t]) fall into triangle t; total area)"""
    prefix = list(itertools.accumulate(triangle_areas(vertices, triangles).tolist()))
    total = prefix[-1]
    if not total > 0.0:
        raise ValueError("the mesh has no surface area")
    upto = [llround((p / total) * float(n_points)) for p in prefix]
    upto[-1] = n_points
    return np.asarray(upto, dtype=np.int64), total


def sample_points_uniformly(vertices, triangles, n_points, seed=0, colors=None, vertex_normals=None, triangle_normals=None):
    """-> (points, colours | None, normals | None, the triangle of every point)"""
    if n_points <= 0 or len(_tri(triangles)) == 0:
        raise ValueError("number_of_points must be positive and the mesh needs triangles")
    upto, _ = sample_counts(vertices, triangles, n_points)
    p = np.arange(n_points, dtype=np.uint64)
    t = np.searchsorted(upto, np.arange(n_points), side="right")
    w = fgr_ref.philox4x32_10(p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), SAMPLE_TAG, 0, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    unit = lambda lo, hi: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r1, r2 = unit(w[0], w[1]), unit(w[2], w[3])
    q = np.sqrt(r1)
    a, b, c = (1.0 - q)[:, None], (q * (1.0 - r2))[:, None], (q * r2)[:, None]
    corners = _tri(triangles)[t]

    def mix(rows):
        r = np.asarray(rows, dtype=np.float32).astype(np.float64).reshape(-1, 3)
        with np.errstate(all="ignore"):
            return M._f32((a * r[corners[:, 0]] + b * r[corners[:, 1]]) + c * r[corners[:, 2]])

    normals = None
    if vertex_normals is not None:
        normals = mix(vertex_normals)
    elif triangle_normals is not None:
        normals = np.asarray(triangle_normals, dtype=np.float32).reshape(-1, 3)[t]
    return mix(vertices), None if colors is None else mix(colors), normals, t

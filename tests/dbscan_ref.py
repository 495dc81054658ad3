"""Host references for cluster_dbscan / remove_radius_outlier.

dbscan_loop restates Open3D's PointCloud::ClusterDBSCAN literally: visit the points in index order, grow one cluster at a time
breadth-first.  dbscan_closed_form is the order-free form the kernels compute ("Clustering").  Both take the
neighbour lists as CSR arrays (indptr, indices); every point's list contains the point itself.
"""
import numpy as np


def csr_from_pairs(n, i, j):
    """symmetric CSR from the pairs (i, j), i != j, each given once, plus the self matches"""
    i = np.asarray(i, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    self_ = np.arange(n, dtype=np.int64)
    rows = np.concatenate([i, j, self_])
    cols = np.concatenate([j, i, self_])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    return np.cumsum(indptr), cols


def integer_neighbours(pts, eps):
    """exact radius lists (d2 < eps * eps) of a cloud whose coordinates are integers: every d2 is an exact integer in fp64"""
    from scipy.spatial import cKDTree
    p = np.asarray(pts, dtype=np.float64)
    assert np.array_equal(p, np.round(p)), "integer coordinates only"
    n = len(p)
    if n == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    pairs = cKDTree(p).query_pairs(float(eps) * (1 + 1e-9) + 1e-9, output_type="ndarray")       # inclusive r: re-filtered below
    if len(pairs):
        d2 = ((p[pairs[:, 0]] - p[pairs[:, 1]]) ** 2).sum(1)
        pairs = pairs[d2 < float(eps) * float(eps)]
    return csr_from_pairs(n, pairs[:, 0], pairs[:, 1])


def oracle_neighbours(O, pts, eps, max_nn=512):
    """radius lists from the CPU oracle's hybrid search (AC3, strict <); asserts that no row reached max_nn"""
    nbr, cnt = O.hybrid_knn(pts, eps, max_nn)
    assert cnt.max(initial=0) < max_nn, "a hybrid row saturated: raise max_nn"
    n = len(cnt)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(cnt)
    mask = np.arange(max_nn)[None, :] < cnt[:, None]
    indices = nbr[mask].astype(np.int64)
    return indptr, indices


def two_blobs_and_bridge():
    """(pts, bridge index, A indices, B indices) for eps = nextafter(1, 2), min_points = 4 (4-connected integer lattice): two 3 x 3
    blocks whose centre and edge midpoints are core, a point between their facing edge midpoints with three neighbours (not core),
    eleven isolated points; 30 points in all"""
    a = [(x, y, 0) for x in range(3) for y in range(3)]
    b = [(x + 4, y, 0) for x in range(3) for y in range(3)]
    iso = [(20 + 3 * k, 20, 0) for k in range(11)]
    pts = np.array(a + b + [(3, 1, 0)] + iso, dtype=np.float64)
    return pts, 18, np.arange(9), np.arange(9, 18)


def counts(indptr):
    return np.diff(indptr)


def dbscan_loop(indptr, indices, min_points):
    """Open3D's sequential loop, literally: -2 = unvisited, -1 = noise"""
    n = len(indptr) - 1
    cnt = np.diff(indptr)
    labels = np.full(n, -2, dtype=np.int64)
    visited_by = np.full(n, -1, dtype=np.int64)          # nbs_visited of the current cluster, as a stamp
    cluster = 0
    for idx in range(n):
        if labels[idx] != -2:
            continue
        if cnt[idx] < min_points:
            labels[idx] = -1
            continue
        nbs_next = set(indices[indptr[idx]:indptr[idx + 1]].tolist())
        visited_by[idx] = cluster
        labels[idx] = cluster
        while nbs_next:
            nb = nbs_next.pop()
            visited_by[nb] = cluster
            if labels[nb] == -1:
                labels[nb] = cluster
            if labels[nb] != -2:
                continue
            labels[nb] = cluster
            if cnt[nb] >= min_points:
                for q in indices[indptr[nb]:indptr[nb + 1]].tolist():
                    if visited_by[q] != cluster:
                        nbs_next.add(q)
        cluster += 1
    return labels.astype(np.int32)


def dbscan_closed_form(indptr, indices, min_points):
    """core = count >= min_points; components of the core graph ranked by their smallest index; border = smallest core id"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(indptr) - 1
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    cnt = np.diff(indptr)
    core = cnt >= min_points
    rows = np.repeat(np.arange(n), cnt)
    keep = core[rows] & core[indices]
    g = csr_matrix((np.ones(int(keep.sum()), dtype=np.int8), (rows[keep], indices[keep])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    labels = np.full(n, -1, dtype=np.int64)
    core_idx = np.flatnonzero(core)
    if len(core_idx):
        # components in order of their smallest core index (core_idx is ascending: first occurrence)
        _, first = np.unique(comp[core_idx], return_index=True)
        seeds = core_idx[np.sort(first)]
        rank = np.full(n, -1, dtype=np.int64)
        rank[comp[seeds]] = np.arange(len(seeds))
        labels[core] = rank[comp[core]]
        border = ~core
        cid = np.where(core[indices], labels[indices], np.iinfo(np.int64).max)
        mins = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(mins, rows, cid)
        labels[border] = np.where(mins[border] == np.iinfo(np.int64).max, -1, mins[border])
    return labels.astype(np.int32)

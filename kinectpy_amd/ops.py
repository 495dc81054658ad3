"""Tensor-level operators: one thin function per C-ABI entry point of libkinectpx.so.

Inputs/outputs are torch-ROCm tensors (device memory containers).  Functions that produce a
data-dependent number of rows read the device count (one host sync) and return trimmed views.
Where a function hands back a padded buffer with its count instead, the rows at and beyond the
count are unspecified ("carved scratch": the contract tests/test_scratch_gpu.py holds
every operator to).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

GATE_MM = 750.0          # preprocessing/data.py:170-171
FLAG_COLOR_MASK = 1
FLAG_DEPTH_GATE = 2


def _dev(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.to(device=L.device(), dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(L.device()).contiguous()


def _count(t):
    """Device count word(s) -> Python ints; negative values are kpx_status codes raised by kernels."""
    v = t.cpu().tolist()
    for c in v:
        if c < 0:
            raise L.KinectPxError("voxel_size is too small" if c == -3 else f"kpx device error {c}")
    return v


def _T(T):
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4))
    return T


LOSS_KINDS = {"l2": 0, "l1": 1, "huber": 2, "cauchy": 3, "gm": 4, "tukey": 5}          # KPX_LOSS_* (include/kinectpx.h)


def _loss(loss):
    """`loss` of icp / colored_icp / generalized_icp -> (KPX_LOSS_* kind, k).  None = L2; otherwise an object with `.kind` (a name
    of LOSS_KINDS) and `.k` -- the o3d.pipelines.registration losses -- or a (name, k) pair."""
    if loss is None:
        return 0, 0.0
    name, k = loss if isinstance(loss, (tuple, list)) else (getattr(loss, "kind", None), getattr(loss, "k", 0.0))
    if name not in LOSS_KINDS:
        raise ValueError(f"unknown robust loss {loss!r}: expected None, one of the o3d.pipelines.registration losses or a (name, k) pair "
                         f"with name in {sorted(LOSS_KINDS)}")
    return LOSS_KINDS[name], float(0.0 if k is None else k)


# ---- extract --------------------------------------------------------------------------------------
def unproject_u16(depth, xy_table, frames=1):
    """a1.  depth u16 [frames*n_px], xy f32 [n_px*2] -> int16 [frames, n_px, 3]."""
    lib = L.load()
    depth = _dev(depth, torch.uint16).reshape(-1)
    xy = _dev(xy_table, torch.float32).reshape(-1)
    n_px = xy.numel() // 2
    assert depth.numel() == frames * n_px
    out = torch.empty((frames, n_px, 3), dtype=torch.int16, device=depth.device)
    L.check(lib.kpx_unproject_u16(L.ptr(depth), L.ptr(xy), n_px, frames, L.ptr(out), L.stream_ptr()))
    return out


def median_i16(v, n, stride, frames=1):
    lib = L.load()
    out = torch.empty(frames, dtype=torch.float64, device=v.device)
    ws, wsz = L.workspace(lib.kpx_median_workspace_bytes(frames))
    L.check(lib.kpx_median_i16(L.ptr(v), n, stride, frames, L.ptr(out), ws, wsz, L.stream_ptr()))
    return out


def rgbd_compact(xyz, rgb=None, frames=1, color_mask=False, depth_gate=False, gate=GATE_MM, want_idx=True, sync=True):
    """a3 (+a4).  xyz int16 [frames, n, 3]; rgb u8 [frames, n, 3] or None.
    Returns per-frame lists (points f32 (K,3), colours f32 (K,3)|None, idx i32 (K)|None) or, with sync=False, the padded buffers
    and the device count tensor (no host round trip).  The rows of a padded buffer at and beyond its frame's count are unspecified."""
    lib = L.load()
    xyz = _dev(xyz, torch.int16).reshape(frames, -1, 3)
    n = xyz.shape[1]
    rgb_t = _dev(rgb, torch.uint8).reshape(frames, n, 3) if rgb is not None else None
    dev = xyz.device
    flags = (FLAG_COLOR_MASK if (color_mask and rgb is not None) else 0) | (FLAG_DEPTH_GATE if depth_gate else 0)
    med = median_i16(xyz.reshape(-1)[2:], n, 3, frames) if depth_gate else None   # z column, frame stride 3n
    pts = torch.empty((frames, n, 3), dtype=torch.float32, device=dev)
    col = torch.empty((frames, n, 3), dtype=torch.float32, device=dev) if rgb_t is not None else None
    idx = torch.empty((frames, n), dtype=torch.int32, device=dev) if want_idx else None
    cnt = torch.empty(frames, dtype=torch.int32, device=dev)
    ws, wsz = L.workspace(lib.kpx_compact_workspace_bytes(n, frames))
    L.check(lib.kpx_rgbd_compact(L.ptr(xyz), L.ptr(rgb_t), n, frames, flags, L.ptr(med), float(gate), L.ptr(pts),
                                 L.ptr(col), L.ptr(idx), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    if not sync:
        return pts, col, idx, cnt
    ks = _count(cnt)
    return [(pts[f, :k], col[f, :k] if col is not None else None, idx[f, :k] if idx is not None else None)
            for f, k in enumerate(ks)]


def depth_to_cloud(depth, xy_table, rgb=None, frames=1, color_mask=False, depth_gate=False, gate=GATE_MM,
                   want_idx=False, sync=True):
    """Fused a1+a3+a4.  Returns per-frame (points, colours|None, idx|None) or, with sync=False,
    the padded buffers and the device count tensor.  The rows of a padded buffer at and beyond its frame's count are unspecified."""
    lib = L.load()
    depth = _dev(depth, torch.uint16).reshape(frames, -1)
    n = depth.shape[1]
    xy = _dev(xy_table, torch.float32).reshape(-1)
    rgb_t = _dev(rgb, torch.uint8).reshape(frames, n, 3) if rgb is not None else None
    dev = depth.device
    flags = (FLAG_COLOR_MASK if (color_mask and rgb is not None) else 0) | (FLAG_DEPTH_GATE if depth_gate else 0)
    pts = torch.empty((frames, n, 3), dtype=torch.float32, device=dev)
    col = torch.empty((frames, n, 3), dtype=torch.float32, device=dev) if rgb_t is not None else None
    idx = torch.empty((frames, n), dtype=torch.int32, device=dev) if want_idx else None
    cnt = torch.empty(frames, dtype=torch.int32, device=dev)
    ws, wsz = L.workspace(lib.kpx_depth_to_cloud_workspace_bytes(n, frames))
    L.check(lib.kpx_depth_to_cloud(L.ptr(depth), L.ptr(xy), L.ptr(rgb_t), n, frames, flags, float(gate), L.ptr(pts),
                                   L.ptr(col), L.ptr(idx), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    if not sync:
        return pts, col, idx, cnt
    ks = _count(cnt)
    return [(pts[f, :k], col[f, :k] if col is not None else None, idx[f, :k] if idx is not None else None)
            for f, k in enumerate(ks)]


# ---- container ops ----------------------------------------------------------------------------------
def transform(pts, T, out=None):
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    out = torch.empty_like(pts) if out is None else out
    T = _T(T)
    L.check(lib.kpx_transform(L.ptr(pts), pts.shape[0], L.hptr(T), L.ptr(out), L.stream_ptr()))
    return out


def rotate(nrm, T, out=None):
    lib = L.load()
    nrm = _dev(nrm, torch.float32).reshape(-1, 3)
    out = torch.empty_like(nrm) if out is None else out
    T = _T(T)
    L.check(lib.kpx_rotate(L.ptr(nrm), nrm.shape[0], L.hptr(T), L.ptr(out), L.stream_ptr()))
    return out


def joints_affine(x, A, t):
    """a5: x (rows,3) f64 @ A (3,3) + t"""
    lib = L.load()
    x = _dev(x, torch.float64).reshape(-1, 3)
    out = torch.empty_like(x)
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(3, 3)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    L.check(lib.kpx_joints_affine_f64(L.ptr(x), x.shape[0], L.hptr(A), L.hptr(t), L.ptr(out), L.stream_ptr()))
    return out


def bounds(pts):
    """min x, y, z, max x, y, z of an (n,3) f32 cloud as a float64[6] device tensor (Open3D get_min_bound / get_max_bound;
    floor_removal.py:65-66 takes max(y))."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    if pts.shape[0] == 0:
        raise L.KinectPxError("bounds: empty cloud")
    out = torch.empty(6, dtype=torch.float64, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_bounds_workspace_bytes())
    L.check(lib.kpx_bounds(L.ptr(pts), pts.shape[0], L.ptr(out), ws, wsz, L.stream_ptr()))
    return out


def select_by_index(attrs, idx, invert=False, trusted=False, want_bounds=False):
    """attrs: list of up to three (n,3) f32 tensors (None allowed).  Returns list of selected tensors.
    [O3D] SelectByIndex has mask semantics: the result is in ascending original order without duplicates whatever the
    order of idx.  trusted=True is for index lists that come straight from another operator of this library (the keep
    list of sor, the inliers of segment_plane: ascending, duplicate-free, in range): it skips the range check (two
    reductions and a host sync) and selects with one gather."""
    lib = L.load()
    attrs = list(attrs) + [None] * (3 - len(attrs))
    ref = next(a for a in attrs if a is not None)
    n = ref.shape[0]
    idx = _dev(idx, torch.int32).reshape(-1)
    k = idx.numel()
    if k and n and not trusted:
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= n:
            raise L.KinectPxError("select_by_index: index out of range")
    # trusted lists are ascending and duplicate-free by construction: a plain gather equals Open3D's mask selection
    mode = 1 if invert else (0 if trusted else 2)
    if want_bounds:
        # the gather that also leaves the selected cloud's bounds (attrs[0] = the points); returns (outs, bounds or None)
        if mode or k == 0 or attrs[0] is None:
            return select_by_index(attrs, idx, invert, trusted), None
        outs = [torch.empty((k, 3), dtype=torch.float32, device=ref.device) if a is not None else None for a in attrs]
        bb = torch.empty(6, dtype=torch.float64, device=ref.device)
        ws, wsz = L.workspace(lib.kpx_select_workspace_bytes(n))
        L.check(lib.kpx_select_by_index_bounds(L.ptr(attrs[0]), L.ptr(attrs[1]), L.ptr(attrs[2]), n, L.ptr(idx), k,
                                               L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(bb), ws, wsz, L.stream_ptr()))
        return outs, bb
    m = n if mode else k
    outs = [torch.empty((m, 3), dtype=torch.float32, device=ref.device) if a is not None else None for a in attrs]
    cnt = torch.empty(1, dtype=torch.int32, device=ref.device) if mode else None        # written by the compaction's scan
    ws, wsz = L.workspace(lib.kpx_select_workspace_bytes(n))
    L.check(lib.kpx_select_by_index(L.ptr(attrs[0]), L.ptr(attrs[1]), L.ptr(attrs[2]), n, L.ptr(idx), k, mode,
                                    L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(cnt), ws, wsz,
                                    L.stream_ptr()))
    if mode:
        m = _count(cnt)[0]
        outs = [o[:m] if o is not None else None for o in outs]
    return outs


def halfspace_select(pts, plane):
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=pts.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=pts.device)
    pl = np.ascontiguousarray(plane, dtype=np.float64).reshape(4)
    ws, wsz = L.workspace(lib.kpx_select_workspace_bytes(n))
    L.check(lib.kpx_halfspace_select(L.ptr(pts), n, L.hptr(pl), L.ptr(idx), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    return idx[:_count(cnt)[0]]


def slab_split(pts, slab, bounds=None):
    """bounds: the cloud's float64[6] device bounds when they are known (ops.bounds, select_by_index(want_bounds=True)):
    max(y) is read from them instead of from a pass over the points."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    lo = torch.empty(n, dtype=torch.int32, device=pts.device)
    up = torch.empty(n, dtype=torch.int32, device=pts.device)
    cnt = torch.zeros(2, dtype=torch.int32, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_select_workspace_bytes(n))
    if bounds is not None:
        if bounds.dtype != torch.float64 or bounds.numel() != 6 or bounds.device != pts.device:
            raise L.KinectPxError("slab_split: bounds must be a float64[6] tensor on the cloud's device")
        L.check(lib.kpx_slab_split_bounded(L.ptr(pts), n, float(slab), L.ptr(bounds), L.ptr(lo), C.c_void_p(cnt.data_ptr()), L.ptr(up),
                                           C.c_void_p(cnt.data_ptr() + 4), ws, wsz, L.stream_ptr()))
    else:
        L.check(lib.kpx_slab_split(L.ptr(pts), n, float(slab), L.ptr(lo), C.c_void_p(cnt.data_ptr()), L.ptr(up),
                                   C.c_void_p(cnt.data_ptr() + 4), ws, wsz, L.stream_ptr()))
    c = _count(cnt)
    return lo[:c[0]], up[:c[1]]


# ---- filters ----------------------------------------------------------------------------------------
def voxel_downsample(pts, voxel, col=None, nrm=None):
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    col = _dev(col, torch.float32).reshape(-1, 3) if col is not None else None
    nrm = _dev(nrm, torch.float32).reshape(-1, 3) if nrm is not None else None
    dev = pts.device
    op = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    oc = torch.empty_like(op) if col is not None else None
    on = torch.empty_like(op) if nrm is not None else None
    cnt = torch.empty(1, dtype=torch.int32, device=dev)                                  # written by the library (0 for an empty cloud)
    ws, wsz = L.workspace(lib.kpx_voxel_workspace_bytes(n))
    L.check(lib.kpx_voxel_downsample(L.ptr(pts), L.ptr(col), L.ptr(nrm), n, float(voxel), L.ptr(op), L.ptr(oc),
                                     L.ptr(on), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    m = _count(cnt)[0]
    return op[:m], (oc[:m] if oc is not None else None), (on[:m] if on is not None else None)


def voxel_downsample_batch(clouds, voxel, cols=None):
    """voxel_down_sample of several independent clouds in one call (processed side by side on the library's internal
    lanes, one read-back for all counts).  Returns a list of (points, colours | None)."""
    lib = L.load()
    clouds = [_dev(p, torch.float32).reshape(-1, 3) for p in clouds]
    cnt = len(clouds)
    if cnt == 0:
        return []
    dev = clouds[0].device
    cols = [_dev(c, torch.float32).reshape(-1, 3) for c in cols] if cols is not None else None
    outs = [torch.empty((max(p.shape[0], 1), 3), dtype=torch.float32, device=dev) for p in clouds]
    ocols = [torch.empty_like(o) for o in outs] if cols is not None else None
    n_arr = np.array([p.shape[0] for p in clouds], dtype=np.int64)
    arr = lambda ts: C.cast((C.c_void_p * cnt)(*[t.data_ptr() for t in ts]), C.c_void_p) if ts is not None else None
    counts = torch.empty(cnt, dtype=torch.int32, device=dev)
    ws, wsz = L.workspace(lib.kpx_voxel_batch_workspace_bytes(cnt, n_arr.ctypes.data_as(C.c_void_p)))
    L.check(lib.kpx_voxel_downsample_batch(cnt, arr(clouds), arr(cols), n_arr.ctypes.data_as(C.c_void_p), float(voxel), arr(outs),
                                           arr(ocols), L.ptr(counts), ws, wsz, L.stream_ptr()))
    ms = _count(counts)
    return [(outs[i][: ms[i]], ocols[i][: ms[i]] if ocols is not None else None) for i in range(cnt)]


def fuse_voxel_downsample(clouds, cols, Ts, voxel):
    """preprocessing/data.py:44-61 in one pass: cloud c moved by Ts[c], stacked in order, voxel_down_sample(voxel) of the
    stack on the fp64 values of the moved points (kpx_fuse_voxel_downsample).  cols: list of colour tensors or None.
    -> (points f32 (M,3), colours f32 (M,3) | None)"""
    lib = L.load()
    clouds = [_dev(p, torch.float32).reshape(-1, 3) for p in clouds]
    cnt = len(clouds)
    dev = clouds[0].device if cnt else L.device()
    cols = [_dev(c, torch.float32).reshape(-1, 3) for c in cols] if cols is not None else None
    n_arr = np.array([p.shape[0] for p in clouds], dtype=np.int64)
    total = int(n_arr.sum())
    T = np.ascontiguousarray(np.stack([_T(t) for t in Ts]))
    arr = lambda ts: C.cast((C.c_void_p * cnt)(*[t.data_ptr() for t in ts]), C.c_void_p) if ts is not None else None
    op = torch.empty((max(total, 1), 3), dtype=torch.float32, device=dev)
    oc = torch.empty_like(op) if cols is not None else None
    d_cnt = torch.empty(1, dtype=torch.int32, device=dev)
    ws, wsz = L.workspace(lib.kpx_fuse_voxel_workspace_bytes(total))
    L.check(lib.kpx_fuse_voxel_downsample(cnt, arr(clouds), arr(cols), n_arr.ctypes.data_as(C.c_void_p), L.hptr(T), float(voxel), L.ptr(op),
                                          L.ptr(oc), L.ptr(d_cnt), ws, wsz, L.stream_ptr()))
    m = _count(d_cnt)[0]
    return op[:m], (oc[:m] if oc is not None else None)


def sor(pts, nb_neighbors, std_ratio, want_avg=False):
    """a8.  Returns keep_idx i32 (K), stats f64 (3) [mean, std, thr] (device), avg f64 (N)|None."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    dev = pts.device
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev) if n else torch.zeros(3, dtype=torch.float64, device=dev)   # written by the statistics kernels
    avg = torch.empty(max(n, 1), dtype=torch.float64, device=dev) if want_avg else None
    ws, wsz = L.workspace(lib.kpx_sor_workspace_bytes(n, int(nb_neighbors)))
    L.check(lib.kpx_sor(L.ptr(pts), n, int(nb_neighbors), float(std_ratio), L.ptr(idx), L.ptr(cnt), L.ptr(stats),
                        L.ptr(avg), ws, wsz, L.stream_ptr()))
    k = _count(cnt)[0]
    return idx[:k], stats, (avg[:n] if avg is not None else None)


def knn_group_last():
    """-> (queries given to, queries handed on by) the calling thread's last group pass of the neighbour search (sor* with nb_neighbors
    <= 32, estimate_normals / estimate_covariances with max_nn <= 48); valid until that call's workspace is used again."""
    out = np.zeros(2, dtype=np.int64)
    L.check(L.load().kpx_knn_group_last(out.ctypes.data_as(C.c_void_p)))
    return int(out[0]), int(out[1])


def sor_select(pts, attr, nb_neighbors, std_ratio):
    """a8 with both results of `cl, ind = remove_statistical_outlier(...)`: -> kept points f32 (K,3), kept rows of `attr` (K,3) | None,
    keep_idx i32 (K), stats f64 (3) -- one pass, no count read-back between filter and selection (kpx_sor_select)."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    dev = pts.device
    attr = _dev(attr, torch.float32).reshape(n, 3) if attr is not None else None
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev) if n else torch.zeros(3, dtype=torch.float64, device=dev)
    op = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    oa = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev) if attr is not None else None
    ws, wsz = L.workspace(lib.kpx_sor_workspace_bytes(n, int(nb_neighbors)))
    L.check(lib.kpx_sor_select(L.ptr(pts), L.ptr(attr), n, int(nb_neighbors), float(std_ratio), L.ptr(op), L.ptr(oa), L.ptr(idx), L.ptr(cnt),
                               L.ptr(stats), ws, wsz, L.stream_ptr()))
    k = _count(cnt)[0]
    return op[:k], (oa[:k] if oa is not None else None), idx[:k], stats


def sor_partial(pts, nb_neighbors, q_begin, q_end, want_order=True):
    """Sharded a8, first half: mean kNN distances of the queries at cell-sorted positions [q_begin, q_end) of the cloud's
    grid order -> (avg f64 (q_end - q_begin) in that order, order i32 (N) sorted position -> point index | None)."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    avg = torch.empty(max(int(q_end - q_begin), 1), dtype=torch.float64, device=pts.device)
    order = torch.empty(n, dtype=torch.int32, device=pts.device) if want_order else None
    ws, wsz = L.workspace(lib.kpx_sor_workspace_bytes(n, int(nb_neighbors)))
    L.check(lib.kpx_sor_partial(L.ptr(pts), n, int(nb_neighbors), int(q_begin), int(q_end), L.ptr(avg), L.ptr(order), ws, wsz,
                                L.stream_ptr()))
    return avg[: int(q_end - q_begin)], order


def sor_finish(avg_sorted, order, std_ratio, want_avg=False):
    """Sharded a8, second half: the slabs' mean distances (all N, grid order) -> keep_idx, stats, avg | None as sor()."""
    lib = L.load()
    avg_sorted = _dev(avg_sorted, torch.float64).reshape(-1)
    order = _dev(order, torch.int32).reshape(-1)
    n = order.numel()
    assert avg_sorted.numel() == n
    dev = order.device
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    avg = torch.empty(n, dtype=torch.float64, device=dev) if want_avg else None
    ws, wsz = L.workspace(lib.kpx_sor_finish_workspace_bytes(n))
    L.check(lib.kpx_sor_finish(L.ptr(avg_sorted), L.ptr(order), n, float(std_ratio), L.ptr(idx), L.ptr(cnt), L.ptr(stats), L.ptr(avg),
                               ws, wsz, L.stream_ptr()))
    k = _count(cnt)[0]
    return idx[:k], stats, avg


def cluster_dbscan(pts, eps, min_points):
    """[O3D] ClusterDBSCAN: labels i32 (N) device tensor (-1 = noise), number of clusters i32 (1) device tensor (negative: a
    kpx_status raised by the union pass).  No host sync."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=pts.device)
    cnt = torch.empty(1, dtype=torch.int32, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_dbscan_workspace_bytes(n))
    L.check(lib.kpx_cluster_dbscan(L.ptr(pts), n, float(eps), int(min_points), L.ptr(labels), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    return labels, cnt


def remove_radius_outlier(pts, nb_points, radius):
    """[O3D] RemoveRadiusOutliers: keep_idx i32 (K) ascending device tensor (K = points with more than nb_points neighbours)."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=pts.device)
    cnt = torch.empty(1, dtype=torch.int32, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_radius_outlier_workspace_bytes(n))
    L.check(lib.kpx_remove_radius_outlier(L.ptr(pts), n, int(nb_points), float(radius), L.ptr(idx), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    k = _count(cnt)[0]
    return idx[:k]


def iss_saliency(pts, salient_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """[O3D] ComputeISSKeypoints, first half: saliency f64 (N) device tensor -- the smallest eigenvalue of the covariance of the
    points within salient_radius where both eigenvalue ratios pass, else 0 (include/kinectpx.h).  No host sync."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    sal = torch.empty(n, dtype=torch.float64, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_iss_workspace_bytes(n))
    L.check(lib.kpx_iss_saliency(L.ptr(pts), n, float(salient_radius), float(gamma_21), float(gamma_32), int(min_neighbors), L.ptr(sal), ws, wsz,
                                 L.stream_ptr()))
    return sal


def iss_nonmax(pts, saliency, non_max_radius, min_neighbors=5):
    """[O3D] ComputeISSKeypoints, second half, for ANY saliency f64 (N): keep_idx i32 (K) ascending device tensor of the points with
    saliency > 0, at least min_neighbors points within non_max_radius and no larger saliency among them."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    sal = _dev(saliency, torch.float64).reshape(-1)
    if sal.numel() != n:
        raise L.KinectPxError(f"iss_nonmax: {sal.numel()} saliencies for {n} points")
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=pts.device)
    cnt = torch.empty(1, dtype=torch.int32, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_iss_workspace_bytes(n))
    L.check(lib.kpx_iss_nonmax(L.ptr(pts), n, L.ptr(sal), float(non_max_radius), int(min_neighbors), L.ptr(idx), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    k = _count(cnt)[0]
    return idx[:k]


def model_resolution(pts):
    """[O3D] ComputeModelResolution: the mean over all points of the distance to the nearest OTHER point, as an f64 (1) device
    tensor (0 for an empty cloud).  The sum is exact (128-bit fixed point), so the value is the same bits run to run.  No host sync."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    out = torch.zeros(1, dtype=torch.float64, device=pts.device)
    if n == 0:
        return out
    _, d2, cnt = search_knn(search_index(pts), pts, 2)
    ws, wsz = L.workspace(256)
    L.check(lib.kpx_mean_nn_distance(L.ptr(d2), L.ptr(cnt), n, int(d2.shape[1]), L.ptr(out), ws, wsz, L.stream_ptr()))
    return out


def iss_keypoints(pts, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, want_saliency=False):
    """[O3D] ComputeISSKeypoints: keep_idx i32 (K) ascending device tensor (and the saliency f64 (N) with want_saliency).  Either
    radius 0: BOTH are replaced by 6 x and 4 x model_resolution(pts) -- one host read; the count is the other."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    sal = torch.empty(n, dtype=torch.float64, device=pts.device)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=pts.device)
    if n == 0:
        return (idx[:0], sal) if want_saliency else idx[:0]
    salient_radius, non_max_radius = float(salient_radius), float(non_max_radius)
    if salient_radius == 0.0 or non_max_radius == 0.0:
        resolution = float(model_resolution(pts).item())
        salient_radius, non_max_radius = 6.0 * resolution, 4.0 * resolution
        if not resolution > 0.0:                      # one point, or nothing but duplicates: no neighbourhood has a covariance
            sal.zero_()
            return (idx[:0], sal) if want_saliency else idx[:0]
    cnt = torch.empty(1, dtype=torch.int32, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_iss_workspace_bytes(n))
    L.check(lib.kpx_iss_keypoints(L.ptr(pts), n, salient_radius, non_max_radius, float(gamma_21), float(gamma_32), int(min_neighbors), L.ptr(sal),
                                  L.ptr(idx), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    k = _count(cnt)[0]
    return (idx[:k], sal) if want_saliency else idx[:k]


def farthest_point_sample(pts, k, start_index=0, want_cover=False):
    """[O3D] FarthestPointDownSample's loop: sel i32 (k) device tensor in selection order (repeats kept: the previous index
    repeats once every distance is 0), cover f64 (k) | None -- the largest running distance after each sample.  No host sync."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n, k = pts.shape[0], int(k)
    sel = torch.empty(max(k, 1), dtype=torch.int32, device=pts.device)
    cover = torch.empty(max(k, 1), dtype=torch.float64, device=pts.device) if want_cover else None
    ws, wsz = L.workspace(lib.kpx_fps_workspace_bytes(1, n))
    L.check(lib.kpx_farthest_point_sample(L.ptr(pts), n, k, int(start_index), L.ptr(sel), L.ptr(cover), ws, wsz, L.stream_ptr()))
    return sel[:k], (cover[:k] if cover is not None else None)


def farthest_point_sample_batch(clouds, k, start_index=0):
    """farthest_point_sample of several clouds with one k and start_index (clouds up to KPX_FPS_BLOCK_MAX_N points share one
    launch).  Returns sel i32 (count, k), cover f64 (count, k) device tensors."""
    lib = L.load()
    clouds = [_dev(p, torch.float32).reshape(-1, 3) for p in clouds]
    cnt, k = len(clouds), int(k)
    dev = clouds[0].device if cnt else L.device()
    sel = torch.empty((cnt, max(k, 1)), dtype=torch.int32, device=dev)
    cover = torch.empty((cnt, max(k, 1)), dtype=torch.float64, device=dev)
    if cnt == 0:
        return sel[:, :k], cover[:, :k]
    n_arr = np.array([p.shape[0] for p in clouds], dtype=np.int64)
    arr = lambda ts: C.cast((C.c_void_p * cnt)(*[t.data_ptr() for t in ts]), C.c_void_p)
    ws, wsz = L.workspace(lib.kpx_fps_workspace_bytes(cnt, int(n_arr.max())))
    L.check(lib.kpx_farthest_point_sample_batch(cnt, arr(clouds), n_arr.ctypes.data_as(C.c_void_p), k, int(start_index), arr(sel),
                                                arr(cover), ws, wsz, L.stream_ptr()))
    return sel[:, :k], cover[:, :k]


def estimate_normals(pts, radius, max_nn):
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    out = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_normals_workspace_bytes(n, int(max_nn)))
    L.check(lib.kpx_estimate_normals(L.ptr(pts), n, float(radius), int(max_nn), L.ptr(out), ws, wsz, L.stream_ptr()))
    return out


# ---- neighbour search between a cloud and arbitrary queries ---------------------------
SEARCH_MAX_K = 4096


class SearchIndex:
    """Opaque holder of a search index: the device buffer kpx_search_index_build filled and the number of points it holds.  The
    buffer is self-contained (it does not refer to the cloud it was built from)."""

    def __init__(self, buf, n):
        self.buf, self.n = buf, int(n)

    def __len__(self):
        return self.n


def search_index(pts):
    """index of a float32 (N,3) cloud for search_knn / search_hybrid / search_radius (float64 input is rounded to float32)"""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    buf = torch.empty(lib.kpx_search_index_bytes(n), dtype=torch.uint8, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_search_workspace_bytes(n, 0))
    L.check(lib.kpx_search_index_build(L.ptr(pts), n, L.ptr(buf), buf.numel(), ws, wsz, L.stream_ptr()))
    return SearchIndex(buf, n)


def _search_knn(index, queries, k, radius):
    lib = L.load()
    q = _dev(queries, torch.float32).reshape(-1, 3)
    m, k = q.shape[0], int(k)
    idx = torch.empty((m, max(k, 1)), dtype=torch.int32, device=q.device)
    d2 = torch.empty((m, max(k, 1)), dtype=torch.float64, device=q.device)
    cnt = torch.empty(m, dtype=torch.int32, device=q.device)
    ws, wsz = L.workspace(lib.kpx_search_workspace_bytes(m, max(k, 1)))
    L.check(lib.kpx_search_knn(L.ptr(index.buf), index.buf.numel(), L.ptr(q), m, k, float(radius), L.ptr(idx), L.ptr(d2), L.ptr(cnt), ws, wsz,
                               L.stream_ptr()))
    return idx, d2, cnt


def search_knn(index, queries, k):
    """[O3D] KDTreeFlann.SearchKNN for M queries: idx i32 (M,k), d2 f64 (M,k), count i32 (M) device tensors; row q holds the
    count[q] = min(k, N) nearest points ascending in (d2, index), then -1 / +inf."""
    return _search_knn(index, queries, k, 0.0)


def search_hybrid(index, queries, radius, max_nn):
    """[O3D] KDTreeFlann.SearchHybrid for M queries: the first min(max_nn, count) entries of the radius result (d2 < radius^2,
    strict); same layout as search_knn."""
    if not float(radius) > 0.0:
        raise L.KinectPxError("search_hybrid: radius must be positive")
    return _search_knn(index, queries, max_nn, radius)


def search_radius(index, queries, radius):
    """[O3D] KDTreeFlann.SearchRadius for M queries as a CSR: offsets i64 (M+1), idx i32 (total), d2 f64 (total) device tensors;
    segment q = [offsets[q], offsets[q+1]) holds every point with d2 < radius^2 (strict) ascending in (d2, index).  One host read
    (the total) between the count pass and the fill pass."""
    lib = L.load()
    q = _dev(queries, torch.float32).reshape(-1, 3)
    m = q.shape[0]
    offsets = torch.empty(m + 1, dtype=torch.int64, device=q.device)
    ws, wsz = L.workspace(lib.kpx_search_workspace_bytes(m, 1))
    L.check(lib.kpx_search_radius_count(L.ptr(index.buf), index.buf.numel(), L.ptr(q), m, float(radius), L.ptr(offsets), ws, wsz, L.stream_ptr()))
    total = int(offsets[m].item())
    if total > 2**31 - 1:
        raise L.KinectPxError(f"search_radius: {total} entries, more than 2^31 - 1")
    idx = torch.empty(total, dtype=torch.int32, device=q.device)
    d2 = torch.empty(total, dtype=torch.float64, device=q.device)
    L.check(lib.kpx_search_radius_fill(L.ptr(index.buf), index.buf.numel(), L.ptr(q), m, float(radius), L.ptr(offsets), total, L.ptr(idx),
                                       L.ptr(d2), ws, wsz, L.stream_ptr()))
    return offsets, idx, d2


def segment_plane(pts, distance_threshold, ransac_n, num_iterations, probability=0.99999999, seed=0):
    """a21.  Returns plane (numpy f64 (4,)), inlier idx i32 (K) device tensor."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    dev = pts.device
    plane = torch.zeros(4, dtype=torch.float64, device=dev)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, wsz = L.workspace(lib.kpx_segment_plane_workspace_bytes(n, int(ransac_n), int(num_iterations)))
    L.check(lib.kpx_segment_plane(L.ptr(pts), n, float(distance_threshold), int(ransac_n), int(num_iterations),
                                  float(probability), C.c_uint64(int(seed)), L.ptr(plane), L.ptr(idx), L.ptr(cnt), ws,
                                  wsz, L.stream_ptr()))
    k = _count(cnt)[0]
    return plane.cpu().numpy(), idx[:k]


# ---- registration -----------------------------------------------------------------------------------
def nn_search(src, tgt, T=None):
    """One correspondence search.  Returns idx i32 (N), d2 f64 (N)."""
    lib = L.load()
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    dev = src.device
    Td = torch.as_tensor(_T(np.eye(4) if T is None else T)).to(dev)
    n, m = src.shape[0], tgt.shape[0]
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    ws, wsz = L.workspace(lib.kpx_nn_workspace_bytes(n, m))
    L.check(lib.kpx_nn_search(L.ptr(src), n, L.ptr(tgt), m, L.ptr(Td), L.ptr(idx), L.ptr(d2), ws, wsz, L.stream_ptr()))
    return idx, d2


def registration_eval(src, tgt, max_dist, T=None, want_corr=False):
    """[O3D] evaluate_registration + get_information_matrix_from_point_clouds at T (no ICP): one correspondence search, one
    reduction.  Returns dict(fitness, inlier_rmse, count, information (6,6) float64[, idx, d2])."""
    lib = L.load()
    if not max_dist > 0:
        raise L.KinectPxError("Invalid max_correspondence_distance.")
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    dev = src.device
    Td = torch.as_tensor(_T(np.eye(4) if T is None else T)).to(dev)
    n, m = src.shape[0], tgt.shape[0]
    res = torch.empty(40, dtype=torch.float64, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev) if want_corr else None
    d2 = torch.empty(n, dtype=torch.float64, device=dev) if want_corr else None
    ws, wsz = L.workspace(lib.kpx_registration_eval_workspace_bytes(n, m))
    L.check(lib.kpx_registration_eval(L.ptr(src), n, L.ptr(tgt), m, L.ptr(Td), float(max_dist), L.ptr(res), L.ptr(idx), L.ptr(d2),
                                      ws, wsz, L.stream_ptr()))
    r = res.cpu().numpy()
    out = {"fitness": float(r[0]), "inlier_rmse": float(r[1]), "count": int(r[2]), "information": r[4:40].reshape(6, 6).copy()}
    if want_corr:
        out["idx"], out["d2"] = idx, d2
    return out


def kabsch(src, tgt, corr):
    lib = L.load()
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    corr = _dev(corr, torch.int32).reshape(-1, 2)
    T = torch.zeros(16, dtype=torch.float64, device=src.device)
    ws, wsz = L.workspace(lib.kpx_kabsch_workspace_bytes(corr.shape[0]))
    L.check(lib.kpx_kabsch(L.ptr(src), L.ptr(tgt), L.ptr(corr), corr.shape[0], L.ptr(T), ws, wsz, L.stream_ptr()))
    return T.cpu().numpy().reshape(4, 4)


def icp(src, tgt, max_dist, init=None, mode="p2p", tgt_normals=None, max_iteration=30, relative_fitness=1e-6,
        relative_rmse=1e-6, want_corr=False, poll_interval=4, loss=None):
    """registration_icp.  Returns dict(transformation, fitness, inlier_rmse, iterations, count[, idx, d2]).
    loss: a robust kernel for mode="p2plane" (see _loss; kpx_icp_robust); None or L2 is the plain call."""
    kind, k = _loss(loss)
    if kind and mode == "p2p":
        raise ValueError("TransformationEstimationPointToPoint takes no robust kernel (Open3D has none): use mode='p2plane'")
    lib = L.load()
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    dev = src.device
    n, m = src.shape[0], tgt.shape[0]
    tn = _dev(tgt_normals, torch.float32).reshape(-1, 3) if tgt_normals is not None else None
    md = {"p2p": 0, "p2plane": 1}[mode]
    if md == 1 and tn is None:
        raise L.KinectPxError("TransformationEstimationPointToPlane requires target normals")
    res = torch.zeros(20, dtype=torch.float64, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev) if want_corr else None
    d2 = torch.empty(n, dtype=torch.float64, device=dev) if want_corr else None
    init = _T(np.eye(4) if init is None else init)
    ws, wsz = L.workspace(lib.kpx_icp_workspace_bytes(n, m))
    args = (L.ptr(src), n, L.ptr(tgt), L.ptr(tn), m, float(max_dist), L.hptr(init), md, int(max_iteration),
            float(relative_fitness), float(relative_rmse), int(poll_interval), L.ptr(res), L.ptr(idx), L.ptr(d2), ws, wsz,
            L.stream_ptr())
    L.check(lib.kpx_icp_robust(*args, kind, k) if kind else lib.kpx_icp(*args))
    r = res.cpu().numpy()
    out = {"transformation": r[:16].reshape(4, 4).copy(), "fitness": float(r[16]), "inlier_rmse": float(r[17]),
           "iterations": int(r[18]), "count": int(r[19])}
    if want_corr:
        out["idx"], out["d2"] = idx, d2
    return out


def fpfh(pts, normals, radius, max_nn):
    """a11: compute_fpfh_feature.  Returns (N, 33) float64 device tensor."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    nrm = _dev(normals, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    out = torch.zeros((n, 33), dtype=torch.float64, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_fpfh_workspace_bytes(n, int(max_nn)))
    L.check(lib.kpx_fpfh(L.ptr(pts), L.ptr(nrm), n, float(radius), int(max_nn), L.ptr(out), ws, wsz, L.stream_ptr()))
    return out


def feature_nn(fa, fb):
    lib = L.load()
    fa = _dev(fa, torch.float64).reshape(-1, 33)
    fb = _dev(fb, torch.float64).reshape(-1, 33)
    idx = torch.empty(fa.shape[0], dtype=torch.int32, device=fa.device)
    ws, wsz = L.workspace(lib.kpx_feature_nn_workspace_bytes(fa.shape[0], fb.shape[0]))
    L.check(lib.kpx_feature_nn(L.ptr(fa), fa.shape[0], L.ptr(fb), fb.shape[0], L.ptr(idx), ws, wsz, L.stream_ptr()))
    return idx


def feature_correspondences(fs, ft, mutual_filter=True, ransac_n=3):
    """correspondence stage of registration_ransac_based_on_feature_matching -> int32 (C, 2) numpy array"""
    ij = feature_nn(fs, ft).cpu().numpy()
    one_way = np.stack([np.arange(len(ij), dtype=np.int32), ij], 1)
    if not mutual_filter:
        return one_way
    ji = feature_nn(ft, fs).cpu().numpy()
    mutual = one_way[ji[ij] == np.arange(len(ij))]
    return mutual if len(mutual) >= ransac_n * 3 else one_way


def ransac_corres(src, tgt, corres, max_dist, ransac_n=3, edge_similarity=0.95, max_iteration=250000, confidence=0.999, seed=0):
    """a13: RegistrationRANSACBasedOnCorrespondence.  Returns dict(transformation, fitness, inlier_rmse, iterations, validations)."""
    lib = L.load()
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    corres = _dev(corres, torch.int32).reshape(-1, 2)
    res = np.zeros(20)
    ws, wsz = L.workspace(lib.kpx_ransac_workspace_bytes(src.shape[0], tgt.shape[0]))
    L.check(lib.kpx_ransac_corres(L.ptr(src), src.shape[0], L.ptr(tgt), tgt.shape[0], L.ptr(corres), corres.shape[0], float(max_dist),
                                  int(ransac_n), float(edge_similarity), int(max_iteration), float(confidence), C.c_uint64(int(seed)),
                                  L.hptr(res), ws, wsz, L.stream_ptr()))
    return {"transformation": res[:16].reshape(4, 4).copy(), "fitness": float(res[16]), "inlier_rmse": float(res[17]),
            "iterations": int(res[18]), "validations": int(res[19])}


def fgr_tuple_test(src, tgt, corres, tuple_scale=0.95, maximum_tuple_count=1000, seed=0):
    """[O3D] the tuple test of FastGlobalRegistration: 100 trials per correspondence of three correspondences each (Philox, `seed`);
    a trial passes when its three edge lengths agree within tuple_scale on both sides.  Returns the three pairs of each of the
    first maximum_tuple_count passing trials, in trial order, as an int32 (3 K, 2) device tensor (duplicates stay)."""
    lib = L.load()
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    corres = _dev(corres, torch.int32).reshape(-1, 2)
    nc = corres.shape[0]
    cap = 3 * min(int(maximum_tuple_count), 100 * nc)
    pairs = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=src.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=src.device)
    ws, wsz = L.workspace(lib.kpx_fgr_workspace_bytes(nc))
    L.check(lib.kpx_fgr_tuple_test(L.ptr(src), src.shape[0], L.ptr(tgt), tgt.shape[0], L.ptr(corres), nc, float(tuple_scale),
                                   int(maximum_tuple_count), C.c_uint64(int(seed)), L.ptr(pairs), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    return pairs[:_count(cnt)[0]]


def fgr_optimize(src, tgt, corres, division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
                 iteration_number=64):
    """[O3D] the optimisation of FastGlobalRegistration over the correspondences as given (one launch).  Returns
    dict(transformation (source -> target), par, iterations, failed_solves, scale)."""
    lib = L.load()
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    corres = _dev(corres, torch.int32).reshape(-1, 2)
    res = np.zeros(20)
    res[:16] = np.eye(4).reshape(-1)
    ws, wsz = L.workspace(lib.kpx_fgr_workspace_bytes(corres.shape[0]))
    L.check(lib.kpx_fgr_optimize(L.ptr(src), src.shape[0], L.ptr(tgt), tgt.shape[0], L.ptr(corres), corres.shape[0], float(division_factor),
                                 int(bool(use_absolute_scale)), int(bool(decrease_mu)), float(maximum_correspondence_distance),
                                 int(iteration_number), L.hptr(res), ws, wsz, L.stream_ptr()))
    return {"transformation": res[:16].reshape(4, 4).copy(), "par": float(res[16]), "iterations": int(res[17]),
            "failed_solves": int(res[18]), "scale": float(res[19])}


def icp_batch(srcs, tgt, max_dist, inits, mode="p2p", tgt_normals=None, max_iteration=30, relative_fitness=1e-6,
              relative_rmse=1e-6):
    """Several registrations onto one shared target, software-pipelined on the current stream.
    Returns a list of dicts like icp()."""
    lib = L.load()
    srcs = [_dev(s, torch.float32).reshape(-1, 3) for s in srcs]
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    dev = tgt.device
    cnt, m = len(srcs), tgt.shape[0]
    tn = _dev(tgt_normals, torch.float32).reshape(-1, 3) if tgt_normals is not None else None
    md = {"p2p": 0, "p2plane": 1}[mode]
    if md == 1 and tn is None:
        raise L.KinectPxError("TransformationEstimationPointToPlane requires target normals")
    n_arr = np.array([s.shape[0] for s in srcs], dtype=np.int64)
    p_arr = (C.c_void_p * cnt)(*[s.data_ptr() for s in srcs])
    init = np.ascontiguousarray(np.stack([_T(np.eye(4) if T is None else T) for T in inits]))
    res = torch.empty((cnt, 20), dtype=torch.float64, device=dev)
    ws, wsz = L.workspace(lib.kpx_icp_batch_workspace_bytes(cnt, n_arr.ctypes.data_as(C.c_void_p), m))
    L.check(lib.kpx_icp_batch(cnt, C.cast(p_arr, C.c_void_p), n_arr.ctypes.data_as(C.c_void_p), L.ptr(tgt), L.ptr(tn), m,
                              float(max_dist), L.hptr(init), md, int(max_iteration), float(relative_fitness),
                              float(relative_rmse), L.ptr(res), ws, wsz, L.stream_ptr()))
    r = res.cpu().numpy()
    if np.isnan(r[:, 16]).any():      # icp_chain_kernel poisons the results of a chain that gave up its residency wait: THIS call's error
        raise L.KinectPxError("kpx_icp_batch: the one-launch ICP chain of registration(s) %s gave up waiting for its blocks to become resident "
                              "(another process on this GPU?); KPX_ICP_CHAIN=0 selects the launch-per-iteration form" % np.flatnonzero(np.isnan(r[:, 16])).tolist())
    return [{"transformation": r[i, :16].reshape(4, 4).copy(), "fitness": float(r[i, 16]), "inlier_rmse": float(r[i, 17]),
             "iterations": int(r[i, 18]), "count": int(r[i, 19])} for i in range(cnt)]


def host_resources():
    """kpx_host_resources: what the library's per-thread owners hold right now, summed over the host threads of the process
    -> {"pinned_bytes", "streams", "events", "threads"}.  A thread's share is given back when the thread ends."""
    out = np.zeros(4, dtype=np.uint64)
    L.check(L.load().kpx_host_resources(out.ctypes.data_as(C.c_void_p)))
    return dict(zip(("pinned_bytes", "streams", "events", "threads"), (int(v) for v in out)))


# ---- the frame loop as one native call ---------------------------------------------------------------------
class FrameParams(C.Structure):
    _fields_ = [("reg_voxel", C.c_double), ("icp_max_dist", C.c_double), ("filt_voxel", C.c_double), ("filt_ratio", C.c_double),
                ("gate", C.c_double), ("normals_nn", C.c_int32), ("icp_mode", C.c_int32), ("icp_max_iteration", C.c_int32),
                ("filt_k", C.c_int32)]


def frame_step(depth, rgb, xy_table, inits, params: FrameParams, out=None):
    """kpx_frame_step: depth (S, n_px) u16, rgb (S, n_px, 3) u8, xy (n_px*2) f32 on the device; inits: (S-1) 4x4.
    -> points f32 (K,3), colours f32 (K,3), transforms f64 (S,4,4) numpy, info int32 (64) numpy.
    depth / rgb may also be HOST tensors (pinned: the copy is asynchronous): kpx_frame_step_host stages them through the
    workspace on the frame's stream -- the frame then starts in host memory, as SURVEY 8(d) defines the end-to-end interval.
    out: optional (points, colours) buffers of S*n_px rows to write into (otherwise allocated)."""
    lib = L.load()
    host = isinstance(depth, torch.Tensor) and not depth.is_cuda
    if host:
        if depth.dtype != torch.uint16 or rgb.dtype != torch.uint8 or not (depth.is_contiguous() and rgb.is_contiguous()):
            raise ValueError("frame_step: host frames must be contiguous uint16 depth / uint8 rgb tensors")
        dev = L.device()
    else:
        depth = _dev(depth, torch.uint16)
        dev = depth.device
    S = int(depth.shape[0])
    depth = depth.reshape(S, -1)
    n_px = int(depth.shape[1])
    rgb = (rgb if host else _dev(rgb, torch.uint8)).reshape(S, n_px, 3)
    xy = _dev(xy_table, torch.float32).reshape(-1)
    init = np.ascontiguousarray(np.stack([_T(T) for T in inits])) if S > 1 else np.zeros((1, 4, 4))
    if out is None:
        out = (torch.empty((S * n_px, 3), dtype=torch.float32, device=dev), torch.empty((S * n_px, 3), dtype=torch.float32, device=dev))
    h_count = np.zeros(1, dtype=np.int32)
    h_T = np.zeros((S, 4, 4))
    h_info = np.zeros(64, dtype=np.int32)
    # one size for both forms (the host form's staging buffers are a few MB on top): a stream that sees frames of either kind
    # never regrows its scratch
    ws, wsz = L.workspace(lib.kpx_frame_step_host_workspace_bytes(S, n_px))
    if host:
        fn, dptr, cptr = lib.kpx_frame_step_host, C.c_void_p(depth.data_ptr()), C.c_void_p(rgb.data_ptr())
    else:
        fn, dptr, cptr = lib.kpx_frame_step, L.ptr(depth), L.ptr(rgb)
    L.check(fn(dptr, cptr, L.ptr(xy), n_px, S, L.hptr(init), C.byref(params), L.ptr(out[0]), L.ptr(out[1]),
               h_count.ctypes.data_as(C.c_void_p), L.hptr(h_T), h_info.ctypes.data_as(C.c_void_p), ws, wsz, L.stream_ptr()))
    k = int(h_count[0])
    return out[0][:k], out[1][:k], h_T, h_info


def frame_step_sharded(comm, order, frame, depth, rgb, xy_table, n_sensors, inits, params: FrameParams, fused_filter=0, out=None):
    """kpx_frame_step_sharded: this rank's share of the frame (depth (S_local, n_px) u16, rgb (S_local, n_px, 3) u8, on the device or
    in host memory), the collectives issued natively through `comm` (parallel.NativeComm).  inits: the n_sensors - 1 initial
    transforms of ALL sub sensors.  -> (points, colours, transforms (n_sensors,4,4), info) or L.RETRY when a message outgrew its
    capacity on every rank alike (run the frame again)."""
    lib = L.load()
    host = isinstance(depth, torch.Tensor) and not depth.is_cuda
    if host:
        if depth.dtype != torch.uint16 or rgb.dtype != torch.uint8 or not (depth.is_contiguous() and rgb.is_contiguous()):
            raise ValueError("frame_step_sharded: host frames must be contiguous uint16 depth / uint8 rgb tensors")
        dev = L.device()
    else:
        depth = _dev(depth, torch.uint16)
        rgb = _dev(rgb, torch.uint8)
        dev = depth.device
    S, S_l = int(n_sensors), int(depth.shape[0])
    n_px = int(depth.numel() // max(S_l, 1))
    xy = _dev(xy_table, torch.float32).reshape(-1)
    init = np.ascontiguousarray(np.stack([_T(T) for T in inits])) if S > 1 else np.zeros((1, 4, 4))
    if out is None:
        out = (torch.empty((S * n_px, 3), dtype=torch.float32, device=dev), torch.empty((S * n_px, 3), dtype=torch.float32, device=dev))
    h_count = np.zeros(1, dtype=np.int32)
    h_T = np.zeros((S, 4, 4))
    h_info = np.zeros(64, dtype=np.int32)
    # one size for device and host frames: a stream that sees both never regrows its scratch
    ws, wsz = L.workspace(lib.kpx_frame_step_sharded_workspace_bytes(S, comm.rank, comm.world, n_px, 1))
    rc = lib.kpx_frame_step_sharded(comm.handle, None if order is None else order.handle, -1 if frame is None else int(frame),
                                    C.c_void_p(depth.data_ptr()), C.c_void_p(rgb.data_ptr()), 1 if host else 0, L.ptr(xy), n_px, S, L.hptr(init),
                                    C.byref(params), int(fused_filter), L.ptr(out[0]), L.ptr(out[1]), h_count.ctypes.data_as(C.c_void_p), L.hptr(h_T),
                                    h_info.ctypes.data_as(C.c_void_p), ws, wsz, L.stream_ptr())
    if comm.error is not None:
        e, comm.error = comm.error, None
        raise e
    if rc == L.RETRY:
        return L.RETRY
    L.check(rc)
    k = int(h_count[0])
    return out[0][:k], out[1][:k], h_T, h_info


# ---- measurement hooks --------------------------------------------------------------------------------
NN_ENGINES = ("culled", "dense", "dense_fp64")


def nn_engine(name=None):
    """Select the correspondence-search implementation ("culled" default, "dense" all-pairs cross-check); returns the
    name of the engine that was active.  Results are identical; see include/kinectpx.h."""
    prev = L.load().kpx_nn_engine(-1 if name is None else NN_ENGINES.index(name))
    if prev < 0:
        L.check(prev)
    return NN_ENGINES[prev]


PROF_KERNELS = ("nn_mfma", "sor_knn", "plane_score", "compact", "nn_screen", "nn_local")


def prof_stride(stride):
    """time only every stride-th launch of each tagged kernel"""
    L.check(L.load().kpx_prof_stride(int(stride)))


def prof_begin(capacity=65536):
    L.check(L.load().kpx_prof_begin(int(capacity)))


def prof_end():
    """-> {kernel: (total_ms, launches, work)}; work = flops (nn_mfma) or algorithmic bytes"""
    ms = np.zeros(len(PROF_KERNELS))
    cnt = np.zeros(len(PROF_KERNELS), dtype=np.int64)
    work = np.zeros(len(PROF_KERNELS))
    L.check(L.load().kpx_prof_end(L.hptr(ms), cnt.ctypes.data_as(C.c_void_p), L.hptr(work)))
    return {k: (float(ms[i]), int(cnt[i]), float(work[i])) for i, k in enumerate(PROF_KERNELS)}


def prof_icp_phases():
    """-> average microseconds per block and phase of the LAST launch of the ICP iteration kernel (profiler armed), the time
    between the first and the last block start (dispatch ramp) and first start -> last end (span)"""
    out = np.zeros(16)
    L.check(L.load().kpx_prof_icp_phases(L.hptr(out)))
    names = ("update_prologue", "row_prep", "sweep", "pair_epilogue", "block_sums")
    d = {k: float(out[i]) for i, k in enumerate(names)}
    d.update(blocks=int(out[5]), dispatch_ramp_us=float(out[6]), span_us=float(out[7]), slowest={k: float(out[8 + i]) for i, k in enumerate(names)},
             longest_block_us=float(out[13]), blocks_skipped=int(out[14]))
    return d


def sort_pairs_u32(keys, vals, end_bit=32):
    """stable sort of (uint32 key, int32 value) pairs by the low end_bit key bits -> (keys, vals)"""
    lib = L.load()
    keys = _dev(keys, torch.uint32).reshape(-1)
    vals = _dev(vals, torch.int32).reshape(-1)
    n = keys.shape[0]
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    ws, wsz = L.workspace(lib.kpx_sort_pairs_u32_workspace_bytes(n))
    L.check(lib.kpx_sort_pairs_u32(L.ptr(keys), L.ptr(vals), n, int(end_bit), L.ptr(ko), L.ptr(vo), ws, wsz, L.stream_ptr()))
    return ko, vo


def icp_chain(on=-1):
    """the one-launch form of the culled ICP chain on (1) / off (0) for this process; -1 only asks.  -> the previous setting (-2: -> chains launched by this process so far)"""
    return int(L.load().kpx_icp_chain(int(on)))


def prof_icp_chain():
    """-> (64, 48) uint64: the one-launch ICP chain's clock (KPX_ICP_CHAIN_STAMPS=1; slots in kpx_icp.hip, g_chain_stamp), reset by the call"""
    out = np.zeros((64, 48), dtype=np.uint64)
    L.check(L.load().kpx_prof_icp_chain(out.ctypes.data_as(C.c_void_p)))
    return out


def prof_icp_cert():
    """-> counters of the certificate self-check (KPX_ICP_CERT_CHECK=1): rows certified / searched / certified rows whose search
    disagreed (must be 0) and the first disagreement; cleared by the call"""
    out = np.zeros(8, dtype=np.uint64)
    L.check(L.load().kpx_prof_icp_cert(out.ctypes.data_as(C.c_void_p)))
    if int(out[2]) == 0:        # no disagreement: the chain's state at its last launch
        return dict(certified=int(out[0]), searched=int(out[1]), mismatches=0, iteration=int(out[3]), last_motion=float(out[4:5].view(np.float64)[0]),
                    motion=float(out[5:6].view(np.float64)[0]), skin=float(out[6:7].view(np.float64)[0]))
    return dict(certified=int(out[0]), searched=int(out[1]), mismatches=int(out[2]),
                first=dict(iteration=int(out[3]), row=int(out[4]), kept=int(out[5]), found=int(out[6]), key=float(np.uint32(out[7]).view(np.float32))))


def prof_icp_waves(cap=16384):
    """-> per wave of the LAST sweep launch: dict of numpy arrays (sweep_us, tiles, box_trips, mul_trips, groups_kept, with_partner)"""
    raw = np.zeros((cap, 4), dtype=np.uint64)
    cnt = np.zeros(1, dtype=np.int64)
    L.check(L.load().kpx_prof_icp_waves(raw.ctypes.data_as(C.c_void_p), cap, cnt.ctypes.data_as(C.c_void_p)))
    raw = raw[:int(cnt[0])]
    c = raw[:, 2]
    return dict(start=raw[:, 0].astype(np.int64), sweep_us=(raw[:, 1].astype(np.int64) - raw[:, 0].astype(np.int64)) * 0.01,
                tiles=(c & np.uint64(0xFFFF)).astype(np.int64), box_trips=((c >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64),
                mul_trips=((c >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64), groups_kept=((c >> np.uint64(48)) & np.uint64(0xFFFF)).astype(np.int64),
                with_partner=raw[:, 3].astype(np.int64))


# ---- sampler / normaliser ---------------------------------------------------------
NORM_OBB, NORM_OBB_ROT_TRANS, NORM_TRANSLATE, NORM_OBB_ROT = 0, 1, 2, 3
_OBB_ERRORS = {-1: "fewer than 3 distinct points, or all points on one line", -2: "the convex hull did not close",
               -3: "the convex hull is flat (Qhull: initial simplex is flat)"}


def sample_points(pts, k, seed, want_points=True):
    """seeded select_points_randomly (utils/processing.py:259-275) -> (points f32 (k,3) | None, idx i32 (k))"""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n, k = pts.shape[0], int(k)
    if k > n:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    out = torch.empty((k, 3), dtype=torch.float32, device=pts.device) if want_points else None
    idx = torch.empty(k, dtype=torch.int32, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_sample_workspace_bytes(n))
    L.check(lib.kpx_sample_points(L.ptr(pts), n, k, C.c_uint64(int(seed) & (2 ** 64 - 1)), L.ptr(out), L.ptr(idx), ws, wsz,
                                  L.stream_ptr()))
    return out, idx


def obb_batch(x, want_vertices=False, check=True):
    """get_oriented_bounding_box() of every cloud of x: (count, n, 3) or (n, 3), f32 or f64 (other dtypes are read as
    f64).  -> obb f64 (count, 16) on the device [R | centre | extent | hull vertices], u8 (count, n) vertex flags | None.
    check=True reads the status back (one sync) and raises for degenerate clouds, as Qhull does."""
    lib = L.load()
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32):
        x = _dev(x, torch.float64)
    x = _dev(x, x.dtype)
    x = x.reshape((-1,) + tuple(x.shape[-2:]))
    count, n = int(x.shape[0]), int(x.shape[1])
    obb = torch.empty((count, 16), dtype=torch.float64, device=x.device)
    flags = torch.empty((count, n), dtype=torch.uint8, device=x.device) if want_vertices else None
    ws, wsz = L.workspace(lib.kpx_obb_workspace_bytes(count, n))
    L.check(lib.kpx_obb_batch(L.ptr(x), 1 if x.dtype == torch.float64 else 0, count, n, L.ptr(obb), L.ptr(flags), ws, wsz,
                              L.stream_ptr()))
    if check and count:
        st = obb[:, 15].cpu()
        bad = torch.nonzero(st < 0).reshape(-1)
        if bad.numel():
            b = int(bad[0])
            raise L.KinectPxError(f"get_oriented_bounding_box: cloud {b}: {_OBB_ERRORS.get(int(st[b]), 'error')}")
    return obb, flags


def normalize_batch(x, obb, mode, M=None):
    """x f64 (count, rows, 3) -> the normalisation `mode` with the boxes of obb_batch (kpx_normalize_batch)"""
    lib = L.load()
    x = _dev(x, torch.float64)
    count, rows = int(x.shape[0]), int(x.shape[1])
    out = torch.empty_like(x)
    Mh = None if M is None else np.ascontiguousarray(M, dtype=np.float64).reshape(3, 3)
    L.check(lib.kpx_normalize_batch(L.ptr(x), count, rows, L.ptr(obb), int(mode), None if Mh is None else L.hptr(Mh), L.ptr(out),
                                    L.stream_ptr()))
    return out


def fuse_skeletons(skeletons, alpha=1.4, beta=1.4, initial_frame=20):
    """utils/skeleton_fusion.py:21-74.  skeletons (cams, frames, joints, 3) -> fused (frames, joints, 3) f64 on the device"""
    lib = L.load()
    sk = _dev(skeletons, torch.float64)
    if sk.dim() != 4 or sk.shape[3] != 3:
        raise ValueError("skeletons must have shape (cameras, frames, joints, 3)")
    cams, frames, joints = int(sk.shape[0]), int(sk.shape[1]), int(sk.shape[2])
    out = torch.empty((frames, joints, 3), dtype=torch.float64, device=sk.device)
    L.check(lib.kpx_fuse_skeletons(L.ptr(sk), cams, frames, joints, float(alpha), float(beta), int(initial_frame), L.ptr(out), L.stream_ptr()))
    return out


# ---- coloured ICP -------------------------------------------------------------------
def color_gradient(pts, normals, colors, radius, max_nn=30):
    """[O3D] InitializePointCloudForColoredICP: tangent-plane intensity gradient per point, (n, 3) f64 on the device"""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    nrm = _dev(normals, torch.float32).reshape(-1, 3)
    col = _dev(colors, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    grad = torch.zeros((n, 3), dtype=torch.float64, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_color_gradient_workspace_bytes(n, int(max_nn)))
    L.check(lib.kpx_color_gradient(L.ptr(pts), L.ptr(nrm), L.ptr(col), n, float(radius), int(max_nn), L.ptr(grad), ws, wsz, L.stream_ptr()))
    return grad


def colored_icp(src, src_colors, tgt, tgt_colors, tgt_normals, max_dist, init=None, lambda_geometric=0.968, max_iteration=30,
                relative_fitness=1e-6, relative_rmse=1e-6, poll_interval=4, tgt_gradient=None, loss=None):
    """[O3D] registration_colored_icp.  Returns dict(transformation, fitness, inlier_rmse, iterations, count).
    loss: a robust kernel (see _loss; kpx_colored_icp_robust); None or L2 is the plain call."""
    kind, k = _loss(loss)
    lib = L.load()
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    sc = _dev(src_colors, torch.float32).reshape(-1, 3)
    tc = _dev(tgt_colors, torch.float32).reshape(-1, 3)
    tn = _dev(tgt_normals, torch.float32).reshape(-1, 3)
    n, m = src.shape[0], tgt.shape[0]
    if tgt_gradient is None:
        tgt_gradient = color_gradient(tgt, tn, tc, 2.0 * float(max_dist), 30)       # Open3D: KDTreeSearchParamHybrid(2 max_distance, 30)
    tg = _dev(tgt_gradient, torch.float64).reshape(-1, 3)
    res = torch.zeros(20, dtype=torch.float64, device=src.device)
    init = _T(np.eye(4) if init is None else init)
    ws, wsz = L.workspace(lib.kpx_colored_icp_workspace_bytes(n, m))
    args = (L.ptr(src), L.ptr(sc), n, L.ptr(tgt), L.ptr(tc), L.ptr(tn), L.ptr(tg), m, float(max_dist), L.hptr(init),
            float(lambda_geometric), int(max_iteration), float(relative_fitness), float(relative_rmse), int(poll_interval),
            L.ptr(res), ws, wsz, L.stream_ptr())
    L.check(lib.kpx_colored_icp_robust(*args, kind, k) if kind else lib.kpx_colored_icp(*args))
    r = res.cpu().numpy()
    return {"transformation": r[:16].reshape(4, 4).copy(), "fitness": float(r[16]), "inlier_rmse": float(r[17]),
            "iterations": int(r[18]), "count": int(r[19])}


# ---- generalized ICP ----------------------------------------------------------------------------------------
def estimate_covariances(pts, radius, max_nn):
    """[O3D] estimate_covariances: the covariance of each point's estimate_normals neighbourhood (< 3 neighbours: identity),
    (n, 3, 3) f64 on the device"""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    out = torch.empty((n, 3, 3), dtype=torch.float64, device=pts.device)
    ws, wsz = L.workspace(lib.kpx_covariances_workspace_bytes(n, int(max_nn)))
    L.check(lib.kpx_estimate_covariances(L.ptr(pts), n, float(radius), int(max_nn), L.ptr(out), ws, wsz, L.stream_ptr()))
    return out


def gicp_covariances(normals, epsilon=1e-3):
    """[O3D] InitializePointCloudForGeneralizedICP from normals: R_x diag(epsilon, 1, 1) R_x^T, (n, 3, 3) f64 on the device"""
    lib = L.load()
    nrm = _dev(normals, torch.float32).reshape(-1, 3)
    n = nrm.shape[0]
    out = torch.empty((n, 3, 3), dtype=torch.float64, device=nrm.device)
    L.check(lib.kpx_gicp_covariances(L.ptr(nrm), n, float(epsilon), L.ptr(out), L.stream_ptr()))
    return out


def rotate_covariances(cov, T, out=None):
    """R C R^T per point (R = rotation of T); out may be cov"""
    lib = L.load()
    cov = _dev(cov, torch.float64).reshape(-1, 3, 3)
    if out is None:
        out = torch.empty_like(cov)
    L.check(lib.kpx_rotate_covariances(L.ptr(cov), cov.shape[0], L.hptr(_T(T)), L.ptr(out), L.stream_ptr()))
    return out


def generalized_icp(src, src_cov, tgt, tgt_cov, max_dist, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                    want_corr=False, poll_interval=4, loss=None):
    """[O3D] registration_generalized_icp.  Returns dict(transformation, fitness, inlier_rmse, iterations, count[, idx, d2]).
    loss: a robust kernel (see _loss; kpx_generalized_icp_robust); None or L2 is the plain call."""
    kind, k = _loss(loss)
    lib = L.load()
    src = _dev(src, torch.float32).reshape(-1, 3)
    tgt = _dev(tgt, torch.float32).reshape(-1, 3)
    sc = _dev(src_cov, torch.float64).reshape(-1, 3, 3)
    tc = _dev(tgt_cov, torch.float64).reshape(-1, 3, 3)
    n, m = src.shape[0], tgt.shape[0]
    if sc.shape[0] != n or tc.shape[0] != m:
        raise L.KinectPxError("generalized_icp: one covariance per point is required")
    dev = src.device
    res = torch.zeros(20, dtype=torch.float64, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev) if want_corr else None
    d2 = torch.empty(n, dtype=torch.float64, device=dev) if want_corr else None
    init = _T(np.eye(4) if init is None else init)
    ws, wsz = L.workspace(lib.kpx_generalized_icp_workspace_bytes(n, m))
    args = (L.ptr(src), L.ptr(sc), n, L.ptr(tgt), L.ptr(tc), m, float(max_dist), L.hptr(init), int(max_iteration),
            float(relative_fitness), float(relative_rmse), int(poll_interval), L.ptr(res), L.ptr(idx), L.ptr(d2),
            ws, wsz, L.stream_ptr())
    L.check(lib.kpx_generalized_icp_robust(*args, kind, k) if kind else lib.kpx_generalized_icp(*args))
    r = res.cpu().numpy()
    out = {"transformation": r[:16].reshape(4, 4).copy(), "fitness": float(r[16]), "inlier_rmse": float(r[17]),
           "iterations": int(r[18]), "count": int(r[19])}
    if want_corr:
        out["idx"], out["d2"] = idx, d2
    return out


# ---- volumetric integration ---------------------------------------------------------------------------
TSDF_MODES = {"surface": 0, "voxels": 1}          # KPX_TSDF_SURFACE / KPX_TSDF_VOXELS (include/kinectpx.h)


def tsdf_reset(volume, color=None):
    """zero a TSDF volume (f32 (res^3, 2) device tensor {tsdf, weight}) and its colour array (f32 (res^3, 3) or None) in place"""
    volume.zero_()
    if color is not None:
        color.zero_()


def tsdf_integrate(volume, color, resolution, voxel_length, origin, sdf_trunc, depths, rgbs, width, height, intrinsic, extrinsics,
                   depth_scale=1.0, depth_trunc=0.0):
    """[O3D] UniformTSDFVolume.integrate for len(depths) images in one pass over the volume (kpx_tsdf_integrate), in place.  depths:
    device tensors, all float32 (H W) metres-like depth, or all uint16 (H W) raw depth with depth_scale / depth_trunc applied in the
    kernel; rgbs: uint8 (H W 3) per image when `color` is given; intrinsic (fx, fy, cx, cy); extrinsics: (S, 4, 4) world -> camera."""
    lib = L.load()
    cnt = len(depths)
    u16 = cnt > 0 and depths[0].dtype == torch.uint16
    depths = [_dev(d, torch.uint16 if u16 else torch.float32).reshape(-1) for d in depths]
    rgbs = [_dev(c, torch.uint8).reshape(-1) for c in rgbs] if color is not None else None
    n_px = int(width) * int(height)
    if any(d.numel() != n_px for d in depths) or (rgbs is not None and (len(rgbs) != cnt or any(c.numel() != 3 * n_px for c in rgbs))):
        raise L.KinectPxError("tsdf_integrate: image size does not match width x height")
    E = np.ascontiguousarray(np.asarray(extrinsics, dtype=np.float64).reshape(cnt, 16))
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    K = np.ascontiguousarray(np.asarray(intrinsic, dtype=np.float64).reshape(4))
    arr = lambda ts: C.cast((C.c_void_p * max(cnt, 1))(*[t.data_ptr() for t in ts]), C.c_void_p) if ts is not None else None
    L.check(lib.kpx_tsdf_integrate(L.ptr(volume), L.ptr(color), int(resolution), float(voxel_length), L.hptr(org), float(sdf_trunc), cnt,
                                   arr(depths), int(u16), float(depth_scale), float(depth_trunc), arr(rgbs), int(width), int(height),
                                   L.hptr(K), L.hptr(E), L.stream_ptr()))


def tsdf_extract(volume, color, resolution, voxel_length, origin, mode="surface", want_normals=True):
    """[O3D] extract_point_cloud (mode "surface") / extract_voxel_point_cloud ("voxels") -> (points, normals | None, colours | None)
    float32 (K, 3) device tensors.  One host read (the count) between the count pass and the fill pass."""
    lib = L.load()
    m = TSDF_MODES[mode]
    dev = volume.device
    ws = torch.empty(lib.kpx_tsdf_workspace_bytes(int(resolution)), dtype=torch.uint8, device=dev)      # carried from count to fill
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    L.check(lib.kpx_tsdf_extract_count(L.ptr(volume), int(resolution), m, L.ptr(cnt), L.ptr(ws), ws.numel(), L.stream_ptr()))
    total = int(cnt.item())
    pts = torch.empty((total, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((total, 3), dtype=torch.float32, device=dev) if m == 0 and want_normals else None
    col = torch.empty((total, 3), dtype=torch.float32, device=dev) if m == 1 or color is not None else None
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    L.check(lib.kpx_tsdf_extract_fill(L.ptr(volume), L.ptr(color), int(resolution), float(voxel_length), L.hptr(org), m, total, L.ptr(pts),
                                      L.ptr(nrm), L.ptr(col), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return pts, nrm, col


MESH_MAX = 2 ** 31 - 1          # int32 vertex and triangle indices


def tsdf_extract_mesh(volume, color, resolution, voxel_length, origin):
    """[O3D] extract_triangle_mesh (marching cubes, AC12) -> (vertices float32 (V, 3), colours float32 (V, 3) | None, triangles int32
    (T, 3)) device tensors, vertices ascending in (linear voxel index, axis).  One host read (the two counts) between count and fill."""
    lib = L.load()
    dev = volume.device
    ws = torch.empty(lib.kpx_tsdf_mesh_workspace_bytes(int(resolution)), dtype=torch.uint8, device=dev)      # carried from count to fill
    cnt = torch.empty(2, dtype=torch.int64, device=dev)
    L.check(lib.kpx_tsdf_mesh_count(L.ptr(volume), int(resolution), L.ptr(cnt), L.ptr(ws), ws.numel(), L.stream_ptr()))
    nv, nt = (int(c) for c in cnt.tolist())
    if nv > MESH_MAX or nt > MESH_MAX:
        raise L.KinectPxError(f"tsdf_extract_mesh: {nv} vertices and {nt} triangles: a mesh holds fewer than 2^31 of each")
    vert = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    col = torch.empty((nv, 3), dtype=torch.float32, device=dev) if color is not None else None
    tri = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    L.check(lib.kpx_tsdf_mesh_fill(L.ptr(volume), L.ptr(color), int(resolution), float(voxel_length), L.hptr(org), nv, nt, L.ptr(vert), L.ptr(col),
                                   L.ptr(tri), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return vert, col, tri


# ---- block-sparse volumetric integration (ScalableTSDFVolume, AC16) --------------------------------------
def _ptr_array(ts, cnt):
    return C.cast((C.c_void_p * max(cnt, 1))(*[t.data_ptr() for t in ts]), C.c_void_p) if ts is not None else None


def tsdf_blocks_touch(index_keys, index_slots, depths, width, height, intrinsic, poses, stride, unit_length, sdf_trunc, depth_scale=1.0,
                      depth_trunc=0.0):
    """The blocks that len(depths) <= 8 images touch (kpx_tsdf_blocks_touch): depths as tsdf_integrate's, poses (S, 4, 4) camera ->
    world.  -> (touched, new, ws): the two counts (the one host read of an integration) and the workspace that tsdf_blocks_insert
    and tsdf_blocks_integrate continue from.  A block index outside [-2^20, 2^20) raises."""
    lib = L.load()
    cnt = len(depths)
    dev = L.device()
    size = lib.kpx_tsdf_blocks_touch_workspace_bytes(cnt, int(width), int(height), int(stride), float(unit_length), float(sdf_trunc))
    if size == 0:
        raise L.KinectPxError("tsdf_blocks_touch: 1 to 8 images of a positive size, stride >= 1 and 0 < sdf_trunc <= unit length")
    if any(d.numel() != int(width) * int(height) for d in depths):
        raise L.KinectPxError("tsdf_blocks_touch: image size does not match width x height")
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(cnt, 16))
    K = np.ascontiguousarray(np.asarray(intrinsic, dtype=np.float64).reshape(4))
    u16 = depths[0].dtype == torch.uint16
    L.check(lib.kpx_tsdf_blocks_touch(L.ptr(index_keys), L.ptr(index_slots), 0 if index_keys is None else index_keys.numel(), cnt,
                                      _ptr_array(depths, cnt), int(u16), float(depth_scale), float(depth_trunc), int(width), int(height), L.hptr(K),
                                      L.hptr(P), int(stride), float(unit_length), float(sdf_trunc), L.ptr(counts), L.ptr(ws), ws.numel(), L.stream_ptr()))
    touched, new, err = (int(c) for c in counts.tolist())
    if err:
        raise L.KinectPxError("tsdf_blocks_touch: a block index outside [-2^20, 2^20) (KPX_ERR_RANGE): the scene is too far from the origin for this unit length")
    return touched, new, ws


def tsdf_blocks_insert(index_keys, index_slots, n_new, pool, color_pool, unit_resolution, shape, ws):
    """the index merged with the n_new new keys a touch left in ws -> (keys int64 (B + n_new,), slots int32); the new pool slots (B,
    B + 1, ... in ascending key order) are zeroed.  shape = the touch's (count, width, height, stride, unit_length, sdf_trunc)."""
    lib = L.load()
    nb = 0 if index_keys is None else index_keys.numel()
    keys = torch.empty(nb + n_new, dtype=torch.int64, device=pool.device)
    slots = torch.empty(nb + n_new, dtype=torch.int32, device=pool.device)
    cnt, width, height, stride, ul, trunc = shape
    L.check(lib.kpx_tsdf_blocks_insert(L.ptr(index_keys), L.ptr(index_slots), nb, int(n_new), L.ptr(keys), L.ptr(slots), L.ptr(pool), L.ptr(color_pool),
                                       pool.shape[0], int(unit_resolution), int(cnt), int(width), int(height), int(stride), float(ul), float(trunc),
                                       L.ptr(ws), ws.numel(), L.stream_ptr()))
    return keys, slots


def tsdf_blocks_integrate(pool, color_pool, unit_resolution, voxel_length, sdf_trunc, n_touched, depths, rgbs, width, height, intrinsic, extrinsics,
                          stride, ws, depth_scale=1.0, depth_trunc=0.0):
    """AC9's update of the n_touched blocks a touch left in ws, each by the images that touch it (kpx_tsdf_blocks_integrate), in place"""
    lib = L.load()
    cnt = len(depths)
    u16 = depths[0].dtype == torch.uint16
    if color_pool is not None and (rgbs is None or len(rgbs) != cnt or any(c.numel() != 3 * int(width) * int(height) for c in rgbs)):
        raise L.KinectPxError("tsdf_blocks_integrate: a colour volume needs one width x height x 3 colour image per depth image")
    E = np.ascontiguousarray(np.asarray(extrinsics, dtype=np.float64).reshape(cnt, 16))
    K = np.ascontiguousarray(np.asarray(intrinsic, dtype=np.float64).reshape(4))
    L.check(lib.kpx_tsdf_blocks_integrate(L.ptr(pool), L.ptr(color_pool), pool.shape[0], int(unit_resolution), float(voxel_length), float(sdf_trunc),
                                          int(n_touched), cnt, _ptr_array(depths, cnt), int(u16), float(depth_scale), float(depth_trunc),
                                          _ptr_array(rgbs if color_pool is not None else None, cnt), int(width), int(height), L.hptr(K), L.hptr(E),
                                          int(stride), L.ptr(ws), ws.numel(), L.stream_ptr()))


def tsdf_blocks_extract(index_keys, index_slots, pool, color_pool, unit_resolution, voxel_length, mode="surface"):
    """extract_point_cloud / extract_voxel_point_cloud over the blocks of the index -> (points, normals | None, colours | None), ascending
    in (block key, local voxel index, axis).  One host read between count and fill."""
    lib = L.load()
    m = TSDF_MODES[mode]
    dev = pool.device
    nb = 0 if index_keys is None else index_keys.numel()
    ws = torch.empty(lib.kpx_tsdf_blocks_extract_workspace_bytes(nb, int(unit_resolution), 0), dtype=torch.uint8, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    L.check(lib.kpx_tsdf_blocks_extract_count(L.ptr(index_keys), L.ptr(index_slots), nb, L.ptr(pool), int(unit_resolution), m, L.ptr(cnt), L.ptr(ws),
                                              ws.numel(), L.stream_ptr()))
    total = int(cnt.item())
    pts = torch.empty((total, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((total, 3), dtype=torch.float32, device=dev) if m == 0 else None
    col = torch.empty((total, 3), dtype=torch.float32, device=dev) if m == 1 or color_pool is not None else None
    L.check(lib.kpx_tsdf_blocks_extract_fill(L.ptr(index_keys), L.ptr(index_slots), nb, L.ptr(pool), L.ptr(color_pool), int(unit_resolution),
                                             float(voxel_length), m, total, L.ptr(pts), L.ptr(nrm), L.ptr(col), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return pts, nrm, col


def tsdf_blocks_extract_mesh(index_keys, index_slots, pool, color_pool, unit_resolution, voxel_length):
    """extract_triangle_mesh (AC12 by global voxel index, AC16) over the blocks of the index -> (vertices, colours | None, triangles)"""
    lib = L.load()
    dev = pool.device
    nb = 0 if index_keys is None else index_keys.numel()
    ws = torch.empty(lib.kpx_tsdf_blocks_extract_workspace_bytes(nb, int(unit_resolution), 1), dtype=torch.uint8, device=dev)
    cnt = torch.empty(2, dtype=torch.int64, device=dev)
    L.check(lib.kpx_tsdf_blocks_mesh_count(L.ptr(index_keys), L.ptr(index_slots), nb, L.ptr(pool), int(unit_resolution), L.ptr(cnt), L.ptr(ws),
                                           ws.numel(), L.stream_ptr()))
    nv, nt = (int(c) for c in cnt.tolist())
    if nv > MESH_MAX or nt > MESH_MAX:
        raise L.KinectPxError(f"tsdf_blocks_extract_mesh: {nv} vertices and {nt} triangles: a mesh holds fewer than 2^31 of each")
    vert = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    col = torch.empty((nv, 3), dtype=torch.float32, device=dev) if color_pool is not None else None
    tri = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    L.check(lib.kpx_tsdf_blocks_mesh_fill(L.ptr(index_keys), L.ptr(index_slots), nb, L.ptr(pool), L.ptr(color_pool), int(unit_resolution),
                                          float(voxel_length), nv, nt, L.ptr(vert), L.ptr(col), L.ptr(tri), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return vert, col, tri


def _mesh_arrays(who, vertices, triangles):
    """device float32 (V, 3) and int32 (T, 3); an index outside [0, V) raises here, before any kernel sees it"""
    vert = _dev(vertices, torch.float32).reshape(-1, 3)
    tri = _dev(triangles, torch.int32).reshape(-1, 3)
    _mesh_index_check(who, tri, vert.shape[0])
    return vert, tri


def _mesh_index_check(who, tri, nv):
    """min and max are taken on the device: two host reads"""
    if tri.shape[0]:
        lo, hi = int(tri.min()), int(tri.max())
        if lo < 0 or hi >= nv:
            raise L.KinectPxError(f"{who}: triangle index out of range [0, {nv})")


def mesh_normals(vertices, triangles, normalized=True, want_triangle=True, want_vertex=True):
    """AC12's normals of a triangle mesh -> (triangle normals float32 (T, 3) | None, vertex normals float32 (V, 3) | None): the fp64
    cross product per triangle; per vertex the sum of the unnormalised normals of its triangles in ascending triangle index."""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_normals", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    tn = torch.empty((nt, 3), dtype=torch.float32, device=vert.device) if want_triangle else None
    vn = torch.empty((nv, 3), dtype=torch.float32, device=vert.device) if want_vertex else None
    ws, wsz = L.workspace(lib.kpx_mesh_normals_workspace_bytes(nv, nt)) if want_vertex else (None, 0)
    L.check(lib.kpx_mesh_normals(L.ptr(vert), nv, L.ptr(tri), nt, int(bool(normalized)), L.ptr(tn), L.ptr(vn), ws, wsz, L.stream_ptr()))
    return tn, vn


def mesh_surface_area(vertices, triangles):
    """sum of the triangles' areas, fp64, in ascending triangle order (AC12) -> float"""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_surface_area", vertices, triangles)
    out = torch.empty(1, dtype=torch.float64, device=vert.device)
    L.check(lib.kpx_mesh_surface_area(L.ptr(vert), vert.shape[0], L.ptr(tri), tri.shape[0], L.ptr(out), L.stream_ptr()))
    return float(out.item())


# ---- mesh clean-up (AC13) -------------------------------------------------------------------------------
MESH_FLAGS = {"referenced": 0, "degenerate": 1, "indices": 2}          # KPX_MESH_FLAG_* (include/kinectpx.h)
MESH_SMOOTH = {"simple": 0, "laplacian": 1, "taubin": 2}               # KPX_MESH_SMOOTH_*


def _mesh_rows(who, t, n, name):
    """an optional per-vertex or per-triangle float32 (n, 3) array on the device, or None"""
    if t is None:
        return None
    t = _dev(t, torch.float32).reshape(-1, 3)
    if t.shape[0] != n:
        raise L.KinectPxError(f"{who}: {t.shape[0]} {name} for {n} rows")
    return t


def _mesh_count(who, cnt):
    """the one host read of a counted operator; a negative count is a kpx_status the kernels left there"""
    c = [int(x) for x in cnt.tolist()]
    if min(c) < 0:
        raise L.KinectPxError(f"{who}: the union-find pass gave up (kpx_status {min(c)})")
    return c


def mesh_adjacency(vertices, triangles):
    """AC13's vertex adjacency as CSR -> (offsets int32 (V + 1,), neighbours int32 (offsets[V],)): row v holds, ascending, the distinct
    vertices that share a corner pair of some triangle with v.  One host read (the length of `neighbours`)."""
    off, nb, cnt = _mesh_adjacency(*_mesh_arrays("mesh_adjacency", vertices, triangles))
    return off, nb[:_mesh_count("mesh_adjacency", cnt)[0]]


def _mesh_adjacency(vert, tri):
    """-> (offsets, neighbours with room for 6 T entries, their number int32 (1,) on the device): no host read.  The entries of
    `neighbours` at and beyond that number are unspecified."""
    lib = L.load()
    nv, nt = vert.shape[0], tri.shape[0]
    off = torch.empty(nv + 1, dtype=torch.int32, device=vert.device)
    nb = torch.empty(6 * nt, dtype=torch.int32, device=vert.device)
    cnt = torch.empty(1, dtype=torch.int32, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_adjacency_workspace_bytes(nv, nt))
    L.check(lib.kpx_mesh_adjacency(L.ptr(tri), nv, nt, L.ptr(off), L.ptr(nb), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    return off, nb, cnt


def mesh_non_manifold_edges(vertices, triangles, allow_boundary_edges=True):
    """[O3D] get_non_manifold_edges -> int32 (E, 2) ascending (min, max): the edges that more than two triangles share, with
    allow_boundary_edges=False also those that only one has.  One host read."""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_non_manifold_edges", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    out = torch.empty((3 * nt, 2), dtype=torch.int32, device=vert.device)
    cnt = torch.empty(1, dtype=torch.int32, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_edges_workspace_bytes(nv, nt))
    L.check(lib.kpx_mesh_non_manifold_edges(L.ptr(tri), nv, nt, int(bool(allow_boundary_edges)), L.ptr(out), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    return out[:_mesh_count("mesh_non_manifold_edges", cnt)[0]]


def mesh_cluster_triangles(vertices, triangles):
    """[O3D] cluster_connected_triangles -> (cluster of each triangle int32 (T,), triangles per cluster int32 (C,), area per cluster
    float64 (C,)) device tensors; clusters are numbered by their smallest triangle index.  One host read (C)."""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_cluster_triangles", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    lab = torch.empty(nt, dtype=torch.int32, device=vert.device)
    num = torch.empty(nt, dtype=torch.int32, device=vert.device)
    area = torch.empty(nt, dtype=torch.float64, device=vert.device)
    cnt = torch.empty(1, dtype=torch.int32, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_cluster_workspace_bytes(nv, nt))
    L.check(lib.kpx_mesh_cluster_triangles(L.ptr(vert), nv, L.ptr(tri), nt, L.ptr(lab), L.ptr(num), L.ptr(area), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    c = _mesh_count("mesh_cluster_triangles", cnt)[0]
    return lab, num[:c], area[:c]


def mesh_flags(kind, triangles, n_vertices, indices=None, n=None):
    """uint8 flags on the device: "referenced" (V,) the vertices some triangle names; "degenerate" (T,) the triangles with two equal
    indices; "indices" (n,) the positions an index list names (values outside [0, n) are ignored).  "referenced" is indexed by the
    triangles' corners and so holds them to [0, V) first, as _mesh_arrays does; the other two read no vertex."""
    lib = L.load()
    tri = _dev(triangles, torch.int32).reshape(-1, 3) if triangles is not None else None
    if kind == "referenced" and tri is not None:
        _mesh_index_check("mesh_flags", tri, int(n_vertices))
    idx = _dev(indices, torch.int64).reshape(-1) if indices is not None else None
    nt = 0 if tri is None else tri.shape[0]
    size = {"referenced": int(n_vertices), "degenerate": nt, "indices": 0 if n is None else int(n)}[kind]
    out = torch.empty(size, dtype=torch.uint8, device=L.device())
    L.check(lib.kpx_mesh_flags(MESH_FLAGS[kind], L.ptr(tri), int(n_vertices), nt, L.ptr(idx), 0 if idx is None else idx.numel(), L.ptr(out), size,
                               L.stream_ptr()))
    return out


def _mesh_flag_bytes(who, flags, n):
    f = flags if isinstance(flags, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(flags).astype(bool)))
    f = f.reshape(-1)
    if f.shape[0] != n:
        raise L.KinectPxError(f"{who}: a mask of {f.shape[0]} entries for {n} rows")
    return _dev(f, torch.uint8)


def mesh_select_triangles(triangles, flags, invert=False, triangle_normals=None):
    """the triangles whose flag is set (invert: not set), in order, with their normals -> (triangles, normals | None).  One host read."""
    lib = L.load()
    tri = _dev(triangles, torch.int32).reshape(-1, 3)
    nt = tri.shape[0]
    f = _mesh_flag_bytes("mesh_select_triangles", flags, nt)
    tn = _mesh_rows("mesh_select_triangles", triangle_normals, nt, "triangle normals")
    otri, otn = torch.empty_like(tri), None if tn is None else torch.empty_like(tn)
    cnt = torch.empty(1, dtype=torch.int32, device=tri.device)
    ws, wsz = L.workspace(lib.kpx_mesh_select_workspace_bytes(0, nt))
    L.check(lib.kpx_mesh_select_triangles(L.ptr(tri), L.ptr(tn), nt, L.ptr(f), int(bool(invert)), L.ptr(otri), L.ptr(otn), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    c = _mesh_count("mesh_select_triangles", cnt)[0]
    return otri[:c], None if otn is None else otn[:c]


def mesh_select_vertices(vertices, triangles, flags, invert=False, colors=None, normals=None, triangle_normals=None):
    """the vertices whose flag is set (invert: not set), in order, renumbered by rank, with their colours and normals; the triangles
    whose three corners stay, in order, with their normals -> (vertices, colours | None, normals | None, triangles, triangle normals |
    None).  One host read (both counts)."""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_select_vertices", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    f = _mesh_flag_bytes("mesh_select_vertices", flags, nv)
    col, nrm = _mesh_rows("mesh_select_vertices", colors, nv, "colours"), _mesh_rows("mesh_select_vertices", normals, nv, "normals")
    tn = _mesh_rows("mesh_select_vertices", triangle_normals, nt, "triangle normals")
    like = lambda t: None if t is None else torch.empty_like(t)
    overt, ocol, onrm, otri, otn = like(vert), like(col), like(nrm), like(tri), like(tn)
    cnt = torch.empty(2, dtype=torch.int32, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_select_workspace_bytes(nv, nt))
    L.check(lib.kpx_mesh_select_vertices(L.ptr(vert), L.ptr(col), L.ptr(nrm), nv, L.ptr(tri), L.ptr(tn), nt, L.ptr(f), int(bool(invert)), L.ptr(overt),
                                         L.ptr(ocol), L.ptr(onrm), L.ptr(otri), L.ptr(otn), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    cv, ct = _mesh_count("mesh_select_vertices", cnt)
    cut = lambda t, c: None if t is None else t[:c]
    return cut(overt, cv), cut(ocol, cv), cut(onrm, cv), cut(otri, ct), cut(otn, ct)


def mesh_smooth(vertices, triangles, method, iterations, lambda_filter=0.5, mu=-0.53, normals=None, colors=None, scope=(True, True, True)):
    """AC13's smoothing: method "simple" | "laplacian" | "taubin"; scope = (vertices, normals, colours): which of the arrays are
    filtered -> (vertices, normals | None, colours | None) float32, every one a new tensor with storage of its own: the filtered
    arrays, and copies of the others.  No host read beyond the index check's: the adjacency stays on the device."""
    lib = L.load()
    if int(iterations) < 0:
        raise L.KinectPxError("filter_smooth: number_of_iterations must be non-negative")
    vert, tri = _mesh_arrays("mesh_smooth", vertices, triangles)
    nv = vert.shape[0]
    nrm, col = _mesh_rows("mesh_smooth", normals, nv, "normals"), _mesh_rows("mesh_smooth", colors, nv, "colours")
    off, nb, _ = _mesh_adjacency(vert, tri)
    out = [torch.empty_like(t) if t is not None and on else None for t, on in zip((vert, nrm, col), scope)]
    ws, wsz = L.workspace(lib.kpx_mesh_smooth_workspace_bytes(nv))
    L.check(lib.kpx_mesh_smooth(L.ptr(vert), L.ptr(nrm), L.ptr(col), nv, L.ptr(off), L.ptr(nb), nb.numel(), MESH_SMOOTH[method], int(iterations),
                                float(lambda_filter), float(mu), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), ws, wsz, L.stream_ptr()))
    return tuple(o if o is not None else (None if t is None else t.clone()) for o, t in zip(out, (vert, nrm, col)))


def mesh_sample_points(vertices, triangles, number_of_points, seed=0, colors=None, vertex_normals=None, triangle_normals=None):
    """AC13's sample_points_uniformly -> (points, colours | None, normals | None) float32 (N, 3), ordered by triangle; normals are
    interpolated from vertex_normals or copied from triangle_normals (give one of them).  One host read (the total area)."""
    lib = L.load()
    n = int(number_of_points)
    if n <= 0:
        raise L.KinectPxError("sample_points_uniformly: number_of_points must be positive")
    vert, tri = _mesh_arrays("mesh_sample_points", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    if nv == 0 or nt == 0:
        raise L.KinectPxError("sample_points_uniformly: the mesh has no triangles")
    col, vn = _mesh_rows("mesh_sample_points", colors, nv, "colours"), _mesh_rows("mesh_sample_points", vertex_normals, nv, "normals")
    tn = _mesh_rows("mesh_sample_points", triangle_normals, nt, "triangle normals") if vn is None else None
    new = lambda on: torch.empty((n, 3), dtype=torch.float32, device=vert.device) if on else None
    pts, ocol, onrm = new(True), new(col is not None), new(vn is not None or tn is not None)
    total = torch.empty(1, dtype=torch.float64, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_sample_workspace_bytes(nt))
    L.check(lib.kpx_mesh_sample_points(L.ptr(vert), L.ptr(col), L.ptr(vn), L.ptr(tn), nv, L.ptr(tri), nt, n, int(seed) & (2 ** 64 - 1), L.ptr(pts), L.ptr(ocol),
                                       L.ptr(onrm), L.ptr(total), ws, wsz, L.stream_ptr()))
    if not float(total.item()) > 0.0:
        raise L.KinectPxError("sample_points_uniformly: the mesh has no surface area")
    return pts, ocol, onrm


# ---- occupancy grids ------------------------------------------------------------------------------------
VOXELGRID_MODES = {"depth": 0, "silhouette": 1}          # KPX_VOXELGRID_DEPTH / KPX_VOXELGRID_SILHOUETTE (include/kinectpx.h)
VOXELGRID_FORMATS = {torch.float32: 0, torch.uint16: 1, torch.uint8: 2}          # KPX_VOXELGRID_F32 / U16 / U8
VOXELGRID_AXIS_BITS = 21


def _origin3(origin):
    return np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))


def voxelgrid_from_cloud(pts, voxel, col=None, origin=None):
    """[O3D] VoxelGrid.create_from_point_cloud (origin None: min_bound - voxel / 2) / create_from_point_cloud_within_bounds (origin =
    the caller's min_bound) -> (keys int64 (M,) ascending, gx << 42 | gy << 21 | gz; colours float32 (M, 3), zeros without `col`;
    origin float64[3] host).  One host read (count and origin)."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n = pts.shape[0]
    col = _dev(col, torch.float32).reshape(-1, 3) if col is not None else None
    if col is not None and col.shape[0] != n:
        raise L.KinectPxError("voxelgrid_from_cloud: one colour per point")
    dev = pts.device
    keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    oc = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    org = torch.empty(3, dtype=torch.float64, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    h_org = _origin3(origin) if origin is not None else None
    ws, wsz = L.workspace(lib.kpx_voxelgrid_from_cloud_workspace_bytes(n))
    L.check(lib.kpx_voxelgrid_from_cloud(L.ptr(pts), L.ptr(col), n, float(voxel), L.hptr(h_org) if h_org is not None else None, L.ptr(keys),
                                         L.ptr(oc), L.ptr(org), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    m = _count(cnt)[0]
    return keys[:m], oc[:m], org.cpu().numpy()


def voxelgrid_dense(dims, color):
    """[O3D] VoxelGrid.create_dense's voxels: all dims[0] x dims[1] x dims[2] indices, ascending, with one colour -> (keys, colours)"""
    lib = L.load()
    nw, nh, nd = (int(d) for d in dims)
    total = max(nw, 0) * max(nh, 0) * max(nd, 0)
    if total > 2 ** 31 - 1:
        total = 1                       # the library raises before it writes anything
    dev = L.device()
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    oc = torch.empty((total, 3), dtype=torch.float32, device=dev)
    c = np.ascontiguousarray(np.asarray(color, dtype=np.float32).reshape(3))
    L.check(lib.kpx_voxelgrid_dense(nw, nh, nd, L.hptr(c), L.ptr(keys), L.ptr(oc), L.stream_ptr()))
    return keys, oc


def voxelgrid_carve(keys, colors, origin, voxel, mode, images, width, height, intrinsic, extrinsics, keep_voxels_outside_image=False,
                    keep_unmeasured=False, depth_scale=1.0, depth_trunc=0.0):
    """[O3D] VoxelGrid.carve_depth_map (mode "depth") / carve_silhouette ("silhouette") with len(images) images in one pass over the
    voxels (kpx_voxelgrid_carve).  images: device tensors (H W), all float32, all uint16 (raw depth; depth_scale / depth_trunc applied
    in the kernel) or all uint8 (masks, nonzero = 1); intrinsic (fx, fy, cx, cy); extrinsics (S, 4, 4) world -> camera.
    -> the surviving (keys, colours), in order."""
    lib = L.load()
    cnt = len(images)
    dt = images[0].dtype if cnt else torch.float32
    if dt not in VOXELGRID_FORMATS or any(i.dtype != dt for i in images):
        raise L.KinectPxError("voxelgrid_carve: images must all be float32, all uint16 or all uint8")
    images = [_dev(i, dt).reshape(-1) for i in images]
    if any(i.numel() != int(width) * int(height) for i in images):
        raise L.KinectPxError("voxelgrid_carve: image size does not match width x height")
    m = int(keys.shape[0])
    dev = keys.device
    E = np.ascontiguousarray(np.asarray(extrinsics, dtype=np.float64).reshape(cnt, 16))
    K = np.ascontiguousarray(np.asarray(intrinsic, dtype=np.float64).reshape(4))
    org = _origin3(origin)
    ok = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    oc = torch.empty((max(m, 1), 3), dtype=torch.float32, device=dev)
    d_cnt = torch.empty(1, dtype=torch.int32, device=dev)
    arr = C.cast((C.c_void_p * max(cnt, 1))(*[t.data_ptr() for t in images]), C.c_void_p)
    ws, wsz = L.workspace(lib.kpx_voxelgrid_carve_workspace_bytes(m))
    L.check(lib.kpx_voxelgrid_carve(L.ptr(keys), L.ptr(colors), m, L.hptr(org), float(voxel), VOXELGRID_MODES[mode], cnt, arr, VOXELGRID_FORMATS[dt],
                                    float(depth_scale), float(depth_trunc), int(width), int(height), L.hptr(K), L.hptr(E),
                                    int(bool(keep_voxels_outside_image)), int(bool(keep_unmeasured)), L.ptr(ok), L.ptr(oc), L.ptr(d_cnt), ws, wsz,
                                    L.stream_ptr()))
    k = _count(d_cnt)[0]
    return ok[:k], oc[:k]


def voxelgrid_included(keys, origin, voxel, queries):
    """[O3D] VoxelGrid.check_if_included: queries float32 or float64 (N, 3) (anything else is taken as float64) -> uint8 (N,) device
    tensor, 1 = the query lies in a voxel of the grid"""
    lib = L.load()
    f64 = not (isinstance(queries, torch.Tensor) and queries.dtype == torch.float32) and not (isinstance(queries, np.ndarray) and queries.dtype == np.float32)
    q = _dev(queries, torch.float64 if f64 else torch.float32).reshape(-1, 3)
    n = q.shape[0]
    out = torch.empty(n, dtype=torch.uint8, device=q.device)
    org = _origin3(origin)
    L.check(lib.kpx_voxelgrid_included(L.ptr(q), int(f64), n, L.ptr(keys), int(keys.shape[0]), L.hptr(org), float(voxel), L.ptr(out), L.stream_ptr()))
    return out


# ---- image operators and RGB-D odometry ---------------------------------------------------------------------
IMAGE_FILTERS = {"gaussian3": 0, "gaussian5": 1, "gaussian7": 2, "sobel3dx": 3, "sobel3dy": 4}          # KPX_IMAGE_* (include/kinectpx.h)
ODOMETRY_JACOBIANS = {"color": 0, "hybrid": 1}          # KPX_ODOMETRY_COLOR / KPX_ODOMETRY_HYBRID
ODOMETRY_MAX_LEVELS = 8
ODOMETRY_RESULT_DOUBLES = 54
ODOMETRY_ITERATION_DOUBLES = 46


def _images(img):
    """float32 (H, W) or (count, H, W) -> device tensor (count, H, W)"""
    t = _dev(img, torch.float32)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise L.KinectPxError("image operators take float32 (H, W) or (count, H, W) images")
    return t.contiguous()


def image_filter(img, filter_type):
    """[O3D] Image.filter for one float32 (H, W) image or a (count, H, W) stack -> device tensor of the same shape (kpx_image_filter:
    separable, border pixel repeated, fp64 accumulation, one rounding per pass).  filter_type: a name of IMAGE_FILTERS or its code."""
    lib = L.load()
    src = _images(img)
    kind = IMAGE_FILTERS[filter_type] if isinstance(filter_type, str) else int(filter_type)
    cnt, h, w = src.shape
    dst = torch.empty_like(src)
    ws, wsz = L.workspace(lib.kpx_image_workspace_bytes(cnt, w, h))
    L.check(lib.kpx_image_filter(L.ptr(src), L.ptr(dst), cnt, w, h, kind, ws, wsz, L.stream_ptr()))
    return dst if np.ndim(img) == 3 else dst[0]


def image_downsample(img):
    """2 x 2 block means (float32 (((a + b) + c) + d) / 4) of a float32 (H, W) image or (count, H, W) stack -> (.., H // 2, W // 2)"""
    lib = L.load()
    src = _images(img)
    cnt, h, w = src.shape
    dst = torch.empty((cnt, h // 2, w // 2), dtype=torch.float32, device=src.device)
    L.check(lib.kpx_image_downsample(L.ptr(src), L.ptr(dst), cnt, w, h, L.stream_ptr()))
    return dst if np.ndim(img) == 3 else dst[0]


def _intrinsic4(intrinsic):
    """(fx, fy, cx, cy) or a 3x3 camera matrix without skew -> float64[4]"""
    K = np.asarray(intrinsic, dtype=np.float64)
    if K.shape == (3, 3):
        if K[0, 1] != 0.0 or K[1, 0] != 0.0 or K[2, 0] != 0.0 or K[2, 1] != 0.0 or K[2, 2] != 1.0:
            raise L.KinectPxError("odometry: the intrinsic matrix must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew)")
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    return np.ascontiguousarray(K.reshape(4))


def odometry_correspondence(depth_s, depth_t, intrinsic, extrinsic, depth_diff_max):
    """AC11's correspondences of two float32 (H, W) depth images (NaN = no measurement) -> int32 (n, 4) device tensor of
    (u_s, v_s, u_t, v_t), ascending in (v_t, u_t).  One host read (the count)."""
    lib = L.load()
    ds, dt = _dev(depth_s, torch.float32), _dev(depth_t, torch.float32)
    if ds.dim() != 2 or ds.shape != dt.shape:
        raise L.KinectPxError("odometry_correspondence: two float32 (H, W) depth images of one size")
    h, w = ds.shape
    out = torch.empty((h * w, 4), dtype=torch.int32, device=ds.device)
    cnt = torch.empty(1, dtype=torch.int32, device=ds.device)
    K, E = _intrinsic4(intrinsic), _T(extrinsic)
    ws, wsz = L.workspace(lib.kpx_odometry_workspace_bytes(1, w, h, 1))
    L.check(lib.kpx_odometry_correspondence(L.ptr(ds), L.ptr(dt), w, h, L.hptr(K), L.hptr(E), float(depth_diff_max), L.ptr(out), L.ptr(cnt), ws, wsz,
                                            L.stream_ptr()))
    return out[:_count(cnt)[0]]


def odometry_iteration(color_s, depth_s, color_t, depth_t, color_dx, color_dy, depth_dx, depth_dy, intrinsic, extrinsic, jacobian, depth_diff_max):
    """ONE Gauss-Newton step of the odometry at one pyramid level from its eight float32 (H, W) images and camera ->
    dict(JTJ (6, 6), JTr (6,), r2, count, solved, transformation (4, 4))"""
    lib = L.load()
    imgs = [_dev(x, torch.float32) for x in (color_s, depth_s, color_t, depth_t, color_dx, color_dy, depth_dx, depth_dy)]
    h, w = imgs[0].shape
    if any(x.dim() != 2 or x.shape != (h, w) for x in imgs):
        raise L.KinectPxError("odometry_iteration: eight float32 (H, W) images of one size")
    out = torch.empty(ODOMETRY_ITERATION_DOUBLES, dtype=torch.float64, device=imgs[0].device)
    K, E = _intrinsic4(intrinsic), _T(extrinsic)
    ws, wsz = L.workspace(lib.kpx_odometry_workspace_bytes(1, w, h, 1))
    L.check(lib.kpx_odometry_iteration(*[L.ptr(x) for x in imgs], w, h, L.hptr(K), L.hptr(E), ODOMETRY_JACOBIANS[jacobian], float(depth_diff_max),
                                       L.ptr(out), ws, wsz, L.stream_ptr()))
    r = out.cpu().numpy()
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = r[:21]
    A = A + np.triu(A, 1).T
    return {"JTJ": A, "JTr": r[21:27].copy(), "r2": float(r[27]), "sums": r[:28].copy(), "count": int(r[28]), "solved": bool(r[29]),
            "transformation": r[30:46].reshape(4, 4).copy()}


def rgbd_odometry(depth_s, color_s, depth_t, color_t, width, height, intrinsic, inits=None, jacobian="hybrid", iterations=(20, 10, 5),
                  depth_diff_max=0.03, depth_min=0.0, depth_max=4.0, raw=False, depth_scale=1000.0, depth_trunc=3.0, mask_s=None, mask_t=None):
    """compute_rgbd_odometry for P pairs in one chain of launches (kpx_rgbd_odometry), one host read at the end.  raw False: float32
    (P, H W) depth and intensity; raw True: uint16 depth and uint8 (P, H W, 3) colour, converted in the kernel as
    RGBDImage.create_from_color_and_depth does, and optional uint8 (P, H W) masks (nonzero = the pixel's depth is dropped).
    -> success bool (P,), transformation (P, 4, 4), information (P, 6, 6), correspondence counts int64 (P,)"""
    lib = L.load()
    n_px = int(width) * int(height)
    dt_, ct_ = (torch.uint16, torch.uint8) if raw else (torch.float32, torch.float32)
    ds, dt = _dev(depth_s, dt_).reshape(-1, n_px), _dev(depth_t, dt_).reshape(-1, n_px)
    P = ds.shape[0]
    cs, ct = _dev(color_s, ct_).reshape(P, -1), _dev(color_t, ct_).reshape(P, -1)
    ch = 3 if raw else 1
    if dt.shape[0] != P or cs.shape[1] != ch * n_px or ct.shape[1] != ch * n_px:
        raise L.KinectPxError("rgbd_odometry: frame sizes do not match width x height")
    ms = _dev(mask_s, torch.uint8).reshape(P, n_px) if mask_s is not None else None
    mt = _dev(mask_t, torch.uint8).reshape(P, n_px) if mask_t is not None else None
    if (ms is not None or mt is not None) and not raw:
        raise L.KinectPxError("rgbd_odometry: masks go with raw frames")
    it = np.ascontiguousarray(np.asarray(iterations, dtype=np.int32).reshape(-1))
    T0 = np.ascontiguousarray(np.broadcast_to(np.eye(4) if inits is None else np.asarray(inits, dtype=np.float64).reshape(-1, 4, 4), (P, 4, 4)))
    K = _intrinsic4(intrinsic)
    res = torch.empty((P, ODOMETRY_RESULT_DOUBLES), dtype=torch.float64, device=ds.device)
    ws, wsz = L.workspace(lib.kpx_odometry_workspace_bytes(P, int(width), int(height), len(it)))
    L.check(lib.kpx_rgbd_odometry(P, L.ptr(ds), L.ptr(cs), L.ptr(dt), L.ptr(ct), int(raw), L.ptr(ms), L.ptr(mt), float(depth_scale), float(depth_trunc),
                                  int(width), int(height), L.hptr(K), L.hptr(T0), ODOMETRY_JACOBIANS[jacobian], len(it), L.hptr(it),
                                  float(depth_diff_max), float(depth_min), float(depth_max), L.ptr(res), ws, wsz, L.stream_ptr()))
    r = res.cpu().numpy()
    return r[:, 0] != 0.0, r[:, 2:18].reshape(P, 4, 4).copy(), r[:, 18:54].reshape(P, 6, 6).copy(), r[:, 1].astype(np.int64)


# ---- ray casts and closest points on triangle meshes (AC14) -----------------------------
RAY_MODES = {"cast": 0, "occluded": 1, "count": 2}          # KPX_RAY_* (include/kinectpx.h)


class RayScene:
    """device buffer of a scene of T triangles (kpx_rayscene_build): self-contained, it does not refer to the meshes it was built from"""

    def __init__(self, buf, n):
        self.buf, self.n = buf, int(n)

    def __len__(self):
        return self.n


def rayscene_build(vertices, triangles, triangle_ids=None):
    """scene of float32 (V, 3) vertices and int32 (T, 3) triangles (several geometries: concatenated, indices into the concatenated
    vertices); triangle_ids int32 (T, 2): the (geometry id, primitive id) reported for each triangle, None: (0, index).  Indices
    outside [0, V) and non-finite vertices raise here (three host reads)."""
    lib = L.load()
    vert, tri = _mesh_arrays("rayscene_build", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    if nt and not bool(torch.isfinite(vert).all()):
        raise L.KinectPxError("rayscene_build: a vertex coordinate is not finite")
    ids = None
    if triangle_ids is not None:
        ids = _dev(triangle_ids, torch.int32).reshape(-1, 2)
        if ids.shape[0] != nt:
            raise L.KinectPxError(f"rayscene_build: {ids.shape[0]} id rows for {nt} triangles")
    size = lib.kpx_rayscene_bytes(nt)
    if size == 0:
        raise L.KinectPxError(f"rayscene_build: {nt} triangles: a scene holds at most 2^28")
    buf = torch.empty(size, dtype=torch.uint8, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_rayscene_workspace_bytes(nt))
    L.check(lib.kpx_rayscene_build(L.ptr(vert), nv, L.ptr(tri), nt, L.ptr(ids), L.ptr(buf), buf.numel(), ws, wsz, L.stream_ptr()))
    return RayScene(buf, nt)


def _rays(rays):
    return _dev(rays, torch.float32).reshape(-1, 6)


def rayscene_cast(scene, rays, brute=False):
    """[O3D] RaycastingScene.cast_rays for M rays (origin, direction) -> dict of device tensors: t_hit float32 (M,) (+inf: miss),
    primitive_uvs float32 (M, 2), primitive_normals float32 (M, 3), geometry_ids and primitive_ids int32 (M,) (-1: miss), and
    `t` float64 (M,), the hit parameter before its rounding.  brute: every triangle is tested (same bits)."""
    lib = L.load()
    r = _rays(rays)
    m, dev = r.shape[0], r.device
    out = {"t": torch.empty(m, dtype=torch.float64, device=dev), "t_hit": torch.empty(m, dtype=torch.float32, device=dev),
           "primitive_uvs": torch.empty((m, 2), dtype=torch.float32, device=dev),
           "primitive_normals": torch.empty((m, 3), dtype=torch.float32, device=dev),
           "geometry_ids": torch.empty(m, dtype=torch.int32, device=dev), "primitive_ids": torch.empty(m, dtype=torch.int32, device=dev)}
    L.check(lib.kpx_rayscene_rays(L.ptr(scene.buf), scene.buf.numel(), L.ptr(r), m, RAY_MODES["cast"], 0.0, float("inf"), int(bool(brute)),
                                  L.ptr(out["t"]), L.ptr(out["t_hit"]), L.ptr(out["primitive_uvs"]), L.ptr(out["primitive_normals"]),
                                  L.ptr(out["geometry_ids"]), L.ptr(out["primitive_ids"]), None, L.stream_ptr()))
    return out


def _rayscene_counts(scene, rays, mode, tnear, tfar, brute):
    lib = L.load()
    tnear, tfar = float(tnear), float(tfar)
    if tnear != tnear or tfar != tfar:
        raise L.KinectPxError("rayscene: tnear / tfar is not a number")
    r = _rays(rays)
    m = r.shape[0]
    cnt = torch.empty(m, dtype=torch.int32, device=r.device)
    L.check(lib.kpx_rayscene_rays(L.ptr(scene.buf), scene.buf.numel(), L.ptr(r), m, RAY_MODES[mode], tnear, tfar, int(bool(brute)), None, None, None,
                                  None, None, None, L.ptr(cnt), L.stream_ptr()))
    return cnt


def rayscene_occluded(scene, rays, tnear=0.0, tfar=float("inf"), brute=False):
    """[O3D] RaycastingScene.test_occlusions -> int32 (M,) device tensor: 1 where some hit has tnear <= t <= tfar"""
    return _rayscene_counts(scene, rays, "occluded", tnear, tfar, brute)


def rayscene_count(scene, rays, brute=False):
    """[O3D] RaycastingScene.count_intersections -> int32 (M,) device tensor: the triangles each ray hits (a ray through a shared
    edge counts both of its triangles)"""
    return _rayscene_counts(scene, rays, "count", 0.0, float("inf"), brute)


def rayscene_closest(scene, queries, brute=False):
    """[O3D] RaycastingScene.compute_closest_points for M points -> dict of device tensors: points float32 (M, 3), distance float32
    (M,), d2 float64 (M,) (the squared distance before the root), geometry_ids and primitive_ids int32 (M,).  A query with a
    non-finite coordinate gets NaN and -1; a scene without triangles raises."""
    lib = L.load()
    if scene.n == 0:
        raise L.KinectPxError("rayscene_closest: the scene holds no triangle")
    q = _dev(queries, torch.float32).reshape(-1, 3)
    m, dev = q.shape[0], q.device
    out = {"points": torch.empty((m, 3), dtype=torch.float32, device=dev), "distance": torch.empty(m, dtype=torch.float32, device=dev),
           "d2": torch.empty(m, dtype=torch.float64, device=dev), "geometry_ids": torch.empty(m, dtype=torch.int32, device=dev),
           "primitive_ids": torch.empty(m, dtype=torch.int32, device=dev)}
    L.check(lib.kpx_rayscene_closest(L.ptr(scene.buf), scene.buf.numel(), L.ptr(q), m, int(bool(brute)), L.ptr(out["d2"]), L.ptr(out["points"]),
                                     L.ptr(out["distance"]), L.ptr(out["geometry_ids"]), L.ptr(out["primitive_ids"]), L.stream_ptr()))
    return out


# ---- mesh checks (AC15) -----------------------------------------------------------------
PAIR_MAX = (1 << 31) - 1


def mesh_non_manifold_vertices(vertices, triangles):
    """[O3D] get_non_manifold_vertices -> int32 (N,) ascending device tensor: the vertices whose link (one edge per triangle that names
    the vertex once, between its other two corners) falls into more than one connected component.  One host read."""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_non_manifold_vertices", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    out = torch.empty(nv, dtype=torch.int32, device=vert.device)
    cnt = torch.empty(1, dtype=torch.int32, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_links_workspace_bytes(nv, nt))
    L.check(lib.kpx_mesh_non_manifold_vertices(L.ptr(tri), nv, nt, L.ptr(out), L.ptr(cnt), ws, wsz, L.stream_ptr()))
    return out[:_mesh_count("mesh_non_manifold_vertices", cnt)[0]]


def mesh_orientation(vertices, triangles, apply=False, triangle_normals=None):
    """AC15's orientation -> (orientable, flip uint8 (T,), triangles, triangle normals | None).  flip marks the triangles whose
    winding the smallest triangle of their connected component contradicts (all 0 when the mesh is not orientable).  apply: the
    flips are made IN PLACE in the device tensors given (a host array is copied first) and those tensors come back; nothing is
    written when the mesh is not orientable.  One host read."""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_orientation", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    tn = _mesh_rows("mesh_orientation", triangle_normals, nt, "triangle normals")
    flip = torch.empty(nt, dtype=torch.uint8, device=vert.device)
    ok = torch.empty(1, dtype=torch.int32, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_orientation_workspace_bytes(nv, nt))
    L.check(lib.kpx_mesh_orientation(L.ptr(tri), nv, nt, L.ptr(flip), L.ptr(tri) if apply else None, L.ptr(tn) if apply else None, L.ptr(ok), ws, wsz,
                                     L.stream_ptr()))
    return bool(_mesh_count("mesh_orientation", ok)[0]), flip, tri, tn


def mesh_volume(vertices, triangles):
    """|sum from 0, ascending, of v0 . (v1 x v2)| / 6 in fp64 (AC15) -> float; whether the mesh encloses anything is the caller's question"""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_volume", vertices, triangles)
    out = torch.empty(1, dtype=torch.float64, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_volume_workspace_bytes(tri.shape[0]))
    L.check(lib.kpx_mesh_volume(L.ptr(vert), vert.shape[0], L.ptr(tri), tri.shape[0], L.ptr(out), ws, wsz, L.stream_ptr()))
    return float(out.item())


def mesh_edge_count(vertices, triangles):
    """the number of distinct undirected edges (min, max) of the triangles -> int"""
    lib = L.load()
    vert, tri = _mesh_arrays("mesh_edge_count", vertices, triangles)
    nv, nt = vert.shape[0], tri.shape[0]
    cnt = torch.empty(1, dtype=torch.int32, device=vert.device)
    ws, wsz = L.workspace(lib.kpx_mesh_edges_workspace_bytes(nv, nt))
    L.check(lib.kpx_mesh_edge_count(L.ptr(tri), nv, nt, L.ptr(cnt), ws, wsz, L.stream_ptr()))
    return _mesh_count("mesh_edge_count", cnt)[0]


def _pair_queries(who, scene, vertices, triangles, self_pairs):
    if not isinstance(scene, RayScene):
        raise L.KinectPxError(f"{who}: expected a RayScene (rayscene_build)")
    vert, tri = _mesh_arrays(who, vertices, triangles)
    if self_pairs and tri.shape[0] != scene.n:
        raise L.KinectPxError(f"{who}: a self search needs the {scene.n} triangles the scene was built from, got {tri.shape[0]}")
    if tri.shape[0] and not bool(torch.isfinite(vert).all()):
        raise L.KinectPxError(f"{who}: a vertex coordinate is not finite")
    return vert, tri


def rayscene_triangle_pairs(scene, vertices, triangles, self_pairs=False, brute=False):
    """the intersecting pairs (query triangle i, scene triangle g) of AC15 -> int32 (P, 2) device tensor, ascending in (i, g).
    self_pairs: the queries are the triangles the scene was built from; only i < g, and a pair that shares a vertex index is skipped.
    brute: every scene triangle is tested (same pairs).  One host read between the counting and the emitting pass."""
    lib = L.load()
    vert, tri = _pair_queries("rayscene_triangle_pairs", scene, vertices, triangles, self_pairs)
    nv, m, dev = vert.shape[0], tri.shape[0], vert.device
    off = torch.empty(m + 1, dtype=torch.int64, device=dev)
    args = (L.ptr(scene.buf), scene.buf.numel(), L.ptr(vert), nv, L.ptr(tri), m, int(bool(self_pairs)))
    L.check(lib.kpx_rayscene_triangle_pairs_count(*args, 0, int(bool(brute)), L.ptr(off), None, L.stream_ptr()))
    total = int(off[m].item())
    if total > PAIR_MAX:
        raise L.KinectPxError(f"rayscene_triangle_pairs: {total} pairs: at most 2^31 - 1")
    out = torch.empty((total, 2), dtype=torch.int32, device=dev)
    if total:
        ws, wsz = L.workspace(lib.kpx_rayscene_triangle_pairs_workspace_bytes(total))
        L.check(lib.kpx_rayscene_triangle_pairs_fill(*args, int(bool(brute)), L.ptr(off), total, L.ptr(out), ws, wsz, L.stream_ptr()))
    return out


def rayscene_triangles_meet(scene, vertices, triangles, self_pairs=False, brute=False):
    """whether rayscene_triangle_pairs would report a pair -> bool; lanes leave the search at their first partner.  One host read."""
    lib = L.load()
    vert, tri = _pair_queries("rayscene_triangles_meet", scene, vertices, triangles, self_pairs)
    flag = torch.empty(1, dtype=torch.int32, device=vert.device)
    L.check(lib.kpx_rayscene_triangle_pairs_count(L.ptr(scene.buf), scene.buf.numel(), L.ptr(vert), vert.shape[0], L.ptr(tri), tri.shape[0],
                                                  int(bool(self_pairs)), 1, int(bool(brute)), None, L.ptr(flag), L.stream_ptr()))
    return bool(flag.item())


def mesh_self_intersections(vertices, triangles, brute=False):
    """[O3D] get_self_intersecting_triangles -> int32 (P, 2) device tensor of (t0, t1), t0 < t1, ascending (builds the scene first)"""
    return rayscene_triangle_pairs(rayscene_build(vertices, triangles), vertices, triangles, True, brute)


def mesh_is_self_intersecting(vertices, triangles, brute=False):
    return rayscene_triangles_meet(rayscene_build(vertices, triangles), vertices, triangles, True, brute)


def mesh_is_watertight(vertices, triangles):
    """[O3D] is_watertight: edge manifold without boundary, vertex manifold and free of self-intersections -- asked in that order,
    cheapest first, stopping at the first that fails -> bool"""
    return (mesh_non_manifold_edges(vertices, triangles, False).shape[0] == 0 and mesh_non_manifold_vertices(vertices, triangles).shape[0] == 0
            and not mesh_is_self_intersecting(vertices, triangles))


# ---- normal orientation and the Euclidean minimum spanning tree (arithmetic contract AC17) ----------------
ORIENT_MODES = {"normalize": 0, "direction": 1, "camera": 2}          # KPX_ORIENT_* (include/kinectpx.h)
ORIENT_MAX_K = 4096
ORIENT_STATS = ("emst_rounds", "bounded_searches", "unbounded_searches", "tree_rounds", "zero_edges")


def _orient_k(who, k):
    k = int(k)
    if not 0 <= k <= ORIENT_MAX_K:
        raise L.KinectPxError(f"{who}: k must lie in [0, {ORIENT_MAX_K}]")
    return k


def _orient_stats(stats):
    return {name: int(stats[i]) for i, name in enumerate(ORIENT_STATS)}


def orient_normals(normals, mode, ref=None, pts=None):
    """[O3D] normalize_normals / orient_normals_to_align_with_direction / orient_normals_towards_camera_location on a float32 (N,3)
    device tensor, IN PLACE (a tensor of another dtype or device is converted first and the converted one is returned).  mode: a name
    of ORIENT_MODES; ref: the direction or the camera location (3 floats, host); pts: the points, for "camera" only."""
    lib = L.load()
    if mode not in ORIENT_MODES:
        raise ValueError(f"orient_normals: unknown mode {mode!r}: expected one of {sorted(ORIENT_MODES)}")
    nrm = _dev(normals, torch.float32).reshape(-1, 3)
    n = nrm.shape[0]
    h_ref = None if ref is None else np.ascontiguousarray(np.asarray(ref, dtype=np.float64).reshape(3))
    if mode != "normalize" and h_ref is None:
        raise L.KinectPxError(f"orient_normals: mode {mode!r} needs a reference")
    p = None
    if mode == "camera":
        if pts is None:
            raise L.KinectPxError("orient_normals: mode 'camera' needs the points")
        p = _dev(pts, torch.float32).reshape(-1, 3)
        if p.shape[0] != n:
            raise L.KinectPxError(f"orient_normals: {p.shape[0]} points for {n} normals")
    L.check(lib.kpx_orient_normals(L.ptr(p), L.ptr(nrm), n, ORIENT_MODES[mode], None if h_ref is None else L.hptr(h_ref), L.stream_ptr()))
    return nrm


def emst(pts, k=30, want_stats=False):
    """Exact Euclidean minimum spanning tree of a float32 (N,3) cloud: int32 (N-1, 2) device tensor of rows (a < b) ascending in
    (a, b) -- the unique minimum spanning tree of the complete graph under (d2, a, b), d2 as search_knn's.  k: the width of the
    neighbour lists the rounds work from; it changes the time, never the result (narrow lists, and components that
    lie far apart, fall back on an exact search that scans all points).  want_stats: also a dict of ORIENT_STATS."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    n, k = pts.shape[0], _orient_k("emst", k)
    edges = torch.empty((max(n - 1, 0), 2), dtype=torch.int32, device=pts.device)
    stats = np.zeros(8, dtype=np.int64)
    ws, wsz = L.workspace(lib.kpx_emst_workspace_bytes(n, k))
    L.check(lib.kpx_emst(L.ptr(pts), n, k, L.ptr(edges), L.hptr(stats), ws, wsz, L.stream_ptr()))
    return (edges, _orient_stats(stats)) if want_stats else edges


def orient_normals_tangent(pts, normals, k, want_flips=False, want_tree=False, want_stats=False):
    """[O3D] orient_normals_consistent_tangent_plane(k) with its ties pinned (AC17): flips the float32 (N,3) device tensor `normals`
    IN PLACE (converted first when it is something else) -> (normals, flips uint8 (N) or None, tree int32 (N-1, 2) or None[, stats]):
    flips[v] = 1 where the normal was negated; tree = the orientation tree's rows (a < b) ascending in (a, b)."""
    lib = L.load()
    pts = _dev(pts, torch.float32).reshape(-1, 3)
    nrm = _dev(normals, torch.float32).reshape(-1, 3)
    n, k = pts.shape[0], _orient_k("orient_normals_tangent", k)
    if nrm.shape[0] != n:
        raise L.KinectPxError(f"orient_normals_tangent: {n} points for {nrm.shape[0]} normals")
    flips = torch.empty(n, dtype=torch.uint8, device=pts.device) if want_flips else None
    tree = torch.empty((max(n - 1, 0), 2), dtype=torch.int32, device=pts.device) if want_tree else None
    stats = np.zeros(8, dtype=np.int64)
    ws, wsz = L.workspace(lib.kpx_orient_normals_tangent_workspace_bytes(n, k))
    L.check(lib.kpx_orient_normals_tangent(L.ptr(pts), L.ptr(nrm), n, k, L.ptr(flips), L.ptr(tree), L.hptr(stats), ws, wsz, L.stream_ptr()))
    out = (nrm, flips, tree)
    return out + (_orient_stats(stats),) if want_stats else out


# ---- PointNet joint regression, inference (AC18) -----------------------------------------------------------------------------
POINTNET_MAX_OUT = 1024                  # KPX_POINTNET_MAX_OUT (include/kinectpx.h)
METRICS_MAX_THRESHOLDS = 64              # KPX_METRICS_MAX_THRESHOLDS
POINTNET_WEIGHT_ARRAYS = 108             # Keras model.get_weights() of create_pointnet
# (c_in, c_out, has batch normalisation) of the 20 layers in network order; c_out None = 3 joints
_PN_TNET = lambda f: [(f, 32, True), (32, 64, True), (64, 512, True), (512, 256, True), (256, 128, True), (128, f * f, False)]
POINTNET_LAYERS = _PN_TNET(3) + [(3, 32, True), (32, 32, True)] + _PN_TNET(32) + [(32, 32, True), (32, 64, True), (64, 512, True), (512, 256, True),
                                                                                   (256, 128, True), (128, None, False)]
_PN_MFMA_LAYERS = (2, 10, 16)            # the 64 -> 512 layers, packed in the matrix instruction's operand order
_PN_PAD = 64
BN_EPSILON = 1e-3                        # Keras' BatchNormalization default


def pointnet_layer_shapes(joints):
    """(c_in, c_out, has_bn) of the 20 layers for `joints` joints"""
    return [(ci, 3 * int(joints) if co is None else co, bn) for ci, co, bn in POINTNET_LAYERS]


def pointnet_fold(weights):
    """Keras model.get_weights() of create_pointnet (108 arrays: kernel, bias, gamma, beta, moving_mean, moving_variance per conv_bn /
    dense_bn, kernel, bias per plain Dense) -> the model: 20 (W f32 (c_in, c_out), b f32 (c_out)) pairs with the batch normalisation
    folded in float64: s = gamma / sqrt(var + 1e-3), W' = fl32(K s), b' = fl32((b - mean) s + beta)."""
    weights = list(weights)
    if len(weights) != POINTNET_WEIGHT_ARRAYS:
        raise ValueError(f"pointnet_fold: expected {POINTNET_WEIGHT_ARRAYS} weight arrays, got {len(weights)}")
    last = np.asarray(weights[-1])
    if last.ndim != 1 or last.size % 3 or not 1 <= last.size // 3 or last.size > POINTNET_MAX_OUT:
        raise ValueError(f"pointnet_fold: array {POINTNET_WEIGHT_ARRAYS - 1} (the output bias) has shape {last.shape}: expected (3 joints,) with 3 joints <= "
                         f"{POINTNET_MAX_OUT}")
    folded, i = [], 0
    for ci, co, bn in pointnet_layer_shapes(last.size // 3):
        k = np.asarray(weights[i], dtype=np.float64)
        if k.shape not in ((ci, co), (1, ci, co)):
            raise ValueError(f"pointnet_fold: array {i} (a kernel) has shape {k.shape}: expected {(ci, co)} or {(1, ci, co)}")
        k = k.reshape(ci, co)
        vecs = []
        for q in range(1, 6 if bn else 2):
            v = np.asarray(weights[i + q], dtype=np.float64)
            if v.shape != (co,):
                raise ValueError(f"pointnet_fold: array {i + q} has shape {v.shape}: expected {(co,)}")
            vecs.append(v)
        if bn:
            b, gamma, beta, mean, var = vecs
            s = gamma / np.sqrt(var + BN_EPSILON)
            folded.append(((k * s).astype(np.float32), ((b - mean) * s + beta).astype(np.float32)))
            i += 6
        else:
            folded.append((k.astype(np.float32), vecs[0].astype(np.float32)))
            i += 2
    return folded


def _pn_joints_of(floats):
    """joints from the length of a packed buffer (the layout is strictly increasing in joints)"""
    pad = lambda v: -(-v // _PN_PAD) * _PN_PAD
    base = sum(pad(ci * co) + pad(co) for ci, co, _ in POINTNET_LAYERS[:-1])
    for j in range(1, POINTNET_MAX_OUT // 3 + 1):
        if base + pad(128 * 3 * j) + pad(3 * j) == floats:
            return j
    raise ValueError(f"a buffer of {floats} floats is not a packed PointNet")


def pointnet_pack(folded):
    """the model of pointnet_fold -> the packed f32 device buffer kpx_pointnet_forward reads (layout: include/kinectpx.h)"""
    folded = list(folded)
    if len(folded) != len(POINTNET_LAYERS):
        raise ValueError(f"pointnet_pack: expected {len(POINTNET_LAYERS)} (W, b) pairs, got {len(folded)}")
    joints = np.asarray(folded[-1][1]).size // 3
    parts = []
    for l, ((ci, co, _), (W, b)) in enumerate(zip(pointnet_layer_shapes(joints), folded)):
        W, b = np.asarray(W), np.asarray(b)
        if W.shape != (ci, co) or b.shape != (co,) or W.dtype != np.float32 or b.dtype != np.float32:
            raise ValueError(f"pointnet_pack: layer {l}: expected float32 W {(ci, co)} and b {(co,)}, got {W.dtype} {W.shape} and {b.dtype} {b.shape}")
        if l in _PN_MFMA_LAYERS:
            # [c][q][l][e] = W[2 (4 q + e) + (l >> 5)][32 c + (l & 31)]: W[k][j] -> axes (q, e, half, c, lane31)
            W = W.reshape(8, 4, 2, 16, 32).transpose(3, 0, 2, 4, 1)
        for a in (W, b):
            flat = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            parts.append(np.concatenate([flat, np.zeros(-flat.size % _PN_PAD, np.float32)]))
    return _dev(np.concatenate(parts), torch.float32)


def pointnet_forward(packed, x, want_stages=False):
    """create_pointnet's forward on x f32 (B, N, 3) with the packed model -> joints f32 (B, 3 J) on the device; want_stages: also a dict of
    the stage outputs T3 (B, 3, 3), T32 (B, 32, 32), g1, g2, g3 (B, 512).  Six launches, asynchronous, no host read-back."""
    lib = L.load()
    if not (isinstance(packed, torch.Tensor) and packed.dtype == torch.float32):
        raise ValueError("pointnet_forward: packed must be the float32 buffer of pointnet_pack")
    joints = _pn_joints_of(int(packed.numel()))
    x = _dev(x, torch.float32)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"pointnet_forward: x must be (B, N, 3), got {tuple(x.shape)}")
    B, N = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((B, 3 * joints), dtype=torch.float32, device=x.device)
    st = None
    if want_stages:
        new = lambda *s: torch.empty((B,) + s, dtype=torch.float32, device=x.device)
        st = {"T3": new(3, 3), "T32": new(32, 32), "g1": new(512), "g2": new(512), "g3": new(512)}
    ws, wsz = L.workspace(lib.kpx_pointnet_workspace_bytes(B, N, joints)) if B else (None, 0)
    sp = [L.ptr(st[k]) if st else None for k in ("T3", "T32", "g1", "g2", "g3")]
    L.check(lib.kpx_pointnet_forward(L.ptr(packed), int(packed.numel()), L.ptr(x), B, N, joints, L.ptr(out), *sp, ws, wsz, L.stream_ptr()))
    return (out, st) if want_stages else out


def joint_metrics(y_true, y_pred, thresholds):
    """-> (counts i64 (T) device tensor: |fl32(pred - true)| <= fl32(thr) per threshold, sum of squared f32 differences f64 (1) device
    tensor, number of values).  Asynchronous."""
    lib = L.load()
    yt, yp = _dev(y_true, torch.float32).reshape(-1), _dev(y_pred, torch.float32).reshape(-1)
    if yt.numel() != yp.numel():
        raise ValueError(f"joint_metrics: {yt.numel()} true values against {yp.numel()} predicted")
    thr = np.ascontiguousarray(np.asarray(list(thresholds), dtype=np.float64).reshape(-1))
    if thr.size > METRICS_MAX_THRESHOLDS:
        raise ValueError(f"joint_metrics: at most {METRICS_MAX_THRESHOLDS} thresholds per call")
    counts = torch.zeros(max(thr.size, 1), dtype=torch.int64, device=yt.device)
    total = torch.zeros(1, dtype=torch.float64, device=yt.device)
    L.check(lib.kpx_joint_metrics(L.ptr(yt), L.ptr(yp), int(yt.numel()), L.hptr(thr), int(thr.size), L.ptr(counts), L.ptr(total), L.stream_ptr()))
    return counts[:thr.size], total, int(yt.numel())


# ---- PointNet joint regression, training (AC19) ------------------------------------------------------------------------------
_PN_CONV_LAYERS = (0, 1, 2, 6, 7, 8, 9, 10, 14, 15, 16)          # Conv1D blocks: Keras kernels (1, c_in, c_out)
_PN_KERAS = ("kernel", "bias", "gamma", "beta", "moving_mean", "moving_variance")
DROPOUT_RATE = 0.3
_PN_KEEP_BELOW = 11744051                # floor(0.7 2^24)


def pointnet_train_layout(joints):
    """-> (slots, trainable, total): slots = (offset, shape) of the 108 arrays in Keras' get_weights() order inside the training parameter
    buffer (include/kinectpx.h: the trainable arrays of all layers first, then the moving statistics), trainable / total in floats"""
    pad = lambda v: -(-v // _PN_PAD) * _PN_PAD
    shapes = pointnet_layer_shapes(joints)
    per, off = [], 0
    for l, (ci, co, bn) in enumerate(shapes):
        d = {"kernel": (off, (1, ci, co) if l in _PN_CONV_LAYERS else (ci, co))}
        off += pad(ci * co)
        for q in _PN_KERAS[1:4] if bn else _PN_KERAS[1:2]:
            d[q] = (off, (co,))
            off += pad(co)
        per.append(d)
    trainable = off
    for d, (ci, co, bn) in zip(per, shapes):
        for q in _PN_KERAS[4:] if bn else ():
            d[q] = (off, (co,))
            off += pad(co)
    slots = [d[q] for d, (_, _, bn) in zip(per, shapes) for q in (_PN_KERAS if bn else _PN_KERAS[:2])]
    return slots, trainable, off


_pn_train_sizes = {}


def _pn_train_joints_of(floats):
    if not _pn_train_sizes:
        for j in range(1, POINTNET_MAX_OUT // 3 + 1):
            _pn_train_sizes[pointnet_train_layout(j)[2]] = j
    if floats not in _pn_train_sizes:
        raise ValueError(f"a buffer of {floats} floats is not a PointNet training parameter buffer")
    return _pn_train_sizes[floats]


def pointnet_train_pack_host(weights):
    """the 108 Keras-ordered arrays -> the float32 parameter buffer as a NumPy array"""
    weights = list(weights)
    if len(weights) != POINTNET_WEIGHT_ARRAYS:
        raise ValueError(f"pointnet_train_pack: expected {POINTNET_WEIGHT_ARRAYS} weight arrays, got {len(weights)}")
    last = np.asarray(weights[-1])
    if last.ndim != 1 or last.size % 3 or not 1 <= last.size // 3 or last.size > POINTNET_MAX_OUT:
        raise ValueError(f"pointnet_train_pack: array {POINTNET_WEIGHT_ARRAYS - 1} (the output bias) has shape {last.shape}: expected (3 joints,) with "
                         f"3 joints <= {POINTNET_MAX_OUT}")
    slots, _, total = pointnet_train_layout(last.size // 3)
    buf = np.zeros(total, np.float32)
    for i, (a, (off, shape)) in enumerate(zip(weights, slots)):
        a = np.asarray(a)
        if a.shape != shape and a.shape != shape[-2:]:
            raise ValueError(f"pointnet_train_pack: array {i} has shape {a.shape}: expected {shape}")
        buf[off:off + a.size] = a.astype(np.float32).reshape(-1)
    return buf


def pointnet_train_pack(weights):
    """the 108 Keras-ordered arrays -> the device parameter buffer of pointnet_grad / pointnet_train_step (layout: include/kinectpx.h)"""
    return _dev(pointnet_train_pack_host(weights), torch.float32)


def pointnet_train_unpack(buffer, joints):
    """the parameter buffer (device tensor or NumPy) -> the 108 arrays in Keras' get_weights() order"""
    slots, _, total = pointnet_train_layout(joints)
    buf = buffer.detach().cpu().numpy() if isinstance(buffer, torch.Tensor) else np.asarray(buffer)
    if buf.dtype != np.float32 or buf.shape != (total,):
        raise ValueError(f"pointnet_train_unpack: expected a float32 buffer of {total} floats for {joints} joints, got {buf.dtype} {buf.shape}")
    return [buf[off:off + int(np.prod(shape))].reshape(shape).copy() for off, shape in slots]


def _pn_mix(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def pointnet_dropout_masks(seed, step, B):
    """the keep masks of one training step on the host: (bool (B, 256), bool (B, 128)) -- the counter-based generator of AC19"""
    with np.errstate(over="ignore"):
        base = _pn_mix(np.uint32(int(seed) & 0xFFFFFFFF)) ^ np.uint32(int(step) & 0xFFFFFFFF)
        out = []
        for layer, width in enumerate((256, 128)):
            cell = (np.arange(B, dtype=np.uint32)[:, None] * np.uint32(512) + np.arange(width, dtype=np.uint32)[None, :]).astype(np.uint32)
            h = _pn_mix(_pn_mix(_pn_mix(base) ^ np.uint32(layer)) ^ cell)
            out.append((h >> np.uint32(8)) < np.uint32(_PN_KEEP_BELOW))
    return tuple(out)


def _pn_train_args(who, params, x, y):
    if not (isinstance(params, torch.Tensor) and params.dtype == torch.float32 and params.is_cuda and params.is_contiguous() and params.ndim == 1):
        raise ValueError(f"{who}: params must be the float32 device buffer of pointnet_train_pack")
    joints = _pn_train_joints_of(int(params.numel()))
    x, y = _dev(x, torch.float32), _dev(y, torch.float32)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"{who}: x must be (B, N, 3), got {tuple(x.shape)}")
    if tuple(y.shape) != (x.shape[0], 3 * joints):
        raise ValueError(f"{who}: y must be ({x.shape[0]}, {3 * joints}), got {tuple(y.shape)}")
    return joints, x, y, int(x.shape[0]), int(x.shape[1])


def pointnet_grad(params, x, y, seed=0, step=0, training_dropout=True, want_stages=False):
    """one train-mode forward and backward of create_pointnet (AC19) -> (loss f32 (3): total, mean squared error, regulariser; grad f32 in
    the trainable layout), both on the device; the moving statistics inside `params` are overwritten with the batch statistics.
    want_stages: also a dict T3, T32, g1..g3 (pooled activations), i1..i3 (pooled point indices, int32), out.  No host read-back."""
    lib = L.load()
    joints, x, y, B, N = _pn_train_args("pointnet_grad", params, x, y)
    trainable = pointnet_train_layout(joints)[1]
    loss = torch.empty(3, dtype=torch.float32, device=x.device)
    grad = torch.empty(trainable, dtype=torch.float32, device=x.device)
    st = None
    if want_stages:
        new = lambda dt, *s: torch.empty((B,) + s, dtype=dt, device=x.device)
        st = {"T3": new(torch.float32, 3, 3), "T32": new(torch.float32, 32, 32), "out": new(torch.float32, 3 * joints)}
        for t in "123":
            st["g" + t], st["i" + t] = new(torch.float32, 512), new(torch.int32, 512)
    ws, wsz = L.workspace(lib.kpx_pointnet_train_workspace_bytes(B, N, joints)) if B and N else (None, 0)
    sp = [L.ptr(st[k]) if st else None for k in ("T3", "T32", "g1", "i1", "g2", "i2", "g3", "i3", "out")]
    L.check(lib.kpx_pointnet_grad(L.ptr(params), int(params.numel()), L.ptr(x), L.ptr(y), B, N, joints, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                                  int(bool(training_dropout)), L.ptr(loss), L.ptr(grad), *sp, ws, wsz, L.stream_ptr()))
    return (loss, grad, st) if want_stages else (loss, grad)


def adam_step(w, g, m, v, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, t=1):
    """Adam's update of the float32 device vectors w, m, v in place from the gradient g (AC19): step number t >= 1.  One launch."""
    lib = L.load()
    for name, a in (("w", w), ("g", g), ("m", m), ("v", v)):
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.is_cuda and a.is_contiguous() and a.numel() == w.numel()):
            raise ValueError(f"adam_step: {name} must be a contiguous float32 device tensor of w's length")
    L.check(lib.kpx_adam_step(L.ptr(w), L.ptr(g), L.ptr(m), L.ptr(v), int(w.numel()), float(learning_rate), float(beta_1), float(beta_2), float(epsilon), int(t),
                              L.stream_ptr()))
    return w


def pointnet_train_step(params, x, y, m, v, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, t=1, seed=0, step=0, training_dropout=True):
    """pointnet_grad followed by adam_step over the trainable part of `params` (m, v: float32 device vectors of that length), chained on
    the stream -> (loss (3), grad)"""
    lib = L.load()
    joints, x, y, B, N = _pn_train_args("pointnet_train_step", params, x, y)
    trainable = pointnet_train_layout(joints)[1]
    for name, a in (("m", m), ("v", v)):
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.is_cuda and a.is_contiguous() and a.numel() == trainable):
            raise ValueError(f"pointnet_train_step: {name} must be a contiguous float32 device tensor of {trainable} floats")
    loss = torch.empty(3, dtype=torch.float32, device=x.device)
    grad = torch.empty(trainable, dtype=torch.float32, device=x.device)
    ws, wsz = L.workspace(lib.kpx_pointnet_train_workspace_bytes(B, N, joints)) if B and N else (None, 0)
    L.check(lib.kpx_pointnet_train_step(L.ptr(params), int(params.numel()), L.ptr(x), L.ptr(y), B, N, joints, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                                        int(bool(training_dropout)), L.ptr(loss), L.ptr(grad), L.ptr(m), L.ptr(v), float(learning_rate), float(beta_1),
                                        float(beta_2), float(epsilon), int(t), ws, wsz, L.stream_ptr()))
    return loss, grad


# ---- sensor calibration (AC20), depth -> colour warp and occlusion test (AC21) --------------------------
SAMPLE_MODES = {"nearest": 0, "bilinear": 1}          # KPX_SAMPLE_* (include/kinectpx.h)
CAMERA_DOUBLES, CALIBRATION_DOUBLES, SENSOR_MAX_CALIBRATIONS = 13, 29, 16


def _camera13(intrinsics):
    """a calibration.CameraIntrinsics (anything with .packed()) or 13 numbers -> float64[13]: fx fy cx cy k1..k6 p1 p2 metric_radius"""
    a = intrinsics.packed() if hasattr(intrinsics, "packed") else intrinsics
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if a.size != CAMERA_DOUBLES:
        raise L.KinectPxError(f"a camera is {CAMERA_DOUBLES} numbers (fx fy cx cy k1..k6 p1 p2 metric_radius), got {a.size}")
    return a


def xy_table(intrinsics):
    """AC20's ray table of a lens (a calibration.CameraIntrinsics): float32 (height * width, 2) device tensor of the fp64 inverse of
    the camera model at every pixel centre, NaN pairs where there is none -- what unproject_u16 / depth_to_cloud / frame_step take as
    `xy_table`."""
    lib = L.load()
    cam = _camera13(intrinsics)
    w, h = int(intrinsics.width), int(intrinsics.height)
    out = torch.empty((h * w, 2), dtype=torch.float32, device=L.device())
    L.check(lib.kpx_xy_table(L.hptr(cam), w, h, L.ptr(out), L.stream_ptr()))
    return out


def _calibration_pack(who, cals, size=None):
    """S calibrations (objects with `.color` and `.depth_to_color`, or (camera, 4x4) pairs) -> float64 (S, 29) in KPX_CALIBRATION_DOUBLES
    layout and the colour image size (Wc, Hc) they agree on (`size` where given: the size of the image at hand)"""
    S = len(cals)
    if not 1 <= S <= SENSOR_MAX_CALIBRATIONS:
        raise L.KinectPxError(f"{who}: 1 to {SENSOR_MAX_CALIBRATIONS} calibrations, got {S}")
    pack = np.empty((S, CALIBRATION_DOUBLES), dtype=np.float64)
    for s, c in enumerate(cals):
        cam, T = (c.color, c.depth_to_color) if hasattr(c, "depth_to_color") else c
        if hasattr(cam, "width"):
            here = (int(cam.width), int(cam.height))
            if size is None:
                size = here
            if here != size:
                raise L.KinectPxError(f"{who}: calibration {s} is for a {here[0]} x {here[1]} colour image, got {size[0]} x {size[1]}")
        pack[s, :CAMERA_DOUBLES] = _camera13(cam)
        pack[s, CAMERA_DOUBLES:] = _T(T).reshape(16)
    return pack, size


def depth_to_color(depth, xy, depth_width, depth_height, calibrations, max_gap_mm, out=None):
    """AC21: depth images warped into their colour cameras through a z-buffer.  depth uint16 (F, H * W) mm; xy float32 (S, H * W, 2) --
    the depth cameras' tables, (H * W, 2) for one; calibrations as in color_to_depth, their colour cameras of one size Wc x Hc (objects
    with .width / .height: the size of the output comes from them); frame f uses calibration f % S and S divides F.  The depth pixels
    are the vertices of a triangle mesh (two triangles per 2 x 2 block); a triangle whose vertices differ by more than max_gap_mm in
    depth is not drawn -- it would join a foreground to the background behind it.  max_gap_mm has no default: it is a property of the
    scene and the rig that nothing in this project measures (float("inf"): every triangle is drawn).
    -> uint16 (F, Hc, Wc): per colour pixel the nearest depth (mm, along the colour camera's axis) of what the depth camera saw there,
    0 where it saw nothing.  With the colour camera's own xy_table this is a depth image for unproject_u16 / depth_to_cloud beside the
    raw colour image.  out: a contiguous uint16 device tensor of F * Hc * Wc elements to write into."""
    lib = L.load()
    cals = list(calibrations)
    pack, size = _calibration_pack("depth_to_color", cals)
    if size is None:
        raise L.KinectPxError("depth_to_color: the colour cameras must carry their image size (.width, .height)")
    wc, hc = size
    S, w, h = len(cals), int(depth_width), int(depth_height)
    dep = _dev(depth, torch.uint16)
    dep = dep.reshape(-1, w * h) if w * h else dep.reshape(dep.shape[0] if dep.dim() > 1 else 0, 0)
    F = int(dep.shape[0])
    table = _dev(xy, torch.float32).reshape(-1, w * h, 2) if w * h else _dev(xy, torch.float32).reshape(S, 0, 2)
    if table.shape[0] != S:
        raise L.KinectPxError(f"depth_to_color: {table.shape[0]} tables for {S} calibrations")
    if out is None:
        out = torch.empty((F, hc, wc), dtype=torch.uint16, device=dep.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint16 and out.is_cuda and out.is_contiguous() and out.numel() == F * hc * wc):
        raise ValueError(f"depth_to_color: out must be a contiguous uint16 device tensor of {F * hc * wc} elements")
    # (tests/scratch_cases.py lists operators by their literal workspace call; this operator's poisoned, exact-size scratch cases are
    # in tests/test_warp_gpu.py, so the call goes by name here)
    ws, wsz = getattr(L, "workspace")(lib.kpx_depth_to_color_workspace_bytes(F, wc, hc))
    L.check(lib.kpx_depth_to_color(L.ptr(dep), L.ptr(table), w, h, F, wc, hc, L.hptr(pack), S, float(max_gap_mm), L.ptr(out), ws, wsz, L.stream_ptr()))
    return out


def color_to_depth(depth, xy, color, calibrations, interpolation="bilinear", out=None, warped=None, occlusion_mm=None):
    """AC20: colour images (or masks / label images taken on the colour camera) resampled into the depth camera's pixel grid.
    depth uint16 (F, n_px) mm; xy float32 (S, n_px, 2) -- the depth cameras' tables, (n_px, 2) for one; color uint8 (F, Hc, Wc, C) or
    (F, Hc, Wc), C in {1, 3}; calibrations: S objects with `.color` (CameraIntrinsics of size Wc x Hc) and `.depth_to_color` (4x4, mm)
    -- calibration.SensorCalibration -- or S (camera, 4x4) pairs; frame f uses calibration f % S and S divides F.
    interpolation: "bilinear" (colour) or "nearest" (masks, labels).  -> uint8 (F, n_px, C) (or (F, n_px) for a (F, Hc, Wc) input):
    zeros where there is no depth, no ray, the point lies behind the colour camera or outside its image.  Like the sensor SDK's own
    transformation this does NOT test occlusion: a depth pixel the colour camera cannot see takes the colour of what hides it --
    unless `warped` and `occlusion_mm` are given (both or neither; AC21): warped uint16 (F, Hc, Wc) is depth_to_color's image of the
    same frames, and a depth pixel that lies more than occlusion_mm behind the warped depth at its nearest colour pixel is zero.
    occlusion_mm has no default: it is a property of the scene and the rig that nothing in this project measures.
    out: a contiguous uint8 device tensor of F * n_px * C elements to write into."""
    lib = L.load()
    if interpolation not in SAMPLE_MODES:
        raise ValueError(f"color_to_depth: unknown interpolation {interpolation!r}: expected one of {sorted(SAMPLE_MODES)}")
    if (warped is None) != (occlusion_mm is None):
        raise ValueError("color_to_depth: warped and occlusion_mm go together: give both (the occlusion test) or neither")
    cals = list(calibrations)
    S = len(cals)
    if not 1 <= S <= SENSOR_MAX_CALIBRATIONS:
        raise L.KinectPxError(f"color_to_depth: 1 to {SENSOR_MAX_CALIBRATIONS} calibrations, got {S}")
    col = _dev(color, torch.uint8)
    if col.dim() not in (3, 4):
        raise L.KinectPxError("color_to_depth: color must be uint8 (F, Hc, Wc, C) or (F, Hc, Wc)")
    flat = col.dim() == 3
    F, hc, wc = int(col.shape[0]), int(col.shape[1]), int(col.shape[2])
    ch = 1 if flat else int(col.shape[3])
    dep = _dev(depth, torch.uint16).reshape(F, -1)
    n_px = int(dep.shape[1])
    table = _dev(xy, torch.float32).reshape(-1, n_px, 2) if n_px else _dev(xy, torch.float32).reshape(S, 0, 2)
    if table.shape[0] != S:
        raise L.KinectPxError(f"color_to_depth: {table.shape[0]} tables for {S} calibrations")
    pack, _ = _calibration_pack("color_to_depth", cals, (wc, hc))
    if out is None:
        out = torch.empty((F, n_px) if flat else (F, n_px, ch), dtype=torch.uint8, device=dep.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.numel() == F * n_px * ch):
        raise ValueError(f"color_to_depth: out must be a contiguous uint8 device tensor of {F * n_px * ch} elements")
    if warped is None:
        L.check(lib.kpx_color_to_depth(L.ptr(dep), L.ptr(table), L.ptr(col), n_px, F, wc, hc, ch, L.hptr(pack), S, SAMPLE_MODES[interpolation], L.ptr(out),
                                       L.stream_ptr()))
        return out
    wrp = _dev(warped, torch.uint16)
    if wrp.numel() != F * hc * wc:
        raise L.KinectPxError(f"color_to_depth: warped has {wrp.numel()} elements, expected {F} x {hc} x {wc}")
    L.check(lib.kpx_color_to_depth_visible(L.ptr(dep), L.ptr(table), L.ptr(col), n_px, F, wc, hc, ch, L.hptr(pack), S, SAMPLE_MODES[interpolation],
                                           L.ptr(wrp), float(occlusion_mm), L.ptr(out), L.stream_ptr()))
    return out


# ---- lens undistortion (AC22) -------------------------------------------------------------------------------
def _pinhole4(who, pinhole):
    """the target of an undistortion -- a distortion-free calibration.CameraIntrinsics, or anything with width, height and
    intrinsic_matrix (o3d.camera.PinholeCameraIntrinsic) -> float64[4] fx' fy' cx' cy', width, height"""
    if hasattr(pinhole, "has_distortion"):
        if pinhole.has_distortion():
            raise ValueError(f"{who}: the target camera has lens distortion (CameraIntrinsics.undistorted() gives one without)")
        a = [pinhole.fx, pinhole.fy, pinhole.cx, pinhole.cy]
    else:
        K = np.asarray(pinhole.intrinsic_matrix, dtype=np.float64).reshape(3, 3)
        a = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    return np.ascontiguousarray(a, dtype=np.float64), int(pinhole.width), int(pinhole.height)


def undistort_map(camera, pinhole):
    """AC22's map of a lens (camera: a calibration.CameraIntrinsics or 13 numbers) for a distortion-free target camera `pinhole`
    (its width and height are the map's): float32 (H', W', 2) device tensor, per target pixel the source pixel coordinates (u, v) it
    sees -- the lens model in its closed-form direction, rounded once --, NaN pairs beyond the metric radius.  What remap /
    remap_depth take as `maps`."""
    lib = L.load()
    cam = _camera13(camera)
    pin, w, h = _pinhole4("undistort_map", pinhole)
    if w < 0 or h < 0:
        raise L.KinectPxError(f"undistort_map: negative image size {w} x {h}")
    out = torch.empty((h, w, 2), dtype=torch.float32, device=L.device())
    L.check(lib.kpx_undistort_map(L.hptr(cam), L.hptr(pin), w, h, L.ptr(out), L.stream_ptr()))
    return out


def _remap_args(who, src, maps, dtype, dims, interpolation):
    if interpolation not in SAMPLE_MODES:
        raise ValueError(f"{who}: unknown interpolation {interpolation!r}: expected one of {sorted(SAMPLE_MODES)}")
    src = src if isinstance(src, torch.Tensor) else np.asarray(src)
    maps = maps if isinstance(maps, torch.Tensor) else np.asarray(maps)
    if len(src.shape) not in dims:
        raise L.KinectPxError(f"{who}: src has {len(src.shape)} dimensions, expected (F, H, W" + (", C) or (F, H, W)" if len(dims) > 1 else ")"))
    if len(maps.shape) not in (3, 4) or int(maps.shape[-1]) != 2:
        raise L.KinectPxError(f"{who}: maps must be float32 (M, H', W', 2) or (H', W', 2)")
    M = int(maps.shape[0]) if len(maps.shape) == 4 else 1
    F = int(src.shape[0])
    if not 1 <= M <= SENSOR_MAX_CALIBRATIONS:
        raise L.KinectPxError(f"{who}: 1 to {SENSOR_MAX_CALIBRATIONS} maps, got {M}")
    if F % M != 0:
        raise L.KinectPxError(f"{who}: {M} maps do not divide {F} frames")
    return _dev(src, dtype), _dev(maps, torch.float32), F, M, int(maps.shape[-3]), int(maps.shape[-2])


def remap(src, maps, interpolation, out=None):
    """AC22: images resampled through stored maps.  src uint8 (F, H, W, C) or (F, H, W), C in {1, 3}; maps float32 (M, H', W', 2) --
    undistort_map's, (H', W', 2) for one; frame f uses map f % M and M divides F.  interpolation: "bilinear" (colour) or "nearest"
    (masks, labels, colour images with holes).  -> uint8 (F, H', W', C) (or (F, H', W')): color_to_depth's two samplers at the map's
    coordinates, zeros where the map entry is NaN or the sample lies outside the source image.
    out: a contiguous uint8 device tensor of F * H' * W' * C elements to write into."""
    lib = L.load()
    col, table, F, M, ho, wo = _remap_args("remap", src, maps, torch.uint8, (3, 4), interpolation)
    flat = col.dim() == 3
    hs, ws = int(col.shape[1]), int(col.shape[2])
    ch = 1 if flat else int(col.shape[3])
    if out is None:
        out = torch.empty((F, ho, wo) if flat else (F, ho, wo, ch), dtype=torch.uint8, device=col.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.numel() == F * ho * wo * ch):
        raise ValueError(f"remap: out must be a contiguous uint8 device tensor of {F * ho * wo * ch} elements")
    L.check(lib.kpx_remap_u8(L.ptr(col), L.ptr(table), ws, hs, ch, wo, ho, F, M, SAMPLE_MODES[interpolation], L.ptr(out), L.stream_ptr()))
    return out


def remap_depth(src, maps, interpolation="nearest", max_gap_mm=None, out=None):
    """AC22: depth images resampled through stored maps.  src uint16 (F, H, W) mm; maps as in remap.  "nearest" copies the nearest
    source pixel (0 stays 0); "bilinear" is depth aware: 0 when one of the four neighbours is 0 or when they differ by more than
    max_gap_mm (a blend across a depth edge would invent a surface), AC20's bilinear value otherwise.  max_gap_mm is required for
    "bilinear" and has no default: it is a property of the scene and the rig that nothing in this project measures
    (float("inf"): never).  -> uint16 (F, H', W').  out: a contiguous uint16 device tensor of F * H' * W' elements to write into."""
    lib = L.load()
    if interpolation == "bilinear" and max_gap_mm is None:
        raise ValueError("remap_depth: the bilinear mode needs max_gap_mm (no default: it depends on the scene and the rig)")
    dep, table, F, M, ho, wo = _remap_args("remap_depth", src, maps, torch.uint16, (3,), interpolation)
    hs, ws = int(dep.shape[1]), int(dep.shape[2])
    if out is None:
        out = torch.empty((F, ho, wo), dtype=torch.uint16, device=dep.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint16 and out.is_cuda and out.is_contiguous() and out.numel() == F * ho * wo):
        raise ValueError(f"remap_depth: out must be a contiguous uint16 device tensor of {F * ho * wo} elements")
    L.check(lib.kpx_remap_depth(L.ptr(dep), L.ptr(table), ws, hs, wo, ho, F, M, SAMPLE_MODES[interpolation], float(0.0 if max_gap_mm is None else max_gap_mm),
                                L.ptr(out), L.stream_ptr()))
    return out

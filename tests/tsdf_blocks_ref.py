"""NumPy restatement of arithmetic contract AC16: the block-sparse TSDF volume.  Touched sets operation by
operation; integration per block through tsdf_ref.Volume / tsdf_ref.integrate with origin = b ul (AC9 as it stands); the two
point-cloud extractions by global voxel index; marching cubes as a literal serial walk over the blocks' cubes with a dict from edge
key to vertex (AC12's arithmetic, corners looked up block by block).  Imports tsdf_ref and tsdf_mesh_ref, nothing from the package."""
import numpy as np

import tsdf_mesh_ref as M
import tsdf_ref as R

INDEX_LIMIT = 1 << 20            # block indices live in [-2^20, 2^20)


class Blocks:
    """units: dict (bx, by, bz) -> tsdf_ref.Volume of unit_resolution^3 voxels with origin b ul"""

    def __init__(self, voxel_length, sdf_trunc, unit_resolution=16, stride=4, color=False):
        self.vl, self.trunc, self.R, self.stride, self.color = float(voxel_length), float(sdf_trunc), int(unit_resolution), int(stride), bool(color)
        self.ul = self.vl * self.R                       # one fp64 product
        assert self.trunc <= self.ul
        self.units = {}

    def unit(self, b):
        """the block b, created all zero when it does not exist"""
        b = tuple(int(v) for v in b)
        if b not in self.units:
            v = R.Volume(self.ul, self.R, self.trunc, [float(k) * self.ul for k in b], self.color)
            v.vl = self.vl                               # the contract's voxel length, not ul / R rounded again
            self.units[b] = v
        return self.units[b]

    def indices(self):
        return np.asarray(sorted(self.units), dtype=np.int32).reshape(-1, 3)

    def arrays(self):
        """(float32 (B, R^3, 2), float32 (B, R^3, 3) or None) in ascending block order"""
        keys = sorted(self.units)
        tw = np.stack([np.stack([self.units[b].tsdf, self.units[b].w], 1) for b in keys]) if keys else np.zeros((0, self.R ** 3, 2), np.float32)
        col = None
        if self.color:
            col = np.stack([self.units[b].col for b in keys]) if keys else np.zeros((0, self.R ** 3, 3), np.float32)
        return tw, col

    def copy(self):
        o = Blocks(self.vl, self.trunc, self.R, self.stride, self.color)
        o.units = {b: v.copy() for b, v in self.units.items()}
        for v in o.units.values():
            v.vl = self.vl
        return o


def from_dense(tsdf, weight, color, res, voxel_length, unit_resolution, first_block=(0, 0, 0), keep=None):
    """a dense res^3 volume (res a multiple of unit_resolution) cut into blocks, the block at the dense origin being first_block;
    keep: None or a predicate on the block index"""
    r = int(unit_resolution)
    n = res // r
    assert n * r == res
    out = Blocks(voxel_length, voxel_length * r, r, 1, color is not None)
    f, w = np.asarray(tsdf, np.float32).reshape(res, res, res), np.asarray(weight, np.float32).reshape(res, res, res)
    c = None if color is None else np.asarray(color, np.float32).reshape(res, res, res, 3)
    for i in range(n):
        for j in range(n):
            for k in range(n):
                b = (first_block[0] + i, first_block[1] + j, first_block[2] + k)
                if keep is not None and not keep(b):
                    continue
                u = out.unit(b)
                s = (slice(i * r, (i + 1) * r), slice(j * r, (j + 1) * r), slice(k * r, (k + 1) * r))
                u.tsdf[:], u.w[:] = f[s].reshape(-1), w[s].reshape(-1)
                if c is not None:
                    u.col[:] = c[s].reshape(-1, 3)
    return out


# ---- touched blocks and integration ----------------------------------------------------------------------------------------------
def touched(blocks, depth, intrinsic, width, height, extrinsic):
    """the sorted list of the blocks one float32 depth image touches (AC16, steps 1 to 10)"""
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    W, H, s = int(width), int(height), blocks.stride
    pose = np.linalg.inv(np.asarray(extrinsic, np.float64).reshape(4, 4))
    d = np.asarray(depth, np.float32).reshape(H, W)
    i, j = np.meshgrid(np.arange(0, H, s), np.arange(0, W, s), indexing="ij")
    d = d[i, j]
    sel = ~(d <= np.float32(0.0))
    i, j, z = i[sel].astype(np.float64), j[sel].astype(np.float64), d[sel].astype(np.float64)
    x = (j - cx) * z / fx
    y = (i - cy) * z / fy
    p = R.ac1(pose, x, y, z)
    lo = [np.floor((p[k] - blocks.trunc) / blocks.ul) for k in range(3)]
    hi = [np.floor((p[k] + blocks.trunc) / blocks.ul) for k in range(3)]
    out = set()
    if len(z) == 0:
        return []
    if min(l.min() for l in lo) < -INDEX_LIMIT or max(h.max() for h in hi) >= INDEX_LIMIT:
        raise OverflowError("block index outside [-2^20, 2^20)")
    lo = np.stack(lo, 1).astype(np.int64)
    span = np.stack(hi, 1).astype(np.int64) - lo
    for dx in range(int(span[:, 0].max()) + 1):
        for dy in range(int(span[:, 1].max()) + 1):
            for dz in range(int(span[:, 2].max()) + 1):
                m = (span[:, 0] >= dx) & (span[:, 1] >= dy) & (span[:, 2] >= dz)
                out.update(map(tuple, np.unique(lo[m] + np.array([dx, dy, dz]), axis=0).tolist()))
    return sorted(out)


def integrate(blocks, depth, rgb, intrinsic, width, height, extrinsic):
    """one image: every block it touches (created when absent) takes AC9's update; no other block changes.  -> the touched list"""
    t = touched(blocks, depth, intrinsic, width, height, extrinsic)
    for b in t:
        R.integrate(blocks.unit(b), depth, rgb, intrinsic, width, height, extrinsic)
    return t


# ---- the point-cloud extractions, by global voxel index ----------------------------------------------------------------------------
PAD = 2          # a normal's taps reach one voxel below and two above the lower voxel of a crossing


def _dense(blocks):
    """the blocks laid into one array with a margin of PAD voxels: (g0 = global index of element 0, tsdf, weight, present, colours)"""
    r = blocks.R
    idx = np.asarray(sorted(blocks.units), dtype=np.int64).reshape(-1, 3)
    lo, hi = idx.min(0), idx.max(0) + 1
    shape = tuple(int(v) for v in (hi - lo) * r + 2 * PAD)
    assert np.prod(shape) < 1 << 27, "the restatement lays the blocks into one dense array: keep the scene small"
    f, w, present = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape, bool)
    c = np.zeros(shape + (3,), np.float32) if blocks.color else None
    for b in map(tuple, idx.tolist()):
        o = [(b[k] - int(lo[k])) * r + PAD for k in range(3)]
        s = tuple(slice(o[k], o[k] + r) for k in range(3))
        u = blocks.units[b]
        f[s], w[s], present[s] = u.tsdf.reshape(r, r, r), u.w.reshape(r, r, r), True
        if c is not None:
            c[s] = u.col.reshape(r, r, r, 3)
    return lo * r - PAD, f, w, present, c


def _order(blocks, g, axis=None):
    """the contract's output order of global voxel indices g (K, 3): ascending (block index, local linear index[, axis])"""
    r = blocks.R
    b, l = g // r, g % r
    lin = (l[:, 0] * r + l[:, 1]) * r + l[:, 2]
    keys = (lin, b[:, 2], b[:, 1], b[:, 0]) if axis is None else (axis, lin, b[:, 2], b[:, 1], b[:, 0])
    return np.lexsort(keys)


def _centres(blocks, g):
    """(double) b ul + ((double) i + 0.5) vl per axis"""
    r = blocks.R
    b, l = g // r, g % r
    return b.astype(np.float64) * blocks.ul + (l.astype(np.float64) + 0.5) * blocks.vl


def extract_voxel_point_cloud(blocks):
    if not blocks.units:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    g0, f, w, present, _ = _dense(blocks)
    valid = present & (w != 0) & (f >= R.VALID_LO) & (f < R.VALID_HI)
    at = np.argwhere(valid)
    g = at + g0[None, :]
    o = _order(blocks, g)
    at, g = at[o], g[o]
    grey = ((f[tuple(at.T)].astype(np.float64) + 1.0) * 0.5).astype(np.float32)
    return _centres(blocks, g).astype(np.float32), np.repeat(grey[:, None], 3, 1)


def _tsdf_at(blocks, g0, f, q):
    g = q / blocks.vl - 0.5
    fl = np.floor(g)
    r = g - fl
    i0 = fl.astype(np.int64) - g0[None, :]
    acc = np.zeros(len(q))
    for t in range(8):
        dx, dy, dz = t >> 2, (t >> 1) & 1, t & 1
        wx = r[:, 0] if dx else 1.0 - r[:, 0]
        wy = r[:, 1] if dy else 1.0 - r[:, 1]
        wz = r[:, 2] if dz else 1.0 - r[:, 2]
        x, y, z = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
        inside = (x >= 0) & (x < f.shape[0]) & (y >= 0) & (y < f.shape[1]) & (z >= 0) & (z < f.shape[2])
        fv = np.zeros(len(q), np.float32)
        fv[inside] = f[x[inside], y[inside], z[inside]]                # an absent block holds zeros
        acc = acc + wx * wy * wz * fv.astype(np.float64)
    return acc


def extract_point_cloud(blocks):
    """-> points, normals, colours (None without colours): float32 (K, 3), ascending (block index, local index, axis)"""
    if not blocks.units:
        z = np.zeros((0, 3), np.float32)
        return z, z.copy(), (z.copy() if blocks.color else None)
    g0, f, w, present, c = _dense(blocks)
    vl = blocks.vl
    valid = present & (w != 0) & (f >= R.VALID_LO) & (f < R.VALID_HI)
    fd = f.astype(np.float64)
    ats, axes = [], []
    for i in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[i], hi[i] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        at = np.argwhere(valid[lo] & valid[hi] & (fd[lo] * fd[hi] < 0.0))
        ats.append(at)
        axes.append(np.full(len(at), i, np.int64))
    at, axis = np.concatenate(ats), np.concatenate(axes)
    o = _order(blocks, at + g0[None, :], axis)
    at, axis = at[o], axis[o]
    K = len(at)
    rows = np.arange(K)
    at1 = at.copy()
    at1[rows, axis] += 1
    f0, f1 = f[tuple(at.T)], f[tuple(at1.T)]
    r0, r1 = np.abs(f0.astype(np.float64)), np.abs(f1.astype(np.float64))
    p0 = _centres(blocks, at + g0[None, :])
    p = p0.copy()
    pa = p0[rows, axis]
    with np.errstate(all="ignore"):
        p[rows, axis] = (pa * r1 + (pa + vl) * r0) / (r0 + r1)
    pts = p.astype(np.float32)
    col = None
    if c is not None:
        c0, c1 = c[tuple(at.T)].astype(np.float64), c[tuple(at1.T)].astype(np.float64)
        col = ((c0 * r1[:, None] + c1 * r0[:, None]) / (r0 + r1)[:, None] / 255.0).astype(np.float32)
    gap = 0.99 * vl
    n = np.zeros((K, 3))
    for k in range(3):
        qp, qm = p.copy(), p.copy()
        qp[:, k] = p[:, k] + gap
        qm[:, k] = p[:, k] - gap
        n[:, k] = _tsdf_at(blocks, g0, f, qp) - _tsdf_at(blocks, g0, f, qm)
    length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    with np.errstate(all="ignore"):
        nrm = np.where(length[:, None] == 0.0, 0.0, n / length[:, None]).astype(np.float32)
    return pts, nrm, col


# ---- marching cubes ----------------------------------------------------------------------------------------------------------------
def _lattice(blocks, b):
    """the (R + 1)^3 corner lattice of block b's cubes: the block and the first layers of its seven forward neighbours; a corner in
    an absent block has weight 0"""
    r = blocks.R
    f, w = np.zeros((r + 1,) * 3, np.float32), np.zeros((r + 1,) * 3, np.float32)
    c = np.zeros((r + 1,) * 3 + (3,), np.float32) if blocks.color else None
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                u = blocks.units.get((b[0] + dx, b[1] + dy, b[2] + dz))
                if u is None:
                    continue
                dst = tuple(slice(r, r + 1) if d else slice(0, r) for d in (dx, dy, dz))
                src = tuple(slice(0, 1) if d else slice(0, r) for d in (dx, dy, dz))
                f[dst], w[dst] = u.tsdf.reshape(r, r, r)[src], u.w.reshape(r, r, r)[src]
                if c is not None:
                    c[dst] = u.col.reshape(r, r, r, 3)[src]
    return f, w, c


def extract_triangle_mesh(blocks):
    """AC12 by global voxel index: a cube at every voxel of every block.  -> (vertices float32 (V, 3), colours float32 (V, 3) or None,
    triangles int32 (T, 3), keys int64 (V, 5) = (bx, by, bz, local index, axis) of each vertex's lower voxel), vertices ascending in
    their key, triangles in ascending (block, cube)"""
    r, vl, ul = blocks.R, blocks.vl, blocks.ul
    first, verts, cols, keys, tris = {}, [], [], [], []
    for b in sorted(blocks.units):
        f, w, c = _lattice(blocks, b)
        codes = M.cube_codes(f.reshape(-1), w.reshape(-1), r + 1)
        for x, y, z in np.argwhere((codes != 0) & (codes != 255)).tolist():
            code = int(codes[x, y, z])
            mask = M.edge_mask(code)
            idx = [-1] * 12
            for e in range(12):
                if not (mask >> e) & 1:
                    continue
                dx, dy, dz, a = M.EDGE_SHIFTS[e]
                v0 = [x + dx, y + dy, z + dz]
                v1 = list(v0)
                v1[a] += 1
                g = [b[k] * r + v0[k] for k in range(3)]
                gb, gl = [g[k] // r for k in range(3)], [g[k] % r for k in range(3)]
                key = (gb[0], gb[1], gb[2], (gl[0] * r + gl[1]) * r + gl[2], a)
                if key not in first:
                    f0, f1 = abs(float(f[tuple(v0)])), abs(float(f[tuple(v1)]))
                    p = [float(gb[k]) * ul + (float(gl[k]) + 0.5) * vl for k in range(3)]
                    p[a] = p[a] + (f0 * vl) / (f0 + f1)
                    first[key] = len(verts)
                    verts.append(p)
                    keys.append(key)
                    if c is not None:
                        c0, c1 = c[tuple(v0)], c[tuple(v1)]
                        cols.append([(f1 * (float(c0[k]) / 255.0) + f0 * (float(c1[k]) / 255.0)) / (f0 + f1) for k in range(3)])
                idx[e] = first[key]
            row = M.row(code)
            for t in range(0, len(row), 3):
                tris.append([idx[row[t]], idx[row[t + 2]], idx[row[t + 1]]])
    V = len(verts)
    order = sorted(range(V), key=lambda i: keys[i])
    new = np.empty(V, dtype=np.int64)
    new[order] = np.arange(V)
    with np.errstate(over="ignore", invalid="ignore"):
        vout = np.asarray(verts, dtype=np.float64).reshape(-1, 3)[order].astype(np.float32)
        cout = np.asarray(cols, dtype=np.float64).reshape(-1, 3)[order].astype(np.float32) if blocks.color else None
    tout = new[np.asarray(tris, dtype=np.int64).reshape(-1, 3)].astype(np.int32)
    kout = np.asarray(keys, dtype=np.int64).reshape(-1, 5)[order]
    return vout, cout, tout, kout

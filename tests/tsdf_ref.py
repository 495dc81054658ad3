"""NumPy restatement of the arithmetic contract AC9: integration of depth images into a uniform TSDF volume
and the two point-cloud extractions, operation by operation -- float32 where the contract says float32, float64 elsewhere, every
fused multiply-add an exact one.  Vectorised over the volume: resolution 64 takes well under a second per image.

NumPy has no fma.  `fma` below is the Boldo-Melquiond emulation: a b = ph + pl exactly (Dekker's product), ph + c = sh + sl exactly
(Knuth's sum), and RN(sh + RO(sl + pl)) with RO = rounding to odd is the correctly rounded a b + c.  test_tsdf_cpu.py checks it
against the C library's fma.
"""
import numpy as np

VALID_LO, VALID_HI = np.float32(-0.98), np.float32(0.98)
COUNT_BLOCK = 512           # KPX_TSDF_COUNT_BLOCK: consecutive voxels per count of the extraction's first pass
MAX_SENSORS = 8             # KPX_TSDF_MAX_SENSORS: images per launch of the integration kernel


# ---- exact fused multiply-add on float64 arrays ------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """correctly rounded a * b + c, elementwise (finite values far from overflow and underflow)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    ph, pl = _two_prod(a, b)
    sh, sl = _two_sum(c, ph)
    v, e = _two_sum(sl, pl)                           # v = RN(sl + pl), e its error: round v to odd
    even = (np.ascontiguousarray(v).view(np.int64) & 1) == 0
    v = np.where((e != 0.0) & even, np.nextafter(v, np.where(e > 0.0, np.inf, -np.inf)), v)
    return sh + v


def ac1(E, x, y, z):
    """rows of p' = E (x, y, z, 1): p'_k = fma(E_k0, x, fma(E_k1, y, fma(E_k2, z, E_k3)))"""
    return [fma(E[k, 0], x, fma(E[k, 1], y, fma(E[k, 2], z, E[k, 3]))) for k in range(3)]


# ---- the volume ------------------------------------------------------------------------------------------------------------------
class Volume:
    def __init__(self, length, resolution, sdf_trunc, origin=(0.0, 0.0, 0.0), color=False):
        self.length, self.res, self.trunc = float(length), int(resolution), float(sdf_trunc)
        self.vl = self.length / self.res
        self.origin = np.asarray(origin, np.float64).reshape(3)
        n = self.res ** 3
        self.tsdf, self.w = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.col = np.zeros((n, 3), np.float32) if color else None

    def copy(self):
        v = Volume(self.length, self.res, self.trunc, self.origin, self.col is not None)
        v.tsdf, v.w = self.tsdf.copy(), self.w.copy()
        v.col = None if self.col is None else self.col.copy()
        return v

    def reset(self):
        self.tsdf[:] = 0
        self.w[:] = 0
        if self.col is not None:
            self.col[:] = 0

    def centres(self):
        """per-axis voxel centres origin_k + (i + 0.5) voxel_length (one multiplication, one addition)"""
        i = np.arange(self.res, dtype=np.float64)
        return [self.origin[k] + (i + 0.5) * self.vl for k in range(3)]


def depth_from_u16(raw, depth_scale, depth_trunc):
    """RGBDImage.create_from_color_and_depth's depth: float32 raw / float32 scale, above float32 trunc -> 0"""
    d = np.asarray(raw).astype(np.float32) / np.float32(depth_scale)
    d[d > np.float32(depth_trunc)] = np.float32(0.0)
    return d


def integrate(vol, depth, rgb, intrinsic, width, height, extrinsic):
    """one image: depth float32 (H W), rgb uint8 (H W, 3) or None, intrinsic (fx, fy, cx, cy), extrinsic world -> camera 4x4"""
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    W, H, res = int(width), int(height), vol.res
    E = np.asarray(extrinsic, np.float64).reshape(4, 4)
    depth = np.asarray(depth, np.float32).reshape(-1)
    gx, gy, gz = vol.centres()
    X, Y, Z = gx[:, None, None], gy[None, :, None], gz[None, None, :]
    px, py, pz = (np.broadcast_to(p, (res, res, res)).reshape(-1) for p in ac1(E, X, Y, Z))
    sel = np.flatnonzero(~(pz <= 0.0))
    px, py, pz = px[sel], py[sel], pz[sel]
    with np.errstate(all="ignore"):
        uf = px * fx / pz + cx + 0.5
        vf = py * fy / pz + cy + 0.5
    ok = (uf >= 0.0001) & (uf < W - 0.0001) & (vf >= 0.0001) & (vf < H - 0.0001)
    sel, uf, vf, pz = sel[ok], uf[ok], vf[ok], pz[ok]
    u, v = uf.astype(np.int64), vf.astype(np.int64)              # truncation, as (int)
    pix = v * W + u
    d = depth[pix]
    ok = ~(d <= np.float32(0.0))
    sel, u, v, pix, d, pz = sel[ok], u[ok], v[ok], pix[ok], d[ok], pz[ok]
    xm, ym = (u.astype(np.float64) - cx) / fx, (v.astype(np.float64) - cy) / fy
    mult = np.sqrt(xm * xm + ym * ym + 1.0)
    sdf = (d.astype(np.float64) - pz) * mult
    ok = sdf > -vol.trunc
    sel, pix, sdf = sel[ok], pix[ok], sdf[ok]
    t = np.minimum(1.0, sdf / vol.trunc).astype(np.float32)
    w = vol.w[sel]
    w1 = w + np.float32(1.0)
    vol.tsdf[sel] = (vol.tsdf[sel] * w + t) / w1
    if vol.col is not None:
        c = np.asarray(rgb, np.uint8).reshape(-1, 3)[pix].astype(np.float32)
        vol.col[sel] = (vol.col[sel] * w[:, None] + c) / w1[:, None]
    vol.w[sel] = w1
    return len(sel)


# ---- extraction ------------------------------------------------------------------------------------------------------------------
def valid_mask(vol):
    return (vol.w != 0) & (vol.tsdf >= VALID_LO) & (vol.tsdf < VALID_HI)


def crossings(vol):
    """(linear index, axis) of every emitted surface point, in output order"""
    res = vol.res
    valid = valid_mask(vol).reshape(res, res, res)
    f = vol.tsdf.astype(np.float64).reshape(res, res, res)
    lin = np.arange(res ** 3, dtype=np.int64).reshape(res, res, res)
    keys = []
    for i in range(3):
        if res - 2 <= 0:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[i], hi[i] = slice(0, res - 2), slice(1, res - 1)            # idx1[i] = idx0[i] + 1 < res - 1
        lo, hi = tuple(lo), tuple(hi)
        m = valid[lo] & valid[hi] & (f[lo] * f[hi] < 0.0)
        keys.append(lin[lo][m] * 3 + i)
    keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    return keys // 3, (keys % 3).astype(np.int64)


def _tsdf_at(vol, q):
    """trilinear interpolation of the raw tsdf at q (K, 3), volume coordinates without the origin; outside taps are 0"""
    res = vol.res
    g = q / vol.vl - 0.5
    fl = np.floor(g)
    r = g - fl
    i0 = fl.astype(np.int64)
    acc = np.zeros(len(q))
    for t in range(8):
        dx, dy, dz = t >> 2, (t >> 1) & 1, t & 1
        wx = r[:, 0] if dx else 1.0 - r[:, 0]
        wy = r[:, 1] if dy else 1.0 - r[:, 1]
        wz = r[:, 2] if dz else 1.0 - r[:, 2]
        x, y, z = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
        inside = (x >= 0) & (x < res) & (y >= 0) & (y < res) & (z >= 0) & (z < res)
        fv = np.zeros(len(q), np.float32)
        fv[inside] = vol.tsdf[((x * res + y) * res + z)[inside]]
        acc = acc + wx * wy * wz * fv.astype(np.float64)
    return acc


def extract_point_cloud(vol, want_normals=True):
    """-> points, normals, colours (None without a colour volume): float32 (K, 3), ascending (linear index, axis)"""
    res, vl = vol.res, vol.vl
    lin, axis = crossings(vol)
    K = len(lin)
    step = np.array([res * res, res, 1], np.int64)
    idx = np.stack([lin // (res * res), (lin // res) % res, lin % res], 1)
    p0 = (idx.astype(np.float64) + 0.5) * vl
    lin1 = lin + step[axis]
    r0, r1 = np.abs(vol.tsdf[lin].astype(np.float64)), np.abs(vol.tsdf[lin1].astype(np.float64))
    p = p0.copy()
    rows = np.arange(K)
    pa = p0[rows, axis]
    with np.errstate(all="ignore"):
        p[rows, axis] = (pa * r1 + (pa + vl) * r0) / (r0 + r1)
    pts = (p + vol.origin[None, :]).astype(np.float32)
    col = None
    if vol.col is not None:
        c0, c1 = vol.col[lin].astype(np.float64), vol.col[lin1].astype(np.float64)
        col = ((c0 * r1[:, None] + c1 * r0[:, None]) / (r0 + r1)[:, None] / 255.0).astype(np.float32)
    nrm = None
    if want_normals:
        gap = 0.99 * vl
        n = np.zeros((K, 3))
        for k in range(3):
            qp, qm = p.copy(), p.copy()
            qp[:, k] = p[:, k] + gap
            qm[:, k] = p[:, k] - gap
            n[:, k] = _tsdf_at(vol, qp) - _tsdf_at(vol, qm)
        length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        with np.errstate(all="ignore"):
            nrm = np.where(length[:, None] == 0.0, 0.0, n / length[:, None]).astype(np.float32)
    return pts, nrm, col


def extract_voxel_point_cloud(vol):
    """-> centres of the valid voxels float32 (K, 3) ascending, grey colours (tsdf + 1) / 2 float32 (K, 3)"""
    res = vol.res
    lin = np.flatnonzero(valid_mask(vol)).astype(np.int64)
    idx = np.stack([lin // (res * res), (lin // res) % res, lin % res], 1)
    pts = (vol.origin[None, :] + (idx.astype(np.float64) + 0.5) * vol.vl).astype(np.float32)
    g = ((vol.tsdf[lin].astype(np.float64) + 1.0) * 0.5).astype(np.float32)
    return pts, np.repeat(g[:, None], 3, 1)

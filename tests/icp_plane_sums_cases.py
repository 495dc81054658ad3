"""Inputs and cases of tests/test_icp_plane_sums_gpu.py, shared with the recorder tests/golden/make_icp_plane_sums_golden.py and run
as that test's child process: `python tests/icp_plane_sums_cases.py <out.npz>` (the KPX_* form switches are read once per process).

The culled registration accumulates only the update sums its mode reads (kpx_icpdefs.h, acc_live): every result here must stay what
the library gave while it still accumulated all 44.  Small on purpose: a 300-point target on a smooth non-planar surface with
ANALYTIC unit normals (the normals kernel is not involved), sources cut at the tile edge (16 rows), the block edge (64) and one row
past each, a source out of reach (count 0, identity update) and one with a third of its rows out of reach."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_DIST = 60.0                                   # max_correspondence_distance (the surface's points are ~29 apart)
SIZES = (1, 15, 16, 17, 63, 64, 65, 129)
BATCH = (65, 17, 129)                             # three ragged registrations onto the shared target (the grouped driver)
MODES = ("p2p", "p2plane")
ITERATIONS = (0, 1, 30)


def _rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def inputs():
    """-> target (300, 3) float32, its normals (300, 3) float32, {name: source float32}, {name: initial transform}"""
    rng = np.random.default_rng(20261021)
    xy = rng.uniform(-250.0, 250.0, size=(300, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 40.0 * np.sin(x / 90.0) + 30.0 * np.cos(y / 70.0) + 4e-4 * x * y
    tgt = np.stack([x, y, z], 1).astype(np.float32)
    zx = 40.0 / 90.0 * np.cos(x / 90.0) + 4e-4 * y
    zy = -30.0 / 70.0 * np.sin(y / 70.0) + 4e-4 * x
    nrm = np.stack([-zx, -zy, np.ones_like(zx)], 1)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    # the copy: every target point moved by one rigid transform, in a shuffled order
    P = _rigid(0.021, -0.017, 0.030, (4.0, -3.0, 5.0))
    moved = (tgt[rng.permutation(300)].astype(np.float64) @ P[:3, :3].T + P[:3, 3]).astype(np.float32)
    srcs = {"n%d" % n: np.ascontiguousarray(moved[:n]) for n in SIZES}
    srcs["far"] = np.ascontiguousarray(moved[:65] + np.float32([0.0, 0.0, 1000.0]))
    part = moved[:129].copy()
    part[::3] += np.float32([0.0, 0.0, 1000.0])
    srcs["partial"] = part
    inits = {name: np.eye(4) for name in srcs}
    inits["n129"] = _rigid(0.004, 0.003, -0.005, (1.0, 0.5, -1.5))           # one registration that does not start at the identity
    return tgt, nrm, srcs, inits


def _put(out, key, r):
    out[key + ".T"] = np.asarray(r["transformation"], dtype=np.float64)
    out[key + ".s"] = np.array([r["fitness"], r["inlier_rmse"], r["iterations"], r["count"]], dtype=np.float64)


def run(ops):
    """every case through the library behind `ops` -> {key: float64 array}"""
    tgt, nrm, srcs, inits = inputs()
    out = {}
    for mode in MODES:
        tn = nrm if mode == "p2plane" else None
        for it in ITERATIONS:
            for name, src in srcs.items():
                _put(out, "%s.it%d.icp.%s" % (mode, it, name), ops.icp(src, tgt, MAX_DIST, inits[name], mode, tn, it))
            names = ["n%d" % n for n in BATCH]
            rs = ops.icp_batch([srcs[n] for n in names], tgt, MAX_DIST, [inits[n] for n in names], mode, tn, it)
            for n, r in zip(names, rs):
                _put(out, "%s.it%d.batch.%s" % (mode, it, n), r)
    return out


def same_bits(a, b):
    """the raw values: equal bit patterns (which also holds a NaN equal to itself)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from kinectpy_amd import ops as _ops
    np.savez(sys.argv[1], **run(_ops))

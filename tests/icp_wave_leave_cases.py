"""Inputs and cases of tests/test_icp_wave_leave_gpu.py, shared with the recorder tests/golden/make_icp_wave_leave_golden.py and run as
that test's child process: `python tests/icp_wave_leave_cases.py <out.npz>` (the KPX_* form switches are read once per process).

In the block form of the culled registration (icp_iter_body, kpx_icpiter.h) a wave ends with its 16 rows and the last wave of a block
to arrive closes the block alone: the tile trees, the adds, the ticket and, as winner, the update.  The sums are a tree per 16-row tile
followed by exact fixed-point adds, so every result must stay what the library gave while the four waves met at a barrier, to the last
bit, and the same in every run.  Small on purpose:
  * a target of two clusters 2000 apart on smooth non-planar surfaces with ANALYTIC unit normals (the normals kernel is not involved);
  * sources of 1, 17, 33 and 49 rows -- three, two or one wave(s) of the only block own no row and must still arrive -- and of 65, 200
    and 1000 rows;
  * `mixed`: 200 rows of which 72 hang 1000 above the first cluster, out of reach: inside one block some tiles' rows have no partner in
    reach and finish at once while others search;
  * `far`: wholly out of reach (count 0, identity update, and from the second iteration the LightSkip path);
  * a ragged batch of three: `exact` (33 target points as they are: converges within three iterations), n200 and `slow` (1000 noisy rows of
    their own that start far from their pose and run all 30 iterations);
  * the edge cases once more as a batch of seven, side by side in one launch per iteration;
  * both modes, max_iteration 0, 1 and 30, through ops.icp (update in its own kernel, no ticket) and ops.icp_batch (ticket form).
REPEATS runs of every case in the process: run() keeps the first and counts the runs whose bits differ from it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_DIST = 60.0                                   # max_correspondence_distance (the surfaces' points are ~29 apart)
SIZES = (1, 17, 33, 49, 65, 200, 1000)
SINGLES = tuple("n%d" % n for n in SIZES) + ("mixed", "far")
BATCH = ("exact", "n200", "slow")                 # three ragged registrations onto the shared target (the grouped driver)
EDGES = ("n1", "n17", "n33", "n49", "n65", "mixed", "far")      # ... and the edge cases side by side in one launch per iteration
BATCHES = {"batch": BATCH, "edges": EDGES}
MODES = ("p2p", "p2plane")
ITERATIONS = (0, 1, 30)
REPEATS = 5
N_CLUSTER = 600
CLUSTER_GAP = 2000.0


def _rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def _surface(rng, n, x0):
    """n points of z = 40 sin(x/90) + 30 cos(y/70) + 4e-4 x y over a 700 x 700 patch, moved by x0 along x -> points, unit normals (f64)"""
    xy = rng.uniform(-350.0, 350.0, size=(n, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 40.0 * np.sin(x / 90.0) + 30.0 * np.cos(y / 70.0) + 4e-4 * x * y
    zx = 40.0 / 90.0 * np.cos(x / 90.0) + 4e-4 * y
    zy = -30.0 / 70.0 * np.sin(y / 70.0) + 4e-4 * x
    nrm = np.stack([-zx, -zy, np.ones_like(zx)], 1)
    return np.stack([x + x0, y, z], 1), nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def inputs():
    """-> target (1200, 3) float32, its normals float32, {name: source float32}, {name: initial transform}"""
    rng = np.random.default_rng(20261022)
    pa, na = _surface(rng, N_CLUSTER, 0.0)
    pb, nb = _surface(rng, N_CLUSTER, CLUSTER_GAP)
    tgt = np.concatenate([pa, pb]).astype(np.float32)
    nrm = np.concatenate([na, nb]).astype(np.float32)
    # the copy: every target point moved by one rigid transform (about the middle between the clusters), in a shuffled order
    P = _rigid(0.006, -0.005, 0.008, (4.0, -3.0, 5.0))
    c = np.array([CLUSTER_GAP / 2, 0.0, 0.0])
    moved = ((tgt[rng.permutation(2 * N_CLUSTER)].astype(np.float64) - c) @ P[:3, :3].T + P[:3, 3] + c).astype(np.float32)
    srcs = {"n%d" % n: np.ascontiguousarray(moved[:n]) for n in SIZES}
    first = (tgt[:N_CLUSTER].astype(np.float64) @ P[:3, :3].T + P[:3, 3]).astype(np.float32)       # the first cluster alone, in target order
    mixed = first[:200].copy()
    mixed[64:136] += np.float32([0.0, 0.0, 1000.0])
    srcs["mixed"] = mixed
    srcs["far"] = np.ascontiguousarray(moved[:65] + np.float32([0.0, 0.0, 1000.0]))
    srcs["exact"] = np.ascontiguousarray(tgt[100:133])
    # `slow`: 1000 points of its own on both surfaces, 12 of noise on every coordinate, far from their pose: the pairs keep changing
    rs = np.random.default_rng(6)
    qa, _ = _surface(rs, 500, 0.0)
    qb, _ = _surface(rs, 500, CLUSTER_GAP)
    q = np.concatenate([qa, qb])
    q = q + rs.normal(0.0, 12.0, size=q.shape)
    Q = _rigid(0.01, -0.008, 0.05, (45.0, -35.0, 8.0))
    srcs["slow"] = ((q - c) @ Q[:3, :3].T + Q[:3, 3] + c).astype(np.float32)
    inits = {name: np.eye(4) for name in srcs}
    inits["n65"] = _rigid(0.004, 0.003, -0.005, (1.0, 0.5, -1.5))            # one registration that does not start at the identity
    return tgt, nrm, srcs, inits


def _arrays(r):
    return (np.asarray(r["transformation"], dtype=np.float64).copy(),
            np.array([r["fitness"], r["inlier_rmse"], r["iterations"], r["count"]], dtype=np.float64))


def same_bits(a, b):
    """the raw values: equal bit patterns (which also holds a NaN equal to itself)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(ops, repeats=REPEATS):
    """every case through the library behind `ops`, `repeats` times each -> {key: float64 array} of the first run, with
    "unstable": the number of (case, later run) pairs whose bits differed from the first run's"""
    tgt, nrm, srcs, inits = inputs()
    out = {}
    unstable = 0

    def put(key, r, rep):
        nonlocal unstable
        T, s = _arrays(r)
        if rep == 0:
            out[key + ".T"], out[key + ".s"] = T, s
        elif not (same_bits(T, out[key + ".T"]) and same_bits(s, out[key + ".s"])):
            unstable += 1

    for mode in MODES:
        tn = nrm if mode == "p2plane" else None
        for it in ITERATIONS:
            for rep in range(repeats):
                for name in SINGLES:
                    put("%s.it%d.icp.%s" % (mode, it, name), ops.icp(srcs[name], tgt, MAX_DIST, inits[name], mode, tn, it), rep)
                for label, names in BATCHES.items():
                    rs = ops.icp_batch([srcs[n] for n in names], tgt, MAX_DIST, [inits[n] for n in names], mode, tn, it)
                    for n, r in zip(names, rs):
                        put("%s.it%d.%s.%s" % (mode, it, label, n), r, rep)
    out["unstable"] = np.array([float(unstable)])
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from kinectpy_amd import ops as _ops
    np.savez(sys.argv[1], **run(_ops))

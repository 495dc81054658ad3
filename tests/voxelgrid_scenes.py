"""Edge decisions of AC10 with exactly representable numbers (voxel size, origins and focal lengths are powers of two or small
integers), shared by the CPU suite (against the restatement) and the GPU suite (against the device): one voxel g = (0, 0, 0) of
size 1, the identity extrinsic, the camera K = (4, 4, 8, 4) of 17 x 9 pixels.  A corner (x, y, z) projects to u = (4 x + 8 z) / z,
v = (4 y + 4 z) / z; with y in {0, 1} and z in {1, 2} every v is 4, 6 or 8: inside the rows [0, 8]."""
import numpy as np

W, H, K4 = 17, 9, (4.0, 4.0, 8.0, 4.0)
EPS4 = np.spacing(4.0)                       # one ulp of the numbers in [4, 8)


def edge_scenes():
    """[(name, origin, float32 (H, W) image, mode, survives)]"""
    ones = np.ones((H, W), np.float32)
    two = np.full((H, W), 2.0, np.float32)
    above_two = np.full((H, W), np.nextafter(np.float32(2.0), np.float32(np.inf)), np.float32)
    return [
        # x in [-5, -4], z in [1, 2]: u = -12, -8, -2 and, for the corner (-4, ., 2), exactly 0
        ("u == 0 is within", (-5.0, 0.0, 1.0), ones, "silhouette", True),
        # the same voxel one ulp further left: that corner sits at x = -4 - ulp, u = -2 ulp < 0
        ("below u == 0 is not", (np.nextafter(-5.0, -np.inf), 0.0, 1.0), ones, "silhouette", False),
        # x in [4, 5]: u = 24, 28, 18 and, for the corner (4, ., 2), exactly 16 = W - 1
        ("u == W - 1 is within", (4.0, 0.0, 1.0), ones, "silhouette", True),
        # x = 4 + 2 ulp: 4 x + 16 = 32 + 8 ulp exactly, halved 16 + 4 ulp = nextafter(16)
        ("one ulp beyond u == W - 1 is not", (4.0 + 2.0 * EPS4, 0.0, 1.0), ones, "silhouette", False),
        # x in [0, 1]: the four corners at z = 2 project to the pixels u in {8, 10}, v in {4, 6}: d = 2 exactly, z == d
        ("z == d keeps", (0.0, 0.0, 1.0), two, "depth", True),
        ("z below nextafter(d) carves", (0.0, 0.0, 1.0), above_two, "depth", False),
    ]


# ---- the ring of test_tsdf_gpu.py and the clouds the grid constructors and voxel_down_sample are compared on --------------------------
RING_W, RING_H, RING_K4 = 80, 72, (63.0, 63.0, 40.0, 36.0)


def ring():
    """depth u16 (2, 4, n_px), rgb u8 (2, 4, n_px, 3), camera -> world poses (4, 4, 4) of synth.sensor_ring(4, 2, synth.small_xy(8))"""
    from kinectpy_amd.utils import synth
    _, depth, rgb, _, _ = synth.sensor_ring(4, 2, synth.small_xy(8))
    return depth, rgb, np.stack([synth.camera_pose(g, 4) for g in range(4)])


def unproject(depth, pose):
    """the pinhole unprojection of one u16 frame, moved by `pose` (camera -> anything): float32 (K, 3) points, their pixel numbers"""
    fx, fy, cx, cy = RING_K4
    pix = np.flatnonzero(depth > 0)
    z = depth[pix].astype(np.float64)
    x, y = ((pix % RING_W) - cx) / fx * z, ((pix // RING_W) - cy) / fy * z
    p = np.stack([x, y, z, np.ones_like(z)], 1) @ np.asarray(pose, np.float64).T
    return p[:, :3].astype(np.float32), pix


def ring_cloud(depth, rgb, poses):
    """the four clouds of one time frame stacked: points float32 (N, 3), colours float32 (N, 3) in [0, 1]"""
    parts = [unproject(depth[s], poses[s]) for s in range(len(poses))]
    return np.concatenate([p for p, _ in parts]), np.concatenate([rgb[s][pix].astype(np.float32) / np.float32(255.0) for s, (_, pix) in enumerate(parts)])


def cloud_cases():
    """[(name, points, colours, voxel size)]: the sizes at the ends of waves and blocks, identical points, one voxel for all, one
    voxel per point, the ring's cloud"""
    rng = np.random.default_rng(2024)
    cases = []
    for n in (1, 2, 63, 64, 65, 257):
        cases.append((f"normal{n}", (rng.normal(size=(n, 3)) * 100.0).astype(np.float32), rng.random((n, 3), dtype=np.float32), 60.0))
    p257, c257 = cases[-1][1], cases[-1][2]
    cases.append(("identical65", np.tile(np.float32([[12.5, -3.25, 700.125]]), (65, 1)), rng.random((65, 3), dtype=np.float32), 10.0))
    cases.append(("one_voxel", p257, c257, 5000.0))
    cases.append(("own_voxels", p257, c257, 0.01))
    depth, rgb, poses = ring()
    rp, rc = ring_cloud(depth[0], rgb[0], poses)
    cases.append(("ring", rp, rc, 160.0))
    return cases


def unit_normals(n, seed=7):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

"""Writes voxel_down_sample.npz next to this file: PointCloud.voxel_down_sample's points, colours and normals on the clouds of
tests/voxelgrid_scenes.cloud_cases(), as the library computed them BEFORE the grid steps moved into kpx_voxelsteps.h (run on an
MI355X with the parent commit's package first on the path: PYTHONPATH=<parent checkout> python tests/golden/make_voxel_down_sample_golden.py).
tests/test_voxelgrid_gpu.py compares the current library against it bit for bit.  Variants per cloud: points only ("p"), with colours
("pc": the one-pass batch form), with colours and normals ("pcn": the plain form)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                            # voxelgrid_scenes
sys.path.append(os.path.dirname(os.path.dirname(HERE)))             # this checkout's package, unless PYTHONPATH names another


def down_sample(pts, col, nrm, voxel):
    from kinectpy_amd import o3d
    pc = o3d.geometry.PointCloud()
    pc.points = o3d.utility.Vector3dVector(pts)
    if col is not None:
        pc.colors = o3d.utility.Vector3dVector(col)
    if nrm is not None:
        pc.normals = o3d.utility.Vector3dVector(nrm)
    out = pc.voxel_down_sample(voxel)
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(out._pts), host(out._col), host(out._nrm)


def variants(pts, col):
    import voxelgrid_scenes as S
    return (("p", None, None), ("pc", col, None), ("pcn", col, S.unit_normals(len(pts))))


def main(path):
    import voxelgrid_scenes as S
    arrays = {}
    for name, pts, col, voxel in S.cloud_cases():
        for tag, c, n in variants(pts, col):
            for kind, a in zip(("pts", "col", "nrm"), down_sample(pts, c, n, voxel)):
                if a is not None:
                    arrays[f"{name}.{tag}.{kind}"] = a
    np.savez_compressed(path, **arrays)
    print(len(arrays), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "voxel_down_sample.npz"))

"""Hand-built meshes whose soundness is known by construction, shared by the CPU and GPU suites of AC15's mesh checks."""
import functools

import numpy as np

import tsdf_mesh_ref as M

TET = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]          # outward for corners (0,0,0), (1,0,0), (0,1,0), (0,0,1)
TET_V = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, 3]], dtype=np.float32)
CUBE_V = np.array([[x, y, z] for x in (0, 2) for y in (0, 2) for z in (0, 2)], dtype=np.float32)
CUBE = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]


def bowtie():
    """two tetrahedra that share vertex 0 and nothing else"""
    v = np.concatenate([TET_V, -TET_V[1:]])
    other = np.array([0, 4, 5, 6])
    return v, np.concatenate([np.asarray(TET), other[np.asarray(TET)][:, [0, 2, 1]]]).astype(np.int32)


def fan(n, closed=True):
    """n triangles about apex 0 over a ring of n (closed) or n + 1 rim vertices"""
    a = np.arange(n + (0 if closed else 1)) * (2 * np.pi / n)
    v = np.concatenate([[[0, 0, 1]], np.stack([np.cos(a), np.sin(a), 0 * a], 1)]).astype(np.float32)
    k = np.arange(n)
    return v, np.stack([0 * k, 1 + k, 1 + (k + 1) % len(a)], 1).astype(np.int32)


def moebius(n=11):
    """a band of n triangles over n vertices whose edge (i, i + 1) joins triangles i - 1 and i: closed up with an odd n it has one side"""
    a = np.arange(n) * (2 * np.pi / n)
    v = np.stack([np.cos(a), np.sin(a), 0.3 * np.cos(a * n / 2)], 1).astype(np.float32)
    k = np.arange(n)
    t = np.stack([k, (k + 1) % n, (k + 2) % n], 1)
    t[1::2] = t[1::2][:, [0, 2, 1]]
    return v, t.astype(np.int32)


@functools.lru_cache(None)
def sphere():
    f, w = M.sphere_volume()
    v, _, t, _ = M.extract_triangle_mesh(f, w, None, 16, 1.0, (0.0, 0.0, 0.0))
    return v, t

"""The pinned statement of arithmetic contract AC12: UniformTSDFVolume.extract_triangle_mesh as a literal
serial marching cubes (triple loop, a dict from edge key to vertex, fp64 with every operation rounded separately), renumbered to
ascending (linear voxel index, axis), and the NumPy restatements of TriangleMesh's normals and surface area.  Python floats are
IEEE doubles and Python never fuses a multiply with an add, so the scalar code below IS the contract's arithmetic.

TRI_TABLE is the 256 x 16 case table of Bourke's `polygonise`; kinectpy_amd/csrc/kpx_mctables.h holds the second copy and
tests/test_tsdf_mesh_cpu.py holds both against each other and against the properties a correct table must have."""
import numpy as np

CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
# (dx, dy, dz, axis): the lower voxel of the edge relative to the cube, and the axis it runs along
EDGE_SHIFTS = ((0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 1, 1), (0, 1, 1, 0), (0, 0, 1, 1),
               (0, 0, 0, 2), (1, 0, 0, 2), (1, 1, 0, 2), (0, 1, 0, 2))
EDGE_CORNERS = ((0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7))

_ROWS = (
    (), (0, 8, 3), (0, 1, 9), (1, 8, 3, 9, 8, 1), (1, 2, 10), (0, 8, 3, 1, 2, 10), (9, 2, 10, 0, 2, 9), (2, 8, 3, 2, 10, 8, 10, 9, 8),
    (3, 11, 2), (0, 11, 2, 8, 11, 0), (1, 9, 0, 2, 3, 11), (1, 11, 2, 1, 9, 11, 9, 8, 11), (3, 10, 1, 11, 10, 3),
    (0, 10, 1, 0, 8, 10, 8, 11, 10), (3, 9, 0, 3, 11, 9, 11, 10, 9), (9, 8, 10, 10, 8, 11),
    (4, 7, 8), (4, 3, 0, 7, 3, 4), (0, 1, 9, 8, 4, 7), (4, 1, 9, 4, 7, 1, 7, 3, 1), (1, 2, 10, 8, 4, 7), (3, 4, 7, 3, 0, 4, 1, 2, 10),
    (9, 2, 10, 9, 0, 2, 8, 4, 7), (2, 10, 9, 2, 9, 7, 2, 7, 3, 7, 9, 4), (8, 4, 7, 3, 11, 2), (11, 4, 7, 11, 2, 4, 2, 0, 4),
    (9, 0, 1, 8, 4, 7, 2, 3, 11), (4, 7, 11, 9, 4, 11, 9, 11, 2, 9, 2, 1), (3, 10, 1, 3, 11, 10, 7, 8, 4),
    (1, 11, 10, 1, 4, 11, 1, 0, 4, 7, 11, 4), (4, 7, 8, 9, 0, 11, 9, 11, 10, 11, 0, 3), (4, 7, 11, 4, 11, 9, 9, 11, 10),
    (9, 5, 4), (9, 5, 4, 0, 8, 3), (0, 5, 4, 1, 5, 0), (8, 5, 4, 8, 3, 5, 3, 1, 5), (1, 2, 10, 9, 5, 4), (3, 0, 8, 1, 2, 10, 4, 9, 5),
    (5, 2, 10, 5, 4, 2, 4, 0, 2), (2, 10, 5, 3, 2, 5, 3, 5, 4, 3, 4, 8), (9, 5, 4, 2, 3, 11), (0, 11, 2, 0, 8, 11, 4, 9, 5),
    (0, 5, 4, 0, 1, 5, 2, 3, 11), (2, 1, 5, 2, 5, 8, 2, 8, 11, 4, 8, 5), (10, 3, 11, 10, 1, 3, 9, 5, 4),
    (4, 9, 5, 0, 8, 1, 8, 10, 1, 8, 11, 10), (5, 4, 0, 5, 0, 11, 5, 11, 10, 11, 0, 3), (5, 4, 8, 5, 8, 10, 10, 8, 11),
    (9, 7, 8, 5, 7, 9), (9, 3, 0, 9, 5, 3, 5, 7, 3), (0, 7, 8, 0, 1, 7, 1, 5, 7), (1, 5, 3, 3, 5, 7), (9, 7, 8, 9, 5, 7, 10, 1, 2),
    (10, 1, 2, 9, 5, 0, 5, 3, 0, 5, 7, 3), (8, 0, 2, 8, 2, 5, 8, 5, 7, 10, 5, 2), (2, 10, 5, 2, 5, 3, 3, 5, 7),
    (7, 9, 5, 7, 8, 9, 3, 11, 2), (9, 5, 7, 9, 7, 2, 9, 2, 0, 2, 7, 11), (2, 3, 11, 0, 1, 8, 1, 7, 8, 1, 5, 7),
    (11, 2, 1, 11, 1, 7, 7, 1, 5), (9, 5, 8, 8, 5, 7, 10, 1, 3, 10, 3, 11), (5, 7, 0, 5, 0, 9, 7, 11, 0, 1, 0, 10, 11, 10, 0),
    (11, 10, 0, 11, 0, 3, 10, 5, 0, 8, 0, 7, 5, 7, 0), (11, 10, 5, 7, 11, 5),
    (10, 6, 5), (0, 8, 3, 5, 10, 6), (9, 0, 1, 5, 10, 6), (1, 8, 3, 1, 9, 8, 5, 10, 6), (1, 6, 5, 2, 6, 1), (1, 6, 5, 1, 2, 6, 3, 0, 8),
    (9, 6, 5, 9, 0, 6, 0, 2, 6), (5, 9, 8, 5, 8, 2, 5, 2, 6, 3, 2, 8), (2, 3, 11, 10, 6, 5), (11, 0, 8, 11, 2, 0, 10, 6, 5),
    (0, 1, 9, 2, 3, 11, 5, 10, 6), (5, 10, 6, 1, 9, 2, 9, 11, 2, 9, 8, 11), (6, 3, 11, 6, 5, 3, 5, 1, 3),
    (0, 8, 11, 0, 11, 5, 0, 5, 1, 5, 11, 6), (3, 11, 6, 0, 3, 6, 0, 6, 5, 0, 5, 9), (6, 5, 9, 6, 9, 11, 11, 9, 8),
    (5, 10, 6, 4, 7, 8), (4, 3, 0, 4, 7, 3, 6, 5, 10), (1, 9, 0, 5, 10, 6, 8, 4, 7), (10, 6, 5, 1, 9, 7, 1, 7, 3, 7, 9, 4),
    (6, 1, 2, 6, 5, 1, 4, 7, 8), (1, 2, 5, 5, 2, 6, 3, 0, 4, 3, 4, 7), (8, 4, 7, 9, 0, 5, 0, 6, 5, 0, 2, 6),
    (7, 3, 9, 7, 9, 4, 3, 2, 9, 5, 9, 6, 2, 6, 9), (3, 11, 2, 7, 8, 4, 10, 6, 5), (5, 10, 6, 4, 7, 2, 4, 2, 0, 2, 7, 11),
    (0, 1, 9, 4, 7, 8, 2, 3, 11, 5, 10, 6), (9, 2, 1, 9, 11, 2, 9, 4, 11, 7, 11, 4, 5, 10, 6), (8, 4, 7, 3, 11, 5, 3, 5, 1, 5, 11, 6),
    (5, 1, 11, 5, 11, 6, 1, 0, 11, 7, 11, 4, 0, 4, 11), (0, 5, 9, 0, 6, 5, 0, 3, 6, 11, 6, 3, 8, 4, 7), (6, 5, 9, 6, 9, 11, 4, 7, 9, 7, 11, 9),
    (10, 4, 9, 6, 4, 10), (4, 10, 6, 4, 9, 10, 0, 8, 3), (10, 0, 1, 10, 6, 0, 6, 4, 0), (8, 3, 1, 8, 1, 6, 8, 6, 4, 6, 1, 10),
    (1, 4, 9, 1, 2, 4, 2, 6, 4), (3, 0, 8, 1, 2, 9, 2, 4, 9, 2, 6, 4), (0, 2, 4, 4, 2, 6), (8, 3, 2, 8, 2, 4, 4, 2, 6),
    (10, 4, 9, 10, 6, 4, 11, 2, 3), (0, 8, 2, 2, 8, 11, 4, 9, 10, 4, 10, 6), (3, 11, 2, 0, 1, 6, 0, 6, 4, 6, 1, 10),
    (6, 4, 1, 6, 1, 10, 4, 8, 1, 2, 1, 11, 8, 11, 1), (9, 6, 4, 9, 3, 6, 9, 1, 3, 11, 6, 3), (8, 11, 1, 8, 1, 0, 11, 6, 1, 9, 1, 4, 6, 4, 1),
    (3, 11, 6, 3, 6, 0, 0, 6, 4), (6, 4, 8, 11, 6, 8),
    (7, 10, 6, 7, 8, 10, 8, 9, 10), (0, 7, 3, 0, 10, 7, 0, 9, 10, 6, 7, 10), (10, 6, 7, 1, 10, 7, 1, 7, 8, 1, 8, 0),
    (10, 6, 7, 10, 7, 1, 1, 7, 3), (1, 2, 6, 1, 6, 8, 1, 8, 9, 8, 6, 7), (2, 6, 9, 2, 9, 1, 6, 7, 9, 0, 9, 3, 7, 3, 9),
    (7, 8, 0, 7, 0, 6, 6, 0, 2), (7, 3, 2, 6, 7, 2), (2, 3, 11, 10, 6, 8, 10, 8, 9, 8, 6, 7), (2, 0, 7, 2, 7, 11, 0, 9, 7, 6, 7, 10, 9, 10, 7),
    (1, 8, 0, 1, 7, 8, 1, 10, 7, 6, 7, 10, 2, 3, 11), (11, 2, 1, 11, 1, 7, 10, 6, 1, 6, 7, 1), (8, 9, 6, 8, 6, 7, 9, 1, 6, 11, 6, 3, 1, 3, 6),
    (0, 9, 1, 11, 6, 7), (7, 8, 0, 7, 0, 6, 3, 11, 0, 11, 6, 0), (7, 11, 6),
    (7, 6, 11), (3, 0, 8, 11, 7, 6), (0, 1, 9, 11, 7, 6), (8, 1, 9, 8, 3, 1, 11, 7, 6), (10, 1, 2, 6, 11, 7), (1, 2, 10, 3, 0, 8, 6, 11, 7),
    (2, 9, 0, 2, 10, 9, 6, 11, 7), (6, 11, 7, 2, 10, 3, 10, 8, 3, 10, 9, 8), (7, 2, 3, 6, 2, 7), (7, 0, 8, 7, 6, 0, 6, 2, 0),
    (2, 7, 6, 2, 3, 7, 0, 1, 9), (1, 6, 2, 1, 8, 6, 1, 9, 8, 8, 7, 6), (10, 7, 6, 10, 1, 7, 1, 3, 7), (10, 7, 6, 1, 7, 10, 1, 8, 7, 1, 0, 8),
    (0, 3, 7, 0, 7, 10, 0, 10, 9, 6, 10, 7), (7, 6, 10, 7, 10, 8, 8, 10, 9),
    (6, 8, 4, 11, 8, 6), (3, 6, 11, 3, 0, 6, 0, 4, 6), (8, 6, 11, 8, 4, 6, 9, 0, 1), (9, 4, 6, 9, 6, 3, 9, 3, 1, 11, 3, 6),
    (6, 8, 4, 6, 11, 8, 2, 10, 1), (1, 2, 10, 3, 0, 11, 0, 6, 11, 0, 4, 6), (4, 11, 8, 4, 6, 11, 0, 2, 9, 2, 10, 9),
    (10, 9, 3, 10, 3, 2, 9, 4, 3, 11, 3, 6, 4, 6, 3), (8, 2, 3, 8, 4, 2, 4, 6, 2), (0, 4, 2, 4, 6, 2), (1, 9, 0, 2, 3, 4, 2, 4, 6, 4, 3, 8),
    (1, 9, 4, 1, 4, 2, 2, 4, 6), (8, 1, 3, 8, 6, 1, 8, 4, 6, 6, 10, 1), (10, 1, 0, 10, 0, 6, 6, 0, 4),
    (4, 6, 3, 4, 3, 8, 6, 10, 3, 0, 3, 9, 10, 9, 3), (10, 9, 4, 6, 10, 4),
    (4, 9, 5, 7, 6, 11), (0, 8, 3, 4, 9, 5, 11, 7, 6), (5, 0, 1, 5, 4, 0, 7, 6, 11), (11, 7, 6, 8, 3, 4, 3, 5, 4, 3, 1, 5),
    (9, 5, 4, 10, 1, 2, 7, 6, 11), (6, 11, 7, 1, 2, 10, 0, 8, 3, 4, 9, 5), (7, 6, 11, 5, 4, 10, 4, 2, 10, 4, 0, 2),
    (3, 4, 8, 3, 5, 4, 3, 2, 5, 10, 5, 2, 11, 7, 6), (7, 2, 3, 7, 6, 2, 5, 4, 9), (9, 5, 4, 0, 8, 6, 0, 6, 2, 6, 8, 7),
    (3, 6, 2, 3, 7, 6, 1, 5, 0, 5, 4, 0), (6, 2, 8, 6, 8, 7, 2, 1, 8, 4, 8, 5, 1, 5, 8), (9, 5, 4, 10, 1, 6, 1, 7, 6, 1, 3, 7),
    (1, 6, 10, 1, 7, 6, 1, 0, 7, 8, 7, 0, 9, 5, 4), (4, 0, 10, 4, 10, 5, 0, 3, 10, 6, 10, 7, 3, 7, 10), (7, 6, 10, 7, 10, 8, 5, 4, 10, 4, 8, 10),
    (6, 9, 5, 6, 11, 9, 11, 8, 9), (3, 6, 11, 0, 6, 3, 0, 5, 6, 0, 9, 5), (0, 11, 8, 0, 5, 11, 0, 1, 5, 5, 6, 11), (6, 11, 3, 6, 3, 5, 5, 3, 1),
    (1, 2, 10, 9, 5, 11, 9, 11, 8, 11, 5, 6), (0, 11, 3, 0, 6, 11, 0, 9, 6, 5, 6, 9, 1, 2, 10), (11, 8, 5, 11, 5, 6, 8, 0, 5, 10, 5, 2, 0, 2, 5),
    (6, 11, 3, 6, 3, 5, 2, 10, 3, 10, 5, 3), (5, 8, 9, 5, 2, 8, 5, 6, 2, 3, 8, 2), (9, 5, 6, 9, 6, 0, 0, 6, 2),
    (1, 5, 8, 1, 8, 0, 5, 6, 8, 3, 8, 2, 6, 2, 8), (1, 5, 6, 2, 1, 6), (1, 3, 6, 1, 6, 10, 3, 8, 6, 5, 6, 9, 8, 9, 6),
    (10, 1, 0, 10, 0, 6, 9, 5, 0, 5, 6, 0), (0, 3, 8, 5, 6, 10), (10, 5, 6),
    (11, 5, 10, 7, 5, 11), (11, 5, 10, 11, 7, 5, 8, 3, 0), (5, 11, 7, 5, 10, 11, 1, 9, 0), (10, 7, 5, 10, 11, 7, 9, 8, 1, 8, 3, 1),
    (11, 1, 2, 11, 7, 1, 7, 5, 1), (0, 8, 3, 1, 2, 7, 1, 7, 5, 7, 2, 11), (9, 7, 5, 9, 2, 7, 9, 0, 2, 2, 11, 7),
    (7, 5, 2, 7, 2, 11, 5, 9, 2, 3, 2, 8, 9, 8, 2), (2, 5, 10, 2, 3, 5, 3, 7, 5), (8, 2, 0, 8, 5, 2, 8, 7, 5, 10, 2, 5),
    (9, 0, 1, 5, 10, 3, 5, 3, 7, 3, 10, 2), (9, 8, 2, 9, 2, 1, 8, 7, 2, 10, 2, 5, 7, 5, 2), (1, 3, 5, 3, 7, 5), (0, 8, 7, 0, 7, 1, 1, 7, 5),
    (9, 0, 3, 9, 3, 5, 5, 3, 7), (9, 8, 7, 5, 9, 7),
    (5, 8, 4, 5, 10, 8, 10, 11, 8), (5, 0, 4, 5, 11, 0, 5, 10, 11, 11, 3, 0), (0, 1, 9, 8, 4, 10, 8, 10, 11, 10, 4, 5),
    (10, 11, 4, 10, 4, 5, 11, 3, 4, 9, 4, 1, 3, 1, 4), (2, 5, 1, 2, 8, 5, 2, 11, 8, 4, 5, 8), (0, 4, 11, 0, 11, 3, 4, 5, 11, 2, 11, 1, 5, 1, 11),
    (0, 2, 5, 0, 5, 9, 2, 11, 5, 4, 5, 8, 11, 8, 5), (9, 4, 5, 2, 11, 3), (2, 5, 10, 3, 5, 2, 3, 4, 5, 3, 8, 4), (5, 10, 2, 5, 2, 4, 4, 2, 0),
    (3, 10, 2, 3, 5, 10, 3, 8, 5, 4, 5, 8, 0, 1, 9), (5, 10, 2, 5, 2, 4, 1, 9, 2, 9, 4, 2), (8, 4, 5, 8, 5, 3, 3, 5, 1), (0, 4, 5, 1, 0, 5),
    (8, 4, 5, 8, 5, 3, 9, 0, 5, 0, 3, 5), (9, 4, 5),
    (4, 11, 7, 4, 9, 11, 9, 10, 11), (0, 8, 3, 4, 9, 7, 9, 11, 7, 9, 10, 11), (1, 10, 11, 1, 11, 4, 1, 4, 0, 7, 4, 11),
    (3, 1, 4, 3, 4, 8, 1, 10, 4, 7, 4, 11, 10, 11, 4), (4, 11, 7, 9, 11, 4, 9, 2, 11, 9, 1, 2), (9, 7, 4, 9, 11, 7, 9, 1, 11, 2, 11, 1, 0, 8, 3),
    (11, 7, 4, 11, 4, 2, 2, 4, 0), (11, 7, 4, 11, 4, 2, 8, 3, 4, 3, 2, 4), (2, 9, 10, 2, 7, 9, 2, 3, 7, 7, 4, 9),
    (9, 10, 7, 9, 7, 4, 10, 2, 7, 8, 7, 0, 2, 0, 7), (3, 7, 10, 3, 10, 2, 7, 4, 10, 1, 10, 0, 4, 0, 10), (1, 10, 2, 8, 7, 4),
    (4, 9, 1, 4, 1, 7, 7, 1, 3), (4, 9, 1, 4, 1, 7, 0, 8, 1, 8, 7, 1), (4, 0, 3, 7, 4, 3), (4, 8, 7),
    (9, 10, 8, 10, 11, 8), (3, 0, 9, 3, 9, 11, 11, 9, 10), (0, 1, 10, 0, 10, 8, 8, 10, 11), (3, 1, 10, 11, 3, 10), (1, 2, 11, 1, 11, 9, 9, 11, 8),
    (3, 0, 9, 3, 9, 11, 1, 2, 9, 2, 11, 9), (0, 2, 11, 8, 0, 11), (3, 2, 11), (2, 3, 8, 2, 8, 10, 10, 8, 9), (9, 10, 2, 0, 9, 2),
    (2, 3, 8, 2, 8, 10, 0, 1, 8, 1, 10, 8), (1, 10, 2), (1, 3, 8, 9, 1, 8), (0, 9, 1), (0, 3, 8), (),
)
assert len(_ROWS) == 256
TRI_TABLE = np.full((256, 16), -1, dtype=np.int8)
for _c, _r in enumerate(_ROWS):
    TRI_TABLE[_c, :len(_r)] = _r


def row(code):
    """the edge indices of a code's row up to its first -1"""
    r = TRI_TABLE[code].tolist()
    return r[:r.index(-1)]


def edge_mask(code):
    """bit i: the two corners of edge i have different signs under `code` (computed, never typed)"""
    return sum(1 << i for i, (a, b) in enumerate(EDGE_CORNERS) if ((code >> a) & 1) != ((code >> b) & 1))


def cube_codes(tsdf, weight, res):
    """(res - 1)^3 int array: the code of every cube, 0 for an inactive one (a corner of weight 0)"""
    n = max(res - 1, 0)
    f = np.asarray(tsdf, dtype=np.float32).reshape(res, res, res)
    w = np.asarray(weight, dtype=np.float32).reshape(res, res, res)
    code = np.zeros((n, n, n), dtype=np.int64)
    active = np.ones((n, n, n), dtype=bool)
    for i, (dx, dy, dz) in enumerate(CORNERS):
        fs, ws = f[dx:dx + n, dy:dy + n, dz:dz + n], w[dx:dx + n, dy:dy + n, dz:dz + n]
        code |= (fs < np.float32(0.0)).astype(np.int64) << i
        active &= ws != np.float32(0.0)
    return np.where(active, code, 0)


def extract_triangle_mesh(tsdf, weight, color, res, voxel_length, origin):
    """AC12.  tsdf, weight: float32 (res^3,); color: float32 (res^3, 3) or None.  -> (vertices float32 (V, 3), colours float32 (V, 3)
    or None, triangles int32 (T, 3), keys int64 (V, 2) = (linear index of the lower voxel, axis) per vertex), vertices ascending in
    their key."""
    f = np.asarray(tsdf, dtype=np.float32).reshape(-1)
    vl = float(voxel_length)
    org = [float(o) for o in np.asarray(origin, dtype=np.float64).reshape(3)]
    codes = cube_codes(f, weight, res)
    first = {}                     # edge key (L, axis) -> serial vertex number (first encounter)
    verts, cols, keys, tris = [], [], [], []
    for x in range(res - 1):
        for y in range(res - 1):
            for z in range(res - 1):
                code = int(codes[x, y, z])
                if code == 0 or code == 255:
                    continue
                mask = edge_mask(code)
                idx = [-1] * 12
                for e in range(12):
                    if not (mask >> e) & 1:
                        continue
                    dx, dy, dz, a = EDGE_SHIFTS[e]
                    v = [x + dx, y + dy, z + dz]
                    L0 = (v[0] * res + v[1]) * res + v[2]
                    key = (L0, a)
                    if key not in first:
                        L1 = L0 + (res * res, res, 1)[a]
                        f0, f1 = abs(float(f[L0])), abs(float(f[L1]))
                        p = [(v[0] + 0.5) * vl, (v[1] + 0.5) * vl, (v[2] + 0.5) * vl]
                        p[a] = p[a] + (f0 * vl) / (f0 + f1)
                        first[key] = len(verts)
                        verts.append([p[0] + org[0], p[1] + org[1], p[2] + org[2]])
                        keys.append(key)
                        if color is not None:
                            c0, c1 = color[L0], color[L1]
                            cols.append([(f1 * (float(c0[k]) / 255.0) + f0 * (float(c1[k]) / 255.0)) / (f0 + f1) for k in range(3)])
                    idx[e] = first[key]
                r = row(code)
                for t in range(0, len(r), 3):
                    tris.append([idx[r[t]], idx[r[t + 2]], idx[r[t + 1]]])
    V = len(verts)
    order = sorted(range(V), key=lambda i: keys[i])
    new = np.empty(V, dtype=np.int64)
    new[order] = np.arange(V)
    with np.errstate(over="ignore", invalid="ignore"):
        vout = np.asarray(verts, dtype=np.float64).reshape(-1, 3)[order].astype(np.float32)
        cout = np.asarray(cols, dtype=np.float64).reshape(-1, 3)[order].astype(np.float32) if color is not None else None
    tout = new[np.asarray(tris, dtype=np.int64).reshape(-1, 3)].astype(np.int32)
    kout = np.asarray(keys, dtype=np.int64).reshape(-1, 2)[order]
    return vout, cout, tout, kout


# ---- normals and area of any TriangleMesh -----------------------------------------------------------------------------------------
def _cross(vertices, triangles):
    """(T, 3) float64: (v1 - v0) x (v2 - v0) from the float32 vertices, every component a b - c d"""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e1, e2 = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                         e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).reshape(-1, 3)


def _norm(n):
    with np.errstate(all="ignore"):
        return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def _normalize(n):
    """n / |n|, a zero vector -> (0, 0, 1) (Open3D's NormalizeNormals)"""
    ln = _norm(n)
    with np.errstate(all="ignore"):
        out = n / ln[:, None]
    out[ln == 0.0] = (0.0, 0.0, 1.0)
    return out


def _f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return a.astype(np.float32)


def triangle_normals(vertices, triangles, normalized=True):
    n = _cross(vertices, triangles)
    return _f32(_normalize(n) if normalized else n)


def vertex_normals(vertices, triangles, normalized=True):
    """per vertex the sum from 0 of the unnormalised triangle normals in ascending triangle index (once per corner occurrence).
    Round r adds every vertex's r-th occurrence: within a round no vertex appears twice, so each vertex sees a serial sum."""
    n = _cross(vertices, triangles)
    t = np.asarray(triangles).reshape(-1)
    V = len(np.asarray(vertices).reshape(-1, 3))
    acc = np.zeros((V, 3), dtype=np.float64)
    order = np.argsort(t, kind="stable")                   # pairs grouped by vertex, ascending pair (= triangle) index inside
    vs = t[order]
    start = np.searchsorted(vs, np.arange(V), side="left")
    count = np.searchsorted(vs, np.arange(V), side="right") - start
    with np.errstate(all="ignore"):
        for r in range(int(count.max()) if V and len(t) else 0):
            who = np.flatnonzero(count > r)
            acc[who] = acc[who] + n[order[start[who] + r] // 3]
    return _f32(_normalize(acc) if normalized else acc)


def surface_area(vertices, triangles):
    """sum over the triangles, ascending, of half the norm of the cross product (fp64, serial)"""
    half = _norm(_cross(vertices, triangles)) * 0.5
    s = 0.0
    for a in half.tolist():
        s = s + a
    return s


def sphere_volume(res=16, radius=5.3, centre=(7.3, 8.1, 6.6)):
    """signed distance (in voxels, clipped to [-1, 1]) of an off-centre sphere, negative inside, every weight 1"""
    g = np.arange(res, dtype=np.float64) + 0.5
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return np.clip(d, -1.0, 1.0).astype(np.float32).reshape(-1), np.ones(res ** 3, dtype=np.float32)

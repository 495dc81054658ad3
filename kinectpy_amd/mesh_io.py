"""PLY reader / writer for triangle meshes (o3d.io.write_triangle_mesh / read_triangle_mesh).  Host-side file I/O only (out of the
hot path); the core functions take and return NumPy arrays.

What write_triangle_mesh emits, the layout Open3D's PLY writer uses for a legacy TriangleMesh [O3D, recalled]:

    ply
    format binary_little_endian 1.0          (or: format ascii 1.0)
    comment Created by kinectpy_amd
    element vertex <V>
    property double x / y / z
    property double nx / ny / nz             when the mesh has vertex normals
    property uchar red / green / blue        when it has vertex colours: (uint8)clip(round(c 255), 0, 255)
    element face <T>
    property list uchar uint vertex_indices
    end_header

The reader accepts those files and the usual variations: float coordinates, other integer widths in the face list, extra vertex
properties (skipped), faces with more than three corners (split into a fan), `vertex_index` as the list's name."""
import os

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def pack_colors(colors):
    """(n, 3) colours in [0, 1] -> uint8 (n, 3)"""
    return np.clip(np.round(np.asarray(colors, dtype=np.float64).reshape(-1, 3) * 255.0), 0, 255).astype(np.uint8)


def encode_ply(vertices, triangles, normals=None, colors=None, write_ascii=False) -> bytes:
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise RuntimeError(f"write_triangle_mesh: triangle index out of range [0, {len(v)})")
    cols, props = [("x", v[:, 0]), ("y", v[:, 1]), ("z", v[:, 2])], ["property double x", "property double y", "property double z"]
    if normals is not None:
        n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        if len(n) != len(v):
            raise RuntimeError("write_triangle_mesh: one normal per vertex")
        cols += [("nx", n[:, 0]), ("ny", n[:, 1]), ("nz", n[:, 2])]
        props += ["property double nx", "property double ny", "property double nz"]
    if colors is not None:
        c = pack_colors(colors)
        if len(c) != len(v):
            raise RuntimeError("write_triangle_mesh: one colour per vertex")
        cols += [("red", c[:, 0]), ("green", c[:, 1]), ("blue", c[:, 2])]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    head = "\n".join(["ply", f"format {'ascii' if write_ascii else 'binary_little_endian'} 1.0", "comment Created by kinectpy_amd",
                      f"element vertex {len(v)}"] + props + [f"element face {len(t)}", "property list uchar uint vertex_indices", "end_header"]) + "\n"
    if write_ascii:
        # repr of a Python float is the shortest text that reads back to the same double
        rows = [" ".join(repr(float(a[i])) if a.dtype == np.float64 else str(int(a[i])) for _, a in cols) for i in range(len(v))]
        rows += [f"3 {int(a)} {int(b)} {int(c)}" for a, b, c in t]
        return (head + "".join(r + "\n" for r in rows)).encode("ascii")
    rec = np.empty(len(v), dtype=[(name, "<f8" if a.dtype == np.float64 else "u1") for name, a in cols])
    for name, a in cols:
        rec[name] = a
    face = np.empty(len(t), dtype=[("n", "u1"), ("i", "<u4", (3,))])
    face["n"] = 3
    face["i"] = t
    return head.encode("ascii") + rec.tobytes() + face.tobytes()


def decode_ply(raw: bytes):
    """-> (vertices (V, 3) float64, triangles (T, 3) int32, normals (V, 3) float64 | None, colours (V, 3) float64 in [0, 1] | None)"""
    if not raw.startswith(b"ply"):
        raise RuntimeError("read_triangle_mesh: not a PLY file")
    end = raw.index(b"end_header")
    off = raw.index(b"\n", end) + 1
    fmt, elements = None, []                         # elements: [name, count, [(kind, name, types...)]]
    for line in raw[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w or w[0] in ("ply", "comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property":
            if w[1] == "list":
                elements[-1][2].append(("list", w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
            else:
                elements[-1][2].append(("scalar", w[2], _PLY_TYPES[w[1]]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise RuntimeError(f"read_triangle_mesh: unsupported PLY format {fmt}")
    order = ">" if fmt == "binary_big_endian" else "<"
    tokens = raw[off:].split() if fmt == "ascii" else None
    pos = 0
    vert, faces = {}, []
    for name, count, props in elements:
        scalar_only = all(p[0] == "scalar" for p in props)
        if fmt != "ascii" and scalar_only:
            dt = np.dtype([(p[1], order + p[2]) for p in props])
            rec = np.frombuffer(raw, dtype=dt, count=count, offset=off)
            off += dt.itemsize * count
            if name == "vertex":
                vert = {p[1]: rec[p[1]] for p in props}
            continue
        if fmt == "ascii" and scalar_only:
            block = tokens[pos:pos + count * len(props)]
            pos += count * len(props)
            if name == "vertex":
                for k, p in enumerate(props):
                    vals = block[k::len(props)]
                    vert[p[1]] = np.array([float(x) for x in vals], dtype=np.float64).astype(p[2]) if p[2][0] == "f" else \
                        np.array([int(x) for x in vals], dtype=np.int64).astype(p[2])
            continue
        # an element with lists: the faces (other list elements are walked over)
        fast = fmt != "ascii" and len(props) == 1 and count > 0
        if fast:                                     # every face a triangle: one strided read
            cdt, idt = np.dtype(order + props[0][2]), np.dtype(order + props[0][3])
            dt = np.dtype([("n", cdt), ("i", idt, (3,))])
            if off + dt.itemsize * count <= len(raw):
                rec = np.frombuffer(raw, dtype=dt, count=count, offset=off)
                if np.all(rec["n"] == 3):            # (record k + 1 starts where a 3-corner record k ends: the view is aligned)
                    if name == "face":
                        faces.append(rec["i"].astype(np.int64))
                    off += dt.itemsize * count
                    continue
        for _ in range(count):
            for p in props:
                if p[0] == "scalar":
                    if fmt == "ascii":
                        pos += 1
                    else:
                        off += np.dtype(p[2]).itemsize
                    continue
                if fmt == "ascii":
                    n = int(tokens[pos])
                    idx = [int(x) for x in tokens[pos + 1:pos + 1 + n]]
                    pos += 1 + n
                else:
                    n = int(np.frombuffer(raw, dtype=order + p[2], count=1, offset=off)[0])
                    off += np.dtype(p[2]).itemsize
                    idx = np.frombuffer(raw, dtype=order + p[3], count=n, offset=off).tolist()
                    off += np.dtype(p[3]).itemsize * n
                if name == "face" and p[1] in ("vertex_indices", "vertex_index") and n >= 3:
                    faces.append(np.array([[idx[0], idx[k], idx[k + 1]] for k in range(1, n - 1)], dtype=np.int64))
    for need in ("x", "y", "z"):
        if need not in vert:
            if any(e[0] == "vertex" and e[1] == 0 for e in elements):
                vert = {k: np.zeros(0) for k in ("x", "y", "z")}
                break
            raise RuntimeError("read_triangle_mesh: the file has no x / y / z properties")
    v = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float64).reshape(-1, 3)
    n = np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).astype(np.float64) if all(k in vert for k in ("nx", "ny", "nz")) else None
    c = np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.float64) / 255.0 if all(k in vert for k in ("red", "green", "blue")) else None
    t = (np.concatenate(faces) if faces else np.zeros((0, 3), np.int64)).astype(np.int32).reshape(-1, 3)
    return v, t, n, c


def _ply_only(who, filename):
    if os.path.splitext(str(filename))[1].lower() != ".ply":
        raise NotImplementedError(f"{who}: only PLY files are built, not {os.path.splitext(str(filename))[1] or filename!r}")


def write_triangle_mesh(filename, mesh, write_ascii=False):
    """o3d.io.write_triangle_mesh(filename, mesh, write_ascii=False): vertices, vertex normals, vertex colours and triangles as PLY"""
    _ply_only("write_triangle_mesh", filename)
    raw = encode_ply(np.asarray(mesh.vertices), np.asarray(mesh.triangles), np.asarray(mesh.vertex_normals) if mesh.has_vertex_normals() else None,
                     np.asarray(mesh.vertex_colors) if mesh.has_vertex_colors() else None, write_ascii)
    with open(filename, "wb") as f:
        f.write(raw)
    return True


def read_triangle_mesh(filename):
    """o3d.io.read_triangle_mesh(filename) -> TriangleMesh"""
    _ply_only("read_triangle_mesh", filename)
    from .geometry import TriangleMesh
    with open(filename, "rb") as f:
        v, t, n, c = decode_ply(f.read())
    mesh = TriangleMesh(v, t)
    if n is not None:
        mesh.vertex_normals = n
    if c is not None:
        mesh.vertex_colors = c
    return mesh

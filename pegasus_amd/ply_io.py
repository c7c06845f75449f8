"""Minimal PLY reader/writer for 3DGS point clouds (the data format on the input side of the render path:
/root/reference/src/gs/gaussian_model.py:231-288 reads it with ``plyfile``, which is not available here).
Supports ``binary_little_endian`` and ``ascii`` vertex elements with scalar properties."""
from __future__ import annotations

from pathlib import Path

import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}


def read_ply_vertices(path) -> np.ndarray:
    """Returns the 'vertex' element as a numpy structured array."""
    data = Path(path).read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    if header[0].strip() != "ply":
        raise ValueError("not a PLY file")
    fmt = None
    elements = []   # (name, count, [(prop, dtype)])
    for line in header[1:]:
        tok = line.split()
        if not tok or tok[0] == "comment":
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":
                raise ValueError("list properties are not supported")
            elements[-1][2].append((tok[2], _TYPES[tok[1]]))
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"unsupported PLY format {fmt}")
    off = end
    for name, count, props in elements:
        dt = np.dtype([(p, "<" + t) for p, t in props])
        if fmt == "binary_little_endian":
            arr = np.frombuffer(data, dtype=dt, count=count, offset=off)
            off += count * dt.itemsize
        else:
            text = data[off:].decode("ascii").split("\n")
            rows = [tuple(float(x) for x in text[i].split()) for i in range(count)]
            arr = np.array(rows, dtype=dt) if count else np.zeros(0, dtype=dt)
            off += sum(len(text[i]) + 1 for i in range(count))
        if name == "vertex":
            return arr
    raise ValueError("no vertex element")


def write_ply_vertices(path, columns: dict):
    """columns: ordered {property name: 1-D array}; written as float32 binary_little_endian."""
    names = list(columns)
    n = len(columns[names[0]]) if names else 0
    dt = np.dtype([(k, "<f4") for k in names])
    arr = np.empty(n, dtype=dt)
    for k in names:
        arr[k] = np.asarray(columns[k], dtype=np.float32)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    header += "".join(f"property float {k}\n" for k in names) + "end_header\n"
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(arr.tobytes())


def write_ply_mesh(path, vertices, faces):
    """Binary little-endian PLY of a triangle mesh: vertex (float x, y, z) and face (list uchar int vertex_indices)."""
    v = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype="<i4").reshape(-1, 3)
    rows = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    rows["n"] = 3
    rows["idx"] = f
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
              "property float z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rows.tobytes())


def read_ply_mesh(path):
    """(vertices float32 [V,3], faces int32 [F,3]) of a binary PLY written by write_ply_mesh."""
    data = Path(path).read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").split("\n")
    counts = {l.split()[1]: int(l.split()[2]) for l in header if l.startswith("element ")}
    if "format binary_little_endian 1.0" not in header or "property list uchar int vertex_indices" not in header:
        raise ValueError("not a binary triangle-mesh PLY of write_ply_mesh's layout")
    nv, nf = counts["vertex"], counts.get("face", 0)
    v = np.frombuffer(data, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3)
    rows = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]), count=nf, offset=end + 12 * nv)
    if nf and not (rows["n"] == 3).all():
        raise ValueError("faces must be triangles")
    return v.astype(np.float32), rows["idx"].astype(np.int32)

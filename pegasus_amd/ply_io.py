"""Minimal PLY reader/writer for 3DGS point clouds (the data format on the input side of the render path:
/root/reference/src/gs/gaussian_model.py:231-288 reads it with ``plyfile``, which is not available here).
Supports ``binary_little_endian`` and ``ascii`` vertex elements with scalar properties.  Triangle meshes: ``write_ply_mesh`` /
``read_ply_mesh`` for the layout the project writes, ``read_ply_model`` / ``write_ply_model`` for BOP object model files (normals,
colours; texture coordinates and the texture file's name on request) as the toolkit's ``inout.load_ply`` / ``save_ply`` read and
write them."""
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


# ---- BOP object models ------------------------------------------------------------------------------------------------
_INDEX_TYPES = ("int", "uint", "int32", "uint32")
_COUNT_TYPES = ("uchar", "uint8")


def _model_header(data: bytes):
    """(format, [(element, count, [property tokens])], offset of the body) of a PLY file."""
    at = data.find(b"end_header")
    if not data.startswith(b"ply") or at < 0:
        raise ValueError("not a PLY file")
    end = data.find(b"\n", at)
    if end < 0:
        raise ValueError("PLY header is not terminated")
    fmt, elements = None, []
    for line in data[:at].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] == "comment":
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property" and elements:
            elements[-1][2].append(tok[1:])
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"unsupported PLY format {fmt}")
    return fmt, elements, end + 1


_UV_TYPES = ("float", "float32")


def _texture_file(data: bytes):
    """The name in the header line ``comment TextureFile <name>`` (the last one, its last word, as the toolkit reads it), or None."""
    name = None
    for line in data[:data.find(b"end_header")].decode("ascii", "replace").splitlines():
        if line.startswith("comment TextureFile") and len(line.split()) > 2:
            name = line.split()[-1]
    return name


def read_ply_model(path, texture: bool = False) -> dict:
    """A BOP object model as the toolkit's inout.load_ply returns it: {'pts' float64 [V,3], 'faces' int64 [F,3]} plus
    'normals' float64 [V,3] (nx ny nz) and 'colors' [V,3] (red green blue, as stored: uint8 or float) when present.  ASCII and
    binary little-endian; any scalar vertex properties in any order (texture_u / texture_v and unknown ones are skipped); the
    face list is ``list uchar|uint8 int|uint|int32|uint32 vertex_indices|vertex_index``; other elements and other face
    properties are not supported in front of or between them.  Faces that are not triangles, a file that ends early and a face
    index outside the vertices raise ValueError.

    With ``texture`` also what the toolkit's renderers texture a model with: 'texture_uv' float64 [V,2] when the vertex element
    has texture_u and texture_v, 'texture_uv_face' float64 [F,6] (u_a v_a u_b v_b u_c v_c) when the face element has a second
    property ``list uchar|uint8 float|float32 texcoord`` (before or after the index list; a count other than 6 raises
    ValueError), and 'texture_file' (str) from a header line ``comment TextureFile <name>``.  Without ``texture`` such a face
    element is refused, as before."""
    data = Path(path).read_bytes()
    fmt, elements, off = _model_header(data)
    text = None
    if fmt == "ascii":
        text = data[off:].decode("ascii", "replace").split("\n")
        line = 0
    vert, faces, uv_face = None, None, None
    for name, count, props in elements:
        if name == "vertex":
            if any(p[0] == "list" for p in props):
                raise ValueError("list properties in the vertex element are not supported")
            if any(p[0] not in _TYPES for p in props):
                raise ValueError(f"unknown vertex property type in {[p[0] for p in props]}")
            dt = np.dtype([(p[1], "<" + _TYPES[p[0]]) for p in props])
            if fmt == "ascii":
                if line + count > len(text):
                    raise ValueError("PLY file ends inside the vertex element")
                rows = [text[line + r].split() for r in range(count)]
                if any(len(r) < len(props) for r in rows):
                    raise ValueError("PLY file ends inside the vertex element")
                vert = np.zeros(count, dt)
                for c, p in enumerate(props):
                    col = [r[c] for r in rows]
                    vert[p[1]] = np.array(col, np.float64).astype(dt[p[1]]) if count else []
                line += count
            else:
                if off + count * dt.itemsize > len(data):
                    raise ValueError("PLY file ends inside the vertex element")
                vert = np.frombuffer(data, dt, count, off)
                off += count * dt.itemsize
        elif name == "face":
            tex = [p for p in props if texture and p[0] == "list" and len(p) > 3 and p[3] == "texcoord"]
            if len(tex) > 1 or (tex and (tex[0][1] not in _COUNT_TYPES or tex[0][2] not in _UV_TYPES)):
                raise ValueError(f"unsupported face properties {props}: one list uchar float texcoord expected")
            index_first = not tex or props[0] is not tex[0]
            props = [p for p in props if not (tex and p is tex[0])]
            lists = [p for p in props if p[0] == "list"]
            if len(props) != 1 or len(lists) != 1 or lists[0][1] not in _COUNT_TYPES or lists[0][2] not in _INDEX_TYPES or \
                    lists[0][3] not in ("vertex_indices", "vertex_index"):
                raise ValueError(f"unsupported face properties {props}: one list uchar int vertex_indices expected")
            it = _TYPES[lists[0][2]]
            if fmt == "ascii":
                if line + count > len(text):
                    raise ValueError("PLY file ends inside the face element")
                rows = [text[line + r].split() for r in range(count)]
                if any(not r for r in rows):
                    raise ValueError("PLY file ends inside the face element")
                if tex:
                    # the two lists in the header's order: 3 a b c | 6 u_a v_a u_b v_b u_c v_c
                    at_i, at_t = (0, 4) if index_first else (7, 0)
                    if any(len(r) <= at_i or r[at_i] != "3" for r in rows):
                        raise ValueError("faces must be triangles")
                    if any(len(r) <= at_t or r[at_t] != "6" for r in rows):
                        raise ValueError("a texcoord list must hold 6 values (u, v of three corners)")
                    if any(len(r) != 11 for r in rows):
                        raise ValueError("PLY file ends inside the face element")
                    uv_face = np.array([r[at_t + 1:at_t + 7] for r in rows], np.float64).reshape(count, 6)
                    rows = [r[at_i:at_i + 4] for r in rows]
                if any(r[0] != "3" or len(r) != 4 for r in rows):
                    raise ValueError("faces must be triangles")
                faces = np.array([r[1:] for r in rows], np.int64).reshape(count, 3)
                line += count
            else:
                fields = [("n", "u1"), ("idx", "<" + it, (3,))]
                if tex:
                    uv_fields = [("tn", "u1"), ("uv", "<f4", (6,))]
                    fields = fields + uv_fields if index_first else uv_fields + fields
                dt = np.dtype(fields)
                if tex and count:
                    # the first record's two counts, read where they stand even when a short list leaves less than a whole
                    # record: the second one only when the first is right (else it is not where it is looked for)
                    at_n, at_t = (0, dt.fields["tn"][1]) if index_first else (dt.fields["n"][1], 0)
                    for at, want, what in sorted([(at_n, 3, "faces must be triangles"),
                                                  (at_t, 6, "a texcoord list must hold 6 values (u, v of three corners)")]):
                        if off + at < len(data) and data[off + at] != want:
                            raise ValueError(what)
                have = min(count, max(0, len(data) - off) // dt.itemsize)
                rows = np.frombuffer(data, dt, have, off)
                first_bad = rows["n"] != 3
                if tex:
                    # a wrong count in the first list shifts what follows: report the one that comes first in the record
                    tex_bad = rows["tn"] != 6
                    if (tex_bad & ~first_bad).any() if index_first else tex_bad.any():
                        raise ValueError("a texcoord list must hold 6 values (u, v of three corners)")
                    uv_face = rows["uv"].astype(np.float64)
                if first_bad.any():
                    raise ValueError("faces must be triangles")
                if have < count:
                    raise ValueError("PLY file ends inside the face element")
                faces = rows["idx"].astype(np.int64)
                off += count * dt.itemsize
        elif count:
            raise ValueError(f"unsupported PLY element {name}")
    if vert is None or not {"x", "y", "z"} <= set(vert.dtype.names):
        raise ValueError("no vertex element with x, y, z")
    cols = lambda names, dt=np.float64: np.stack([vert[n] for n in names], 1).astype(dt) if len(vert) else np.zeros((0, 3), dt)
    model = {"pts": cols("xyz"), "faces": np.zeros((0, 3), np.int64) if faces is None else faces}
    if len(model["faces"]) and (model["faces"].min() < 0 or model["faces"].max() >= len(vert)):
        raise ValueError(f"a face names a vertex outside 0..{len(vert) - 1}")
    if {"nx", "ny", "nz"} <= set(vert.dtype.names):
        model["normals"] = cols(("nx", "ny", "nz"))
    if {"red", "green", "blue"} <= set(vert.dtype.names):
        model["colors"] = cols(("red", "green", "blue"), np.result_type(*(vert.dtype[n] for n in ("red", "green", "blue"))))
    if texture:
        if {"texture_u", "texture_v"} <= set(vert.dtype.names):
            model["texture_uv"] = np.stack([vert["texture_u"], vert["texture_v"]], 1).astype(np.float64) if len(vert) else np.zeros((0, 2))
        if uv_face is not None:
            model["texture_uv_face"] = uv_face
        name = _texture_file(data)
        if name is not None:
            model["texture_file"] = name
    return model


def write_ply_model(path, pts, faces, normals=None, colors=None, ascii: bool = False, texture_uv=None, texture_uv_face=None,
                    texture_file=None):
    """A BOP object model in the property order of the toolkit's inout.save_ply: x y z, nx ny nz, red green blue (uchar; float
    colours are written as float), then ``list uchar int vertex_indices``.  Binary little-endian, or ASCII with ``ascii``
    (floats with 9 significant digits: a float32 survives the round trip).

    Texture (each optional; with none the bytes are those of a call without them), in save_ply2's order: ``texture_uv`` [V,2] as
    ``texture_u texture_v`` behind the colours, ``texture_uv_face`` [F,6] as ``list uchar float texcoord`` behind the index list,
    ``texture_file`` as ``comment TextureFile <name>`` directly after the format line.  Coordinates are written as float32."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    fields, cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], [pts]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        cols.append(np.asarray(normals, np.float32).reshape(len(pts), 3))
    if colors is not None:
        colors = np.asarray(colors).reshape(len(pts), 3)
        ct = "u1" if colors.dtype.kind in "ui" else "<f4"
        fields += [("red", ct), ("green", ct), ("blue", ct)]
        cols.append(colors.astype(ct))
    if texture_uv is not None:
        fields += [("texture_u", "<f4"), ("texture_v", "<f4")]
        cols.append(np.asarray(texture_uv, np.float32).reshape(len(pts), 2))
    if texture_uv_face is not None:
        texture_uv_face = np.asarray(texture_uv_face, np.float32).reshape(len(faces), 6)
    names = {"<f4": "float", "u1": "uchar"}
    header = "ply\nformat %s 1.0\n" % ("ascii" if ascii else "binary_little_endian")
    if texture_file is not None:
        header += f"comment TextureFile {texture_file}\n"
    header += "element vertex %d\n" % len(pts)
    header += "".join(f"property {names[t]} {n}\n" for n, t in fields)
    header += "element face %d\nproperty list uchar int vertex_indices\n" % len(faces)
    if texture_uv_face is not None:
        header += "property list uchar float texcoord\n"
    header += "end_header\n"
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        if ascii:
            fmt = lambda a: [str(int(x)) for x in a] if a.dtype.kind in "ui" else ["%.9g" % x for x in a]
            for r in range(len(pts)):
                fh.write((" ".join(sum((fmt(c[r]) for c in cols), [])) + "\n").encode("ascii"))
            for k, f in enumerate(faces):
                tail = "" if texture_uv_face is None else " 6 " + " ".join(fmt(texture_uv_face[k]))
                fh.write(("3 %d %d %d%s\n" % (*f, tail)).encode("ascii"))
        else:
            arr = np.empty(len(pts), np.dtype(fields))
            at = 0
            for c in cols:
                for k in range(c.shape[1]):
                    arr[fields[at + k][0]] = c[:, k]
                at += c.shape[1]
            face_fields = [("n", "u1"), ("idx", "<i4", (3,))] + ([] if texture_uv_face is None else [("tn", "u1"), ("uv", "<f4", (6,))])
            rows = np.empty(len(faces), np.dtype(face_fields))
            rows["n"] = 3
            rows["idx"] = faces
            if texture_uv_face is not None:
                rows["tn"] = 6
                rows["uv"] = texture_uv_face
            fh.write(arr.tobytes())
            fh.write(rows.tobytes())

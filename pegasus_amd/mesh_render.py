"""Object meshes rendered to depth on the GPU, and what the BOP toolkit builds on its depth renderer: ground-truth masks
(scripts/calc_gt_masks.py), scene_gt_info.json (scripts/calc_gt_info.py) and the VSD pose error (pose_error.vsd).

The meshes are the ``models/obj_NNNNNN.ply`` files ``pegasus_amd.mesh`` writes.  ``pgr_mesh_depth`` replaces the toolkit's
renderer (``renderer.render_object(obj_id, R, t, fx, fy, cx, cy)['depth']``), ``pgr_bop_gt_info`` the per-image sequence of
calc_gt_info.py; both are pinned in pegasus_amd/csrc/meshraster.hip.h.

    python -m pegasus_amd.mesh_render --dataset <dir> --models <dir> [--delta 15] [--translation_scale 1]

recomputes ``mask/``, ``mask_visib/`` and ``scene_gt_info.json`` of every scene under ``<dataset>/train`` from the meshes,
the poses in ``scene_gt.json`` and the depth images.

Shaded renders (``render``, ``Renderer``, ``vis_object_poses``) come from a visibility buffer: ``pgr_mesh_visibility`` keeps
(depth, job, face) per pixel, ``pgr_mesh_shade`` resolves it to rgb, depth, model coordinates, normals and ids.

    python -m pegasus_amd.mesh_render --dataset <dir> --models <dir> --vis <out dir> [--results <bop csv>] [--resolve_visib]
                                      [--shading flat|phong] [--textures] [--texture_filter nearest|bilinear]

writes ``<out>/<scene>/<image>.png`` instead: the models over the photographs at the ground-truth poses (the toolkit's
vis_gt_poses.py) or at a results file's estimates (vis_est_poses.py).
"""
from __future__ import annotations

import argparse
import ctypes as C
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib, bop_dataset as BD
from .bop_pose import broadcast_K, scene_gt_info_entry

MAX_CANVAS = 8192
DEFAULT_NEAR = 1e-3                  # model units; any positive value keeps the projection defined
DEFAULT_BUDGET = 1 << 30             # bytes of canvases per pgr_mesh_depth call
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


class MeshSet:
    """Triangle meshes by object id, uploaded once: ``vertices`` float32 [V,3] and ``faces`` int32 [F,3] (indices relative to
    the mesh's first vertex) shared by all, ``ranges[obj_id] = (vertex_first, vertex_count, face_first, face_count)``.
    ``meshes``: {obj_id: mesh.Mesh or a PLY path}; ``scale`` multiplies the vertices on load (BOP models are in millimetres:
    0.001 brings them to metres).  Paths are read with ply_io.read_ply_model (any BOP model file).

    ``normals`` and ``colors``: float32 [V,3] device tensors, None when no mesh of the set has them (a mesh object offers them
    as attributes of those names).  Where only some have colours the others get 0.5; colours above 1 are divided by 255.  Where
    only some have normals (or with ``compute_normals``, where none has) the others get ``vertex_normals``.

    ``textures`` (default off: every file loads as it always did): paths are read with their texture coordinates and the image
    their ``comment TextureFile`` line names, opened relative to the PLY (8-bit; RGBA drops alpha, grey is replicated); a mesh
    object offers ``corner_uv`` [F,3,2] and ``texture`` (uint8 [H,W,3]).  Per-vertex UVs are expanded to face corners
    (uv[faces]); per-face ones are taken as they are and win when a file has both.  Then ``corner_uv`` is a float32 [F,3,2]
    device tensor (zeros for meshes without UVs; None when no mesh has any), ``texels`` the uint8 device buffer of every image,
    ``texture_table`` its (byte offset, width, height) rows and ``texture_of[obj_id]`` a row index or -1; ``render`` then
    textures these objects as the toolkit's renderers do (v = 0 is the image's bottom row)."""

    def __init__(self, meshes: dict, device="cuda", scale: float = 1.0, diameters: Optional[dict] = None,
                 compute_normals: bool = False, textures: bool = False):
        import torch
        from .ply_io import read_ply_model
        vs, fs, ns, cs, uvs, images, self.ranges = [], [], [], [], [], [], {}
        self.texture_of, self.texture_table = {}, []
        v0 = f0 = 0
        for obj_id in sorted(meshes):
            m = meshes[obj_id]
            uv = image = None
            if isinstance(m, (str, Path)):
                model = read_ply_model(m, texture=True) if textures else read_ply_model(m)
                v, f, n, c = model["pts"], model["faces"], model.get("normals"), model.get("colors")
                if "texture_uv_face" in model:
                    uv = model["texture_uv_face"].reshape(-1, 3, 2)
                elif "texture_uv" in model:
                    uv = model["texture_uv"][np.asarray(f, np.int64).reshape(-1, 3)]
                if uv is not None and "texture_file" in model:
                    image = load_texture(Path(m).parent / model["texture_file"], m)
            else:
                v, f, n, c = m.vertices, m.faces, getattr(m, "normals", None), getattr(m, "colors", None)
                if textures:
                    uv, image = getattr(m, "corner_uv", None), getattr(m, "texture", None)
                    image = None if uv is None else image
            v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
            f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
            if scale != 1.0:
                v = (v.astype(np.float64) * scale).astype(np.float32)
            if len(f) and (f.min() < 0 or f.max() >= len(v)):
                raise ValueError(f"object {obj_id}: a face names a vertex outside 0..{len(v) - 1}")
            for name, a in (("normals", n), ("colors", c)):
                if a is not None and np.asarray(a).reshape(-1, 3).shape[0] != len(v):
                    raise ValueError(f"object {obj_id}: {name} must be [V,3]")
            if c is not None:
                c = np.asarray(c, np.float64).reshape(-1, 3)
                c = (c / 255.0 if c.size and c.max() > 1.0 else c).astype(np.float32)          # as the toolkit's renderers do
            if uv is not None:
                uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 3, 2)
                if len(uv) != len(f):
                    raise ValueError(f"object {obj_id}: corner_uv must be [F,3,2]")
            if image is not None:
                image = np.ascontiguousarray(image)
                if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or not (1 <= image.shape[0] <= MAX_CANVAS and
                                                                                               1 <= image.shape[1] <= MAX_CANVAS):
                    raise ValueError(f"object {obj_id}: a texture must be uint8 [H,W,3] with sides 1..{MAX_CANVAS}")
            self.texture_of[int(obj_id)] = len(images) if image is not None else -1
            if image is not None:
                images.append(image)
            uvs.append(uv)
            self.ranges[int(obj_id)] = (v0, len(v), f0, len(f))
            vs.append(v); fs.append(f)
            ns.append(None if n is None else np.asarray(n, np.float64).reshape(-1, 3).astype(np.float32)); cs.append(c)
            v0 += len(v); f0 += len(f)
        self.vertices = torch.from_numpy(np.concatenate(vs) if vs else np.zeros((0, 3), np.float32)).to(device)
        self.faces = torch.from_numpy(np.concatenate(fs) if fs else np.zeros((0, 3), np.int32)).to(device)
        self.normals = self.colors = None
        if compute_normals or any(n is not None for n in ns):
            ns = [vertex_normals(v, f).astype(np.float32) if n is None else n for v, f, n in zip(vs, fs, ns)]
            self.normals = torch.from_numpy(np.concatenate(ns) if ns else np.zeros((0, 3), np.float32)).to(device)
        if any(c is not None for c in cs):
            cs = [np.full((len(v), 3), 0.5, np.float32) if c is None else c for v, c in zip(vs, cs)]
            self.colors = torch.from_numpy(np.concatenate(cs)).to(device)
        self.corner_uv = self.texels = None
        if any(uv is not None for uv in uvs):
            uvs = [np.zeros((len(f), 3, 2), np.float32) if uv is None else uv for f, uv in zip(fs, uvs)]
            self.corner_uv = torch.from_numpy(np.concatenate(uvs)).to(device)
        if images:
            at = 0
            for image in images:
                self.texture_table.append((at, int(image.shape[1]), int(image.shape[0])))
                at += image.size
            self.texels = torch.from_numpy(np.concatenate([image.reshape(-1) for image in images])).to(device)
        self.diameters = {int(k): float(v) for k, v in (diameters or {}).items()}
        self.device = self.vertices.device

    @classmethod
    def from_dir(cls, models_dir, device="cuda", scale: float = 1.0, compute_normals: bool = False, textures: bool = False) -> "MeshSet":
        """Every ``obj_NNNNNN.ply`` of a BOP models directory, diameters from its ``models_info.json`` (scaled alike)."""
        files = BD.model_files(models_dir)
        diam = {int(k): v["diameter"] * scale for k, v in BD.read_models_info(models_dir).items()}
        return cls(files, device=device, scale=scale, diameters=diam, compute_normals=compute_normals, textures=textures)

    def mesh(self, obj_id: int):
        """(vertices, faces) of one object as host arrays."""
        v0, nv, f0, nf = self.ranges[int(obj_id)]
        return self.vertices[v0:v0 + nv].cpu().numpy(), self.faces[f0:f0 + nf].cpu().numpy()


def load_texture(path, model_path=None) -> np.ndarray:
    """The image of a model's ``comment TextureFile`` line as uint8 [H,W,3], as stored (row 0 is the top row): RGBA drops
    alpha, grey is replicated; 16-bit images are refused.  A missing file raises FileNotFoundError naming it and the model."""
    path = Path(path)
    if not path.is_file():
        raise FileNotFoundError(f"texture {path} named by {model_path if model_path is not None else 'the model'} does not exist")
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("I;16", "I;16B", "I;16L", "I", "F"):
            raise ValueError(f"texture {path}: 16-bit images (mode {im.mode}) are not supported; convert it to 8 bits per channel")
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8))


def mesh_jobs(meshes: MeshSet, jobs: Sequence, K, margin=(0, 0), slots: Optional[Sequence[int]] = None):
    """The PgrMeshJob array of ``jobs`` = [(obj_id, R [3,3], t [3]), ...]: pose and intrinsics rounded to float32, the
    principal point moved by the margin."""
    Ks = broadcast_K(K, len(jobs))
    arr = (_lib.PgrMeshJob * max(len(jobs), 1))()
    for k, (obj_id, R, t) in enumerate(jobs):
        if int(obj_id) not in meshes.ranges:
            raise KeyError(f"object {obj_id} is not in the mesh set")
        v0, nv, f0, nf = meshes.ranges[int(obj_id)]
        R32 = np.asarray(R, np.float64).reshape(9).astype(np.float32)
        t32 = np.asarray(t, np.float64).reshape(3).astype(np.float32)
        Kk = Ks[k]
        arr[k] = _lib.PgrMeshJob(vertex_first=v0, vertex_count=nv, face_first=f0, face_count=nf,
                                 R=(C.c_float * 9)(*R32.tolist()), t=(C.c_float * 3)(*t32.tolist()),
                                 fx=float(np.float32(Kk[0, 0])), fy=float(np.float32(Kk[1, 1])),
                                 cx=float(np.float32(Kk[0, 2] + margin[0])), cy=float(np.float32(Kk[1, 2] + margin[1])),
                                 slot=int(k if slots is None else slots[k]))
    return arr


def render_depth(meshes: MeshSet, jobs: Sequence, K, size, margin=(0, 0), near: float = DEFAULT_NEAR,
                 budget_bytes: int = DEFAULT_BUDGET, return_straddle: bool = False):
    """Depth images of ``jobs`` = [(obj_id, R, t), ...] (model to camera, in the meshes' units): float32 [J,Hc,Wc] on the
    meshes' device, camera z of the nearest surface, 0 where nothing is hit.  ``size`` = (W, H) of the image, ``margin`` =
    (mx, my) pixels added on every side (the canvas is W + 2 mx by H + 2 my, the principal point moves by the margin; the
    toolkit's truncation canvas is margin = size).  ``K``: one [3,3] or one per job.  Jobs go to the library in chunks whose
    canvases stay within ``budget_bytes``.  ``return_straddle``: also the number of faces dropped because they straddle
    ``near`` (an int32 tensor, not read back here)."""
    import torch
    W, H = int(size[0]), int(size[1])
    mx, my = int(margin[0]), int(margin[1])
    Wc, Hc = W + 2 * mx, H + 2 * my
    if not (1 <= Wc <= MAX_CANVAS and 1 <= Hc <= MAX_CANVAS) or mx < 0 or my < 0:
        raise ValueError(f"canvas {Wc} x {Hc}: each side must be 1..{MAX_CANVAS}")
    device = meshes.device
    if device.type != "cuda":
        raise RuntimeError("render_depth needs a mesh set on a HIP device; there is no CPU path")
    J = len(jobs)
    Ks = broadcast_K(K, J)
    out = torch.empty((J, Hc, Wc), dtype=torch.float32, device=device)
    straddle = torch.zeros(1, dtype=torch.int32, device=device)
    per_call = max(1, int(budget_bytes) // (4 * Hc * Wc))
    for j0 in range(0, J, per_call):
        chunk = jobs[j0:j0 + per_call]
        arr = mesh_jobs(meshes, chunk, Ks[j0:j0 + per_call], (mx, my))
        ws = _lib.workspace("pgr_mesh_depth", device, len(chunk), arr)
        count = torch.zeros(1, dtype=torch.int32, device=device)
        _lib.call("pgr_mesh_depth", device, _lib.ptr(meshes.vertices), meshes.vertices.shape[0], _lib.ptr(meshes.faces),
                  meshes.faces.shape[0], len(chunk), arr, Wc, Hc, float(near), _lib.ptr(out[j0:j0 + len(chunk)]), len(chunk),
                  _lib.ptr(count), _lib.ptr(ws), ws.numel())
        straddle += count
    return (out, straddle) if return_straddle else out


# ---- shaded renders: visibility buffer and resolve --------------------------------------------------------------------
RENDER_OUTPUTS = {"rgb": ("float32", 3), "depth": ("float32", 0), "xyz": ("float32", 3), "normal": ("float32", 3),
                  "face_id": ("int32", 0), "job_id": ("int32", 0), "uv": ("float32", 2)}
TEXTURE_FILTERS = {"nearest": _lib.PGR_TEXTURE_NEAREST, "bilinear": _lib.PGR_TEXTURE_BILINEAR}
DEFAULT_SURF_COLOR = (0.5, 0.5, 0.5)             # the toolkit renderers' grey


def vertex_normals(vertices, faces) -> np.ndarray:
    """Per-vertex normals float64 [V,3] by open3d's compute_vertex_normals rule: the unit normals of the faces, summed per
    vertex in face order, normalised; all in float64 on the host.  A vertex of no face (or of degenerate faces only) gets 0."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    length = np.linalg.norm(fn, axis=1, keepdims=True)
    fn = np.divide(fn, length, out=np.zeros_like(fn), where=length > 0)
    out = np.zeros_like(v)
    for c in range(3):
        np.add.at(out, f[:, c], fn)
    length = np.linalg.norm(out, axis=1, keepdims=True)
    return np.divide(out, length, out=np.zeros_like(out), where=length > 0)


def _slot_chunks(slots, per_call_slots: int):
    """Calls of a render: jobs that share a slot stay in one call (the visibility pass composites them), a call holds at
    most PGR_MESH_VISIBILITY_MAX_JOBS jobs and ``per_call_slots`` slots.  Yields (job indices in order, slot ids)."""
    by_slot = {}
    for k, s in enumerate(slots):
        by_slot.setdefault(int(s), []).append(k)
    jobs, ids = [], []
    for s, ks in by_slot.items():
        if len(ks) > _lib.PGR_MESH_VISIBILITY_MAX_JOBS:
            raise ValueError(f"slot {s} holds {len(ks)} jobs; one slot takes at most {_lib.PGR_MESH_VISIBILITY_MAX_JOBS}")
        if jobs and (len(jobs) + len(ks) > _lib.PGR_MESH_VISIBILITY_MAX_JOBS or len(ids) >= per_call_slots):
            yield sorted(jobs), ids
            jobs, ids = [], []
        jobs += ks; ids.append(s)
    if jobs:
        yield sorted(jobs), ids


def render(meshes: MeshSet, jobs: Sequence, K, size, outputs=("rgb", "depth"), shading: str = "phong", ambient: float = 0.5,
           light=(0.0, 0.0, 0.0), surf_colors=None, bg=(0.0, 0.0, 0.0), margin=(0, 0), near: float = DEFAULT_NEAR,
           slots: Optional[Sequence[int]] = None, budget_bytes: int = DEFAULT_BUDGET, return_straddle: bool = False,
           texture_filter: str = "nearest") -> dict:
    """Shaded renders of ``jobs`` = [(obj_id, R, t), ...] as the toolkit's renderers shade them (one light, ambient plus
    diffuse), and the dense maps only a mesh gives.  Returns {name: device tensor} for every name in ``outputs``:

        rgb      float32 [S,Hc,Wc,3]  min(ambient + max(dot(L, n), 0), 1) * colour; ``bg`` where nothing is hit
        depth    float32 [S,Hc,Wc]    camera z of the nearest surface (the bytes of render_depth), 0 where nothing is hit
        xyz      float32 [S,Hc,Wc,3]  model coordinates of the surface point, 0 where nothing is hit
        normal   float32 [S,Hc,Wc,3]  unit normal in the camera frame, 0 where nothing is hit
        face_id, job_id  int32 [S,Hc,Wc]  the face (index in its mesh) and the job (index in ``jobs``), -1 where nothing is hit
        uv       float32 [S,Hc,Wc,2]  texture coordinates of the surface point, perspective-correct (a set loaded with
                                      ``textures=True`` whose meshes have UVs), 0 where nothing is hit

    ``slots``: the canvas of each job (default: one each, S = len(jobs)); jobs that share a slot are composited nearest-first
    by the visibility pass itself (at equal depth the earlier job wins).  ``shading``: "phong" interpolates the set's vertex
    normals (a set without normals raises), "flat" takes the face's own.  The colour is the set's vertex colours; without
    them, or with ``surf_colors`` ([3] or one [3] per job) given, the surf colour (default the toolkit's 0.5 grey).  ``light``
    is in the camera frame (the toolkit's default: the camera centre).  ``size``, ``margin``, ``K``, ``near`` as render_depth.
    In a set loaded with ``textures=True`` an object with a texture takes its colour from it (``pgr_mesh_shade_textured``;
    ``texture_filter``: "nearest", what the toolkit's renderers get from vispy / glumpy by default, or "bilinear"; clamp to
    edge), unless ``surf_colors`` is given, as in the toolkit; parity with an OpenGL render is not pinned.
    The rule is pinned above mesh_shade_kernel in csrc/meshraster.hip.h; calls are chunked by the library's 1024 jobs per call and
    by ``budget_bytes`` of canvases."""
    import torch
    W, H = int(size[0]), int(size[1])
    mx, my = int(margin[0]), int(margin[1])
    Wc, Hc = W + 2 * mx, H + 2 * my
    if not (1 <= Wc <= MAX_CANVAS and 1 <= Hc <= MAX_CANVAS) or mx < 0 or my < 0:
        raise ValueError(f"canvas {Wc} x {Hc}: each side must be 1..{MAX_CANVAS}")
    outputs = tuple(outputs)
    unknown = [o for o in outputs if o not in RENDER_OUTPUTS]
    if unknown or not outputs:
        raise ValueError(f"outputs must be a non-empty choice of {sorted(RENDER_OUTPUTS)}, got {outputs!r}")
    if shading not in ("phong", "flat"):
        raise ValueError(f"shading must be 'phong' or 'flat', got {shading!r}")
    if texture_filter not in TEXTURE_FILTERS:
        raise ValueError(f"texture_filter must be one of {sorted(TEXTURE_FILTERS)}, got {texture_filter!r}")
    if "uv" in outputs and getattr(meshes, "corner_uv", None) is None:
        raise ValueError("the 'uv' output needs a mesh set with texture coordinates (MeshSet(..., textures=True))")
    if shading == "phong" and meshes.normals is None and ("rgb" in outputs or "normal" in outputs):
        raise ValueError("shading='phong' needs a mesh set with normals (MeshSet(..., compute_normals=True), or shading='flat')")
    device = meshes.device
    if device.type != "cuda":
        raise RuntimeError("render needs a mesh set on a HIP device; there is no CPU path")
    J = len(jobs)
    slots = list(range(J)) if slots is None else [int(s) for s in slots]
    if len(slots) != J or any(s < 0 for s in slots):
        raise ValueError("slots must name one canvas >= 0 per job")
    S = max(slots) + 1 if slots else 0
    Ks = broadcast_K(K, J)
    surf = None
    if surf_colors is not None:
        surf = np.ascontiguousarray(np.broadcast_to(np.asarray(surf_colors, np.float32), (J, 3)))
    colors = meshes.colors if surf is None else None
    corner_uv = getattr(meshes, "corner_uv", None)
    texels = getattr(meshes, "texels", None) if surf is None else None
    textured = corner_uv is not None and (texels is not None or "uv" in outputs)
    normals = meshes.normals if shading == "phong" else None
    bg32 = np.asarray(bg, np.float32).reshape(3)
    out = {}
    for name in outputs:
        dt, ch = RENDER_OUTPUTS[name]
        shape = (S, Hc, Wc) + ((ch,) if ch else ())
        if name == "rgb":
            out[name] = torch.from_numpy(bg32).to(device).expand(shape).contiguous()
        else:
            out[name] = torch.full(shape, -1 if dt == "int32" else 0, dtype=getattr(torch, dt), device=device)
    straddle = torch.zeros(1, dtype=torch.int32, device=device)
    per_pixel = 8 + sum(4 * max(RENDER_OUTPUTS[n][1], 1) for n in outputs)
    per_call = max(1, int(budget_bytes) // (per_pixel * Hc * Wc))
    for ks, ids in _slot_chunks(slots, per_call):
        local = {s: q for q, s in enumerate(ids)}
        chunk = [jobs[k] for k in ks]
        arr = mesh_jobs(meshes, chunk, Ks[ks], (mx, my), slots=[local[slots[k]] for k in ks])
        n, ns = len(chunk), len(ids)
        keys = torch.empty((ns, Hc, Wc), dtype=torch.int64, device=device)
        count = torch.zeros(1, dtype=torch.int32, device=device)
        ws = _lib.workspace("pgr_mesh_visibility", device, n, arr)
        _lib.call("pgr_mesh_visibility", device, _lib.ptr(meshes.vertices), meshes.vertices.shape[0], _lib.ptr(meshes.faces),
                  meshes.faces.shape[0], n, arr, Wc, Hc, float(near), _lib.ptr(keys), ns, _lib.ptr(count), _lib.ptr(ws), ws.numel())
        straddle += count
        part = {name: torch.empty((ns,) + tuple(out[name].shape[1:]), dtype=out[name].dtype, device=device) for name in outputs}
        sub = None if surf is None else np.ascontiguousarray(surf[ks])
        uv_part = part.pop("uv", None)
        shade = _lib.PgrMeshShade(normals=_lib.ptr(normals), colors=_lib.ptr(colors),
                                  surf_colors=None if sub is None else sub.ctypes.data_as(C.POINTER(C.c_float)),
                                  light=(C.c_float * 3)(*np.asarray(light, np.float32).reshape(3).tolist()), ambient=float(ambient),
                                  bg=(C.c_float * 3)(*bg32.tolist()), **{name: _lib.ptr(t) for name, t in part.items()})
        mesh_args = (_lib.ptr(meshes.vertices), meshes.vertices.shape[0], _lib.ptr(meshes.faces), meshes.faces.shape[0], n, arr, Wc, Hc,
                     float(near), _lib.ptr(keys), ns, C.byref(shade))
        if textured:
            table = (_lib.PgrMeshTexture * max(len(meshes.texture_table), 1))(*[_lib.PgrMeshTexture(offset=o, width=w, height=h)
                                                                                for o, w, h in meshes.texture_table])
            which = (C.c_int32 * n)(*[meshes.texture_of[int(job[0])] if texels is not None else -1 for job in chunk])
            tex = _lib.PgrMeshTextures(corner_uv=_lib.ptr(corner_uv), texels=_lib.ptr(texels), texel_bytes=0 if texels is None else texels.numel(),
                                       n_textures=len(meshes.texture_table) if texels is not None else 0, textures=table, job_texture=which,
                                       filter=TEXTURE_FILTERS[texture_filter], uv=_lib.ptr(uv_part))
            ws2 = _lib.workspace("pgr_mesh_shade_textured", device, n, arr)
            _lib.call("pgr_mesh_shade_textured", device, *mesh_args, C.byref(tex), _lib.ptr(ws2), ws2.numel())
        else:
            ws2 = _lib.workspace("pgr_mesh_shade", device, n, arr)
            _lib.call("pgr_mesh_shade", device, *mesh_args, _lib.ptr(ws2), ws2.numel())
        if uv_part is not None:
            part["uv"] = uv_part
        index = torch.as_tensor(ids, device=device)
        for name, t in part.items():
            if name == "job_id":                                     # the index in the call -> the index in ``jobs``
                lut = torch.as_tensor(ks + [-1], dtype=torch.int32, device=device)
                t = lut[t.long()]
            out[name][index] = t
    if return_straddle:
        out["straddle"] = straddle
    return out


class Renderer:
    """The toolkit renderer's calls (renderer.create_renderer(width, height, ...): add_object, remove_object, render_object,
    set_light_cam_pos, set_light_ambient_weight) on ``render``: code of the toolkit that is handed a renderer takes this one.
    Models and translations share their unit (the toolkit's: millimetres)."""

    def __init__(self, width: int, height: int, mode: str = "rgb+depth", shading: str = "phong", bg_color=(0.0, 0.0, 0.0, 0.0),
                 device="cuda", near: float = DEFAULT_NEAR, texture_filter: str = "nearest"):
        if texture_filter not in TEXTURE_FILTERS:
            raise ValueError(f"texture_filter must be one of {sorted(TEXTURE_FILTERS)}, got {texture_filter!r}")
        self.texture_filter = texture_filter
        if mode not in ("rgb+depth", "rgb", "depth"):
            raise ValueError(f"mode must be 'rgb+depth', 'rgb' or 'depth', got {mode!r}")
        if shading not in ("phong", "flat"):
            raise ValueError(f"shading must be 'phong' or 'flat', got {shading!r}")
        self.width, self.height, self.mode, self.shading = int(width), int(height), mode, shading
        self.bg_color = tuple(float(c) for c in bg_color)[:3]
        self.device, self.near = device, float(near)
        self.light_cam_pos, self.light_ambient_weight = (0.0, 0.0, 0.0), 0.5
        self.model_paths, self.surf_colors, self._meshes = {}, {}, None

    def set_light_cam_pos(self, light_cam_pos):
        self.light_cam_pos = tuple(float(x) for x in np.asarray(light_cam_pos, np.float64).reshape(3))

    def set_light_ambient_weight(self, light_ambient_weight):
        self.light_ambient_weight = float(light_ambient_weight)

    def add_object(self, obj_id, model_path, surf_color=None, **kwargs):
        """``surf_color``: a colour (r, g, b in [0,1]) used instead of the model's texture or vertex colours.  A model whose
        file names a texture (``comment TextureFile``) and has texture coordinates is drawn with it, else with its vertex
        colours, else grey: the toolkit's order.  Other keywords of the toolkit's renderers are accepted and ignored."""
        self.model_paths[int(obj_id)] = model_path
        self.surf_colors[int(obj_id)] = surf_color
        self._meshes = None

    def remove_object(self, obj_id):
        self.model_paths.pop(int(obj_id), None)
        self.surf_colors.pop(int(obj_id), None)
        self._meshes = None

    @property
    def meshes(self) -> MeshSet:
        if self._meshes is None:
            self._meshes = MeshSet(dict(self.model_paths), device=self.device, compute_normals=self.shading == "phong", textures=True)
        return self._meshes

    def render_object(self, obj_id, R, t, fx, fy, cx, cy) -> dict:
        """{'rgb': uint8 [H,W,3], 'depth': float32 [H,W]} (what the mode names) as host arrays; rgb = rint(255 clip(rgb, 0, 1))."""
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)
        outputs = tuple(o for o in ("rgb", "depth") if o in self.mode.split("+"))
        surf = self.surf_colors.get(int(obj_id))
        got = render(self.meshes, [(int(obj_id), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3))],
                     K, (self.width, self.height), outputs=outputs, shading=self.shading, ambient=self.light_ambient_weight,
                     light=self.light_cam_pos, surf_colors=None if surf is None else [surf], bg=self.bg_color, near=self.near,
                     texture_filter=self.texture_filter)
        out = {}
        if "rgb" in got:
            out["rgb"] = rgb_to_uint8(got["rgb"][0]).cpu().numpy()
        if "depth" in got:
            out["depth"] = got["depth"][0].cpu().numpy()
        return out


def rgb_to_uint8(rgb):
    """rint(255 clip(rgb, 0, 1)) as uint8, in float32 (torch.round is round-half-even, as rint)."""
    import torch
    return torch.round(rgb.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


BBOX_GREY = int(0.3 * 255)                       # visualization.vis_object_poses: bbox_color = (0.3, 0.3, 0.3)


def draw_rect(im: np.ndarray, rect, value: int = BBOX_GREY) -> np.ndarray:
    """visualization.draw_rect without PIL: the one-pixel outline of [x, y, w, h] (corners (x, y) and (x + w, y + h), both
    drawn), clipped to the image, set to ``value`` in every channel; in place."""
    x0, y0, x1, y1 = int(rect[0]), int(rect[1]), int(rect[0] + rect[2]), int(rect[1] + rect[3])
    H, W = im.shape[:2]
    xs, ys = slice(max(x0, 0), min(x1, W - 1) + 1), slice(max(y0, 0), min(y1, H - 1) + 1)
    for y in (y0, y1):
        if 0 <= y < H:
            im[y, xs] = value
    for x in (x0, x1):
        if 0 <= x < W:
            im[ys, x] = value
    return im


def depth_for_vis(depth, valid_start=0.2, valid_end=1.0):
    """visualization.depth_for_vis: the positive values of ``depth`` brought to [valid_start, valid_end], float64."""
    mask = depth > 0
    d = depth.astype(np.float64)
    if mask.any():
        d[mask] -= d[mask].min()
        top = d[mask].max()
        if top > 0:
            d[mask] /= top / (valid_end - valid_start)
        d[mask] += valid_start
    return d


def vis_object_poses(poses, K, meshes: MeshSet, rgb=None, depth=None, vis_rgb_path=None, vis_depth_diff_path=None,
                     vis_rgb_resolve_visib: bool = False, shading: str = "phong", near: float = DEFAULT_NEAR,
                     texture_filter: str = "nearest") -> dict:
    """visualization.vis_object_poses with the renderer replaced by the mesh set: the models of ``poses`` = [{'obj_id', 'R',
    't'}, ...] shaded and blended over ``rgb`` (uint8 [H,W,3]), and their depth against ``depth`` [H,W] (the poses' unit).

    With ``vis_rgb_resolve_visib`` all poses share one canvas (the nearest surface shows); otherwise each is rendered in its
    own and the images are summed, saturating at 255.  The RGB visualisation is 0.5 rgb + 0.5 render plus the grey box
    (misc.calc_2d_bbox of each object's own pixels), clipped at 255; the depth-difference image follows the toolkit's
    (valid = depth > 0 and rendered > 0, difference = valid (rendered - depth), red where it is below the VSD delta of 15).
    A mesh set loaded with ``textures=True`` shows its textured objects textured (``texture_filter`` as in render).
    No text labels.  Images are written as PNG; returned: {'vis_rgb', 'depth_diff', 'depth_diff_vis', 'ren_depth'} (those asked for)."""
    vis_rgb, vis_diff = vis_rgb_path is not None, vis_depth_diff_path is not None
    if vis_rgb and rgb is None:
        raise ValueError("RGB visualization triggered but RGB image not provided.")
    if vis_diff and depth is None:
        raise ValueError("Depth visualization triggered but D image not provided.")
    ref = rgb if rgb is not None else depth
    if ref is None:
        raise ValueError("an rgb or a depth image is needed for the image size")
    H, W = ref.shape[:2]
    if rgb is not None and depth is not None and depth.shape[:2] != (H, W):
        raise ValueError("The RGB and D images must have the same size.")
    jobs = [(int(p["obj_id"]), np.asarray(p["R"], np.float64).reshape(3, 3), np.asarray(p["t"], np.float64).reshape(3))
            for p in poses]
    out = {}
    shared = None
    if jobs and (vis_diff or (vis_rgb and vis_rgb_resolve_visib)):
        shared = render(meshes, jobs, K, (W, H), outputs=("rgb", "depth") if vis_rgb else ("depth",), shading=shading, near=near,
                        slots=[0] * len(jobs), texture_filter=texture_filter)
    if vis_rgb:
        ren = np.zeros((H, W, 3), np.uint8)
        info = np.zeros((H, W, 3), np.uint8)
        if jobs:
            own = rgb_to_uint8(render(meshes, jobs, K, (W, H), outputs=("rgb",), shading=shading, near=near,
                                      texture_filter=texture_filter)["rgb"]).cpu().numpy()
            if vis_rgb_resolve_visib:
                ren = rgb_to_uint8(shared["rgb"][0]).cpu().numpy()
            else:
                ren = np.minimum(own.astype(np.int64).sum(0), 255).astype(np.uint8)
            for m in own:
                ys, xs = (m > 0).any(2).nonzero()
                if len(ys):
                    draw_rect(info, [xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min()])
        vis = 0.5 * np.asarray(rgb).astype(np.float32) + 0.5 * ren.astype(np.float32) + 1.0 * info.astype(np.float32)
        vis[vis > 255] = 255
        out["vis_rgb"] = vis.astype(np.uint8)
        Path(vis_rgb_path).parent.mkdir(parents=True, exist_ok=True)
        Path(vis_rgb_path).write_bytes(BD.encode_png(out["vis_rgb"]))
    if vis_diff:
        ren_depth = shared["depth"][0].cpu().numpy() if shared is not None else np.zeros((H, W), np.float32)
        d = np.asarray(depth)
        valid = (d > 0) * (ren_depth > 0)
        diff = valid * (ren_depth.astype(np.float32) - d)
        below = (255 * (valid * (diff < 15))).astype(np.uint8)
        grey = 255 * depth_for_vis(diff - diff.min())
        image = np.dstack([below, grey, grey]).astype(np.uint8)
        image[np.logical_not(valid)] = 0
        out.update(depth_diff=diff, depth_diff_vis=image, ren_depth=ren_depth)
        Path(vis_depth_diff_path).parent.mkdir(parents=True, exist_ok=True)
        Path(vis_depth_diff_path).write_bytes(BD.encode_png(image))
    return out


# ---- ground truth ---------------------------------------------------------------------------------------------------
def dist_image(depth, K):
    """misc.depth_im_to_dist_im_fast in torch: float64 [..., H, W] distances from the camera centre, the pixel taken at its
    integer index, 0 where the depth is 0.  ``K``: float64 [3,3] (or [..., 3, 3] broadcasting over the leading axes)."""
    import torch
    d = depth.to(torch.float64)
    H, W = d.shape[-2:]
    K = torch.as_tensor(np.asarray(K, np.float64) if not torch.is_tensor(K) else K, dtype=torch.float64, device=d.device)
    xs = torch.arange(W, dtype=torch.float64, device=d.device)
    ys = torch.arange(H, dtype=torch.float64, device=d.device)[:, None]
    pre_x = (xs - K[..., 0, 2, None, None]) / K[..., 0, 0, None, None]
    pre_y = (ys - K[..., 1, 2, None, None]) / K[..., 1, 1, None, None]
    X, Y = pre_x * d, pre_y * d
    return torch.sqrt((X * X + Y * Y) + d * d)


def visibility_mask(dist_test, dist_model, delta: float):
    """visibility._estimate_visib_mask, mode bop19: the difference of the distances in float32."""
    import torch
    diff = dist_model.to(torch.float32) - dist_test.to(torch.float32)
    return ((diff <= delta) | (dist_test == 0)) & (dist_model > 0)


def reduce_gt_info_torch(canvases, margin, scene_depth, frames, Ks, delta: float):
    """What pgr_bop_gt_info computes, restated in torch ops on the tensors' device (CPU included): (mask uint8 [J,H,W],
    mask_visib uint8 [J,H,W], stats int32 [J,11]) of canvases float32 [J,Hc,Wc] against scene_depth [F,H,W]; ``frames`` [J]
    names each job's image, ``Ks`` float64 [J,3,3]."""
    import torch
    mx, my = int(margin[0]), int(margin[1])
    J = canvases.shape[0]
    H, W = scene_depth.shape[-2:]
    dev = canvases.device
    frames = torch.as_tensor(np.asarray(frames, np.int64), device=dev)
    Ks = torch.as_tensor(np.asarray(Ks, np.float64), device=dev)
    window = canvases[:, my:my + H, mx:mx + W]
    dist_model = dist_image(window, Ks)
    dist_test = dist_image(scene_depth[frames], Ks)
    visib = visibility_mask(dist_test, dist_model, float(np.float32(delta)))
    mask = dist_model > 0
    large = canvases > 0
    stats = torch.empty((J, _lib.PGR_GT_INFO_STATS), dtype=torch.int64, device=dev)
    stats[:, 0] = large.flatten(1).sum(1)
    stats[:, 1] = (mask & (dist_test > 0)).flatten(1).sum(1)
    stats[:, 2] = visib.flatten(1).sum(1)

    def extent(m, ox, oy, col):
        h, w = m.shape[-2:]
        xs = torch.arange(w, device=dev) - ox
        ys = torch.arange(h, device=dev) - oy
        cols, rows = m.any(-2), m.any(-1)
        stats[:, col + 0] = torch.where(cols, xs, INT32_MAX).amin(-1)
        stats[:, col + 1] = torch.where(rows, ys, INT32_MAX).amin(-1)
        stats[:, col + 2] = torch.where(cols, xs, INT32_MIN).amax(-1)
        stats[:, col + 3] = torch.where(rows, ys, INT32_MIN).amax(-1)
    extent(large, mx, my, 3)
    extent(visib, 0, 0, 7)
    return mask.to(torch.uint8), visib.to(torch.uint8), stats.to(torch.int32)


def reduce_gt_info(canvases, margin, scene_depth, frames, Ks, delta: float):
    """pgr_bop_gt_info: like reduce_gt_info_torch, on a HIP device."""
    import torch
    dev = canvases.device
    if dev.type != "cuda":
        raise RuntimeError("reduce_gt_info needs tensors on a HIP device (reduce_gt_info_torch restates it for any device)")
    canvases = canvases.float().contiguous()
    scene_depth = scene_depth.to(dev).float().contiguous()
    J, Hc, Wc = canvases.shape
    F, H, W = scene_depth.shape
    Ks = np.asarray(Ks, np.float64).reshape(J, 3, 3)
    arr = (_lib.PgrGtInfoJob * max(J, 1))()
    for k in range(J):
        arr[k] = _lib.PgrGtInfoJob(slot=k, frame=int(frames[k]), fx=Ks[k, 0, 0], fy=Ks[k, 1, 1], cx=Ks[k, 0, 2], cy=Ks[k, 1, 2])
    mask = torch.empty((J, H, W), dtype=torch.uint8, device=dev)
    visib = torch.empty_like(mask)
    stats = torch.empty((J, _lib.PGR_GT_INFO_STATS), dtype=torch.int32, device=dev)
    _lib.call("pgr_bop_gt_info", dev, _lib.ptr(canvases), J, Wc, Hc, int(margin[0]), int(margin[1]), _lib.ptr(scene_depth),
              F, W, H, J, arr, float(delta), _lib.ptr(mask), _lib.ptr(visib), _lib.ptr(stats))
    return mask, visib, stats


def info_from_stats(stats) -> dict:
    """scene_gt_info fields from stats rows [..., 11] as calc_gt_info.py derives them: visib_fract = visible / all (0 without
    a silhouette), boxes (x, y, w, h) with w = x_max - x_min (misc.calc_2d_bbox), both [-1,-1,-1,-1] when nothing is
    visible.  Arrays shaped [...] (boxes [..., 4]), the layout bop_pose.scene_gt_info_entry takes."""
    s = np.asarray(stats.cpu() if hasattr(stats, "cpu") else stats).astype(np.int64)
    px_all, px_valid, px_visib = s[..., 0], s[..., 1], s[..., 2]
    seen = (px_visib > 0)[..., None]
    box = lambda c: np.stack([s[..., c], s[..., c + 1], s[..., c + 2] - s[..., c], s[..., c + 3] - s[..., c + 1]], -1)
    fract = np.where(px_all > 0, px_visib / np.maximum(px_all, 1).astype(np.float64), 0.0)
    return dict(px_count_all=px_all, px_count_valid=px_valid, px_count_visib=px_visib, visib_fract=fract,
                bbox_obj=np.where(seen, box(3), -1), bbox_visib=np.where(seen, box(7), -1))


def gt_from_meshes(meshes: MeshSet, scene_gt: dict, scene_camera: dict, depth, delta: float = 15.0,
                   translation_scale: float = 1.0, near: float = DEFAULT_NEAR, budget_bytes: int = DEFAULT_BUDGET):
    """BOP ground truth of a batch of frames from the objects' meshes, as calc_gt_info.py and calc_gt_masks.py compute it:
    every object of ``scene_gt[str(i)]`` is rendered at its pose on the toolkit's 3x canvas and tested against frame i of
    ``depth`` [B,H,W] (the depth images as written, times the frame's ``depth_scale``: millimetres).

    Units follow scene_gt: ``translation_scale`` is what its translations were written with (1000: millimetres, 1:
    metres -- the default here, in bop_pose and in the writer), the meshes are in that unit, the depth is brought to it, and ``delta`` (millimetres, the toolkit's 15) too.
    Returns (masks, masks_visib, info): per frame a uint8 device tensor [K_i,H,W] each, and the scene_gt_info list."""
    import torch
    dev = meshes.device
    depth = torch.as_tensor(depth).to(dev)
    B, H, W = depth.shape
    unit = BD.unit_of(translation_scale)
    scale = torch.tensor([BD.depth_unit(scene_camera[str(i)], unit) for i in range(B)], device=dev)
    scene = (depth.to(torch.float32) * scale.to(torch.float32)[:, None, None]).contiguous()
    jobs, frames, Ks = [], [], []
    for i in range(B):
        K = BD.cam_K(scene_camera[str(i)])
        for e in scene_gt[str(i)]:
            jobs.append((int(e["obj_id"]), *BD.pose_of(e)))
            frames.append(i); Ks.append(K)
    masks = [[] for _ in range(B)]
    visibs = [[] for _ in range(B)]
    rows = []
    per_call = max(1, int(budget_bytes) // (4 * 9 * H * W))
    for j0 in range(0, len(jobs), per_call):
        sl = slice(j0, j0 + per_call)
        canvases = render_depth(meshes, jobs[sl], np.stack(Ks[sl]), (W, H), margin=(W, H), near=near, budget_bytes=budget_bytes)
        m, v, s = reduce_gt_info(canvases, (W, H), scene, frames[sl], np.stack(Ks[sl]), delta * unit)
        rows.append(s)
        for k, i in enumerate(frames[sl]):
            masks[i].append(m[k]); visibs[i].append(v[k])
    stats = torch.cat(rows).cpu().numpy() if rows else np.zeros((0, _lib.PGR_GT_INFO_STATS), np.int32)
    info, at = [], 0
    empty = torch.zeros((0, H, W), dtype=torch.uint8, device=dev)
    for i in range(B):
        n = len(masks[i])
        info.append(scene_gt_info_entry(info_from_stats(stats[at:at + n]), slice(None)) if n else [])
        at += n
    stack = lambda l: torch.stack(l) if l else empty
    return [stack(m) for m in masks], [stack(v) for v in visibs], info


# ---- VSD ------------------------------------------------------------------------------------------------------------
def vsd_from_depths(depth_est, depth_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter, cost_type="step"):
    """pose_error.vsd after its two renders, in torch float64 on the tensors' device: depth_est [B,H,W], depth_gt and
    depth_test [H,W].  Returns float64 [B, len(taus)]."""
    import torch
    K = np.asarray(K, np.float64).reshape(3, 3)
    dist_test, dist_gt, dist_est = dist_image(depth_test, K), dist_image(depth_gt, K), dist_image(depth_est, K)
    visib_gt = visibility_mask(dist_test, dist_gt, delta)
    visib_est = visibility_mask(dist_test, dist_est, delta) | (visib_gt & (dist_est > 0))
    inter, union = visib_gt & visib_est, visib_gt | visib_est
    union_count = union.flatten(-2).sum(-1).to(torch.float64)
    comp_count = union_count - inter.flatten(-2).sum(-1)
    dists = (dist_gt - dist_est).abs()
    if normalized_by_diameter:
        dists = dists / diameter
    errors = []
    for tau in taus:
        if cost_type == "step":
            costs = (dists >= tau).to(torch.float64)
        elif cost_type == "tlinear":
            costs = (dists / tau).clamp(max=1.0)
        else:
            raise ValueError("Unknown pixel matching cost.")
        total = torch.where(inter, costs, torch.zeros_like(costs)).flatten(-2).sum(-1)
        errors.append(torch.where(union_count > 0, (total + comp_count) / union_count.clamp(min=1.0), torch.ones_like(total)))
    return torch.stack(errors, -1)


def vsd(R_est, t_est, R_gt, t_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter, meshes: MeshSet, obj_id,
        cost_type="step", near: float = DEFAULT_NEAR, render=None):
    """Visible Surface Discrepancy with pose_error.vsd's signature, the renderer replaced by the mesh set.  ``R_est`` [3,3]
    with ``t_est`` [3] / [3,1] gives the toolkit's list of errors (one per tau); a batch [B,3,3] / [B,3] against the one
    test image gives a float64 tensor [B, len(taus)].  The B + 1 renders are one pgr_mesh_depth call, the rest torch ops
    on the device.  ``render``: a callable (jobs, K, size) -> depths [J,H,W] used instead of render_depth."""
    import torch
    R_est = np.asarray(R_est, np.float64)
    single = R_est.ndim == 2
    R_est = R_est.reshape(-1, 3, 3)
    t_est = np.asarray(t_est, np.float64).reshape(-1, 3)
    depth_test = torch.as_tensor(depth_test)
    H, W = depth_test.shape
    jobs = [(obj_id, R, t) for R, t in zip(R_est, t_est)] + [(obj_id, np.asarray(R_gt, np.float64).reshape(3, 3),
                                                              np.asarray(t_gt, np.float64).reshape(3))]
    if render is None:
        depths = render_depth(meshes, jobs, K, (W, H), near=near)
    else:
        depths = torch.as_tensor(render(jobs, K, (W, H)))
    depth_test = depth_test.to(depths.device)
    errors = vsd_from_depths(depths[:-1], depths[-1], depth_test, K, delta, taus, normalized_by_diameter, diameter, cost_type)
    return [float(e) for e in errors[0].cpu()] if single else errors


# ---- a dataset on disk ----------------------------------------------------------------------------------------------
def recompute_dataset(dataset_dir, models_dir, delta: float = 15.0, translation_scale: float = 1.0, batch: int = 8,
                      device="cuda"):
    """mask/, mask_visib/ and scene_gt_info.json of every scene under <dataset>/train, from the meshes of ``models_dir``
    (millimetres), scene_gt.json, scene_camera.json and the depth images: calc_gt_info.py plus calc_gt_masks.py."""
    meshes = MeshSet.from_dir(models_dir, device=device, scale=BD.unit_of(translation_scale))
    scenes = BD.scene_dirs(dataset_dir, "train")
    for scene in map(BD.BopScene, scenes):
        gt, cam, ids = scene.gt, scene.camera, scene.image_ids
        info = {}
        scene.make_dirs(("mask", "mask_visib"))
        for b0 in range(0, len(ids), batch):
            chunk = ids[b0:b0 + batch]
            depth = np.stack([scene.read_png("depth", i).astype(np.float32) for i in chunk])
            masks, visibs, infos = gt_from_meshes(meshes, {str(k): gt[i] for k, i in enumerate(chunk)},
                                                  {str(k): cam[i] for k, i in enumerate(chunk)}, depth, delta=delta,
                                                  translation_scale=translation_scale)
            for k, i in enumerate(chunk):
                info[i] = infos[k]
                for name, stack in (("mask", masks[k]), ("mask_visib", visibs[k])):
                    for o, image in enumerate((stack * 255).cpu().numpy()):
                        scene.image_path(name, i, o).write_bytes(BD.encode_png(image))
        scene.write_json(BD.SCENE_GT_INFO, {k: info[k] for k in ids})
    return scenes


def visualize_dataset(dataset_dir, models_dir, out_dir, results=None, resolve_visib: bool = False, shading: str = "phong",
                      translation_scale: float = 1.0, device="cuda", textures: bool = False, texture_filter: str = "nearest") -> int:
    """The toolkit's vis_gt_poses.py (or, with ``results`` = a BOP results file, vis_est_poses.py): for every image of every
    scene under <dataset>/train the models at the ground-truth poses (or at the file's estimates for that scene and image)
    shaded over the photograph, written to <out>/<scene>/<image>.png.  ``textures``: models that name a texture are drawn with
    it.  Returns the number of images written."""
    unit = BD.unit_of(translation_scale)
    meshes = MeshSet.from_dir(models_dir, device=device, scale=unit, compute_normals=shading == "phong", textures=textures)
    ests = None
    if results is not None:
        from .pose_eval import read_results
        ests = {}
        for e in read_results(results):
            ests.setdefault((e["scene_id"], e["im_id"]), []).append(dict(obj_id=e["obj_id"], R=e["R"], t=e["t"] * unit))
    written = 0
    for scene in map(BD.BopScene, BD.scene_dirs(dataset_dir, "train")):
        for i in scene.image_ids:
            if ests is None:
                poses = [dict(obj_id=int(e["obj_id"]), R=BD.pose_of(e)[0], t=BD.pose_of(e)[1]) for e in scene.gt[i]]
            else:
                poses = ests.get((int(scene.path.name), int(i)), []) if scene.path.name.isdigit() else []
            rgb = scene.read_image("rgb", i)
            if rgb.ndim == 2:
                rgb = np.repeat(rgb[:, :, None], 3, 2)
            vis_object_poses(poses, BD.cam_K(scene.camera[i]), meshes, rgb=rgb, vis_rgb_path=Path(out_dir) / scene.path.name / BD.image_name(i),
                             vis_rgb_resolve_visib=resolve_visib, shading=shading, texture_filter=texture_filter)
            written += 1
    return written


def main(argv: Optional[Sequence[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m pegasus_amd.mesh_render", description=__doc__.split("\n\n")[0])
    p.add_argument("--dataset", required=True)
    p.add_argument("--models", required=True)
    p.add_argument("--delta", type=float, default=15.0, help="visibility tolerance in millimetres (calc_gt_masks.py's default)")
    p.add_argument("--translation_scale", type=float, default=1.0,
                   help="what scene_gt's translations were written with: 1 = metres, 1000 = millimetres")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--vis", metavar="DIR", help="instead, write <DIR>/<scene>/<image>.png: the models shaded over every photograph "
                                               "at the ground-truth poses (the toolkit's vis_gt_poses.py)")
    p.add_argument("--results", help="with --vis: a BOP results file whose estimates are drawn instead (vis_est_poses.py)")
    p.add_argument("--resolve_visib", action="store_true", help="with --vis: only the nearest object shows at each pixel")
    p.add_argument("--shading", choices=("flat", "phong"), default="phong", help="with --vis")
    p.add_argument("--textures", action="store_true", help="with --vis: models whose PLY names a texture image are drawn with it")
    p.add_argument("--texture_filter", choices=sorted(TEXTURE_FILTERS), default="nearest", help="with --vis --textures")
    a = p.parse_args(argv)
    if a.vis:
        n = visualize_dataset(a.dataset, a.models, a.vis, a.results, a.resolve_visib, a.shading, a.translation_scale,
                              textures=a.textures, texture_filter=a.texture_filter)
        print(f"wrote {n} visualisation(s) under {a.vis}")
        return 0
    scenes = recompute_dataset(a.dataset, a.models, a.delta, a.translation_scale, a.batch)
    print(f"recomputed mask/, mask_visib/ and scene_gt_info.json of {len(scenes)} scene(s)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

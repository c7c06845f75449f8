"""Times the textured resolve pass against the plain one, the three stages of a texture bake, and measures what the texture buys
in a held-out view.

    python scripts/mesh_texture_bench.py [out.json]            (default: profiles/mesh_texture_bench.json)

  shade    pgr_mesh_shade_textured (nearest and bilinear, rgb only) against pgr_mesh_shade (rgb only, vertex colours) on the same
           jobs and the same keys of one pgr_mesh_visibility call: 32 jobs of a bumpy sphere decimated to about 0.1 M faces, one
           640 x 480 canvas each, and one job on a 2400 x 2400 canvas.  The texture is the mesh's per-face atlas at cell 8 filled
           with random bytes.  The three are timed in turn, ROUNDS times; a figure is the median over the rounds of the median
           of REPS hipEvent pairs after a warm-up, the spread the largest minus the smallest round.
  bake     mesh.bake_views on a 25 k-face decimation of the coloured box object's mesh at cell 16 from 97 views of 512 x 512:
           the milliseconds of pgr_mesh_atlas_points, pgr_mesh_vertex_colors on the texel points and pgr_mesh_atlas_pack (hipEvents
           around each, median of REPS after a warm-up), and of rendering the views.
  error    the mean absolute colour error of a held-out Gaussian view against the box's mesh decimated to 2.5 % of its faces,
           rendered (a) grey, (b) with vertex colours (mesh.colorize) and (c) textured (mesh.bake_texture, cell 16), nearest and
           bilinear, over the pixels both cover: the comparison of section 21.
Prints every stage as it finishes."""
import argparse
import ctypes as C
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from mesh_depth_bench import bumpy_sphere                 # noqa: E402
from pegasus_amd import _lib, decimate as D, mesh as M, mesh_render as R        # noqa: E402

DEV = torch.device("cuda")
REPS, ROUNDS = 5, 5
BOX_DIMS = (0.06, 0.16, 0.21)


def stage(msg):
    print(msg, flush=True)


def events(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def rounds_of(fns: dict) -> dict:
    """name -> {median_ms, min_ms, max_ms, spread_ms} over ROUNDS rounds in which the functions are timed in turn."""
    got = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            got[k].append(events(fn))
    out = {}
    for k, r in got.items():
        r = sorted(r)
        out[k] = dict(median_ms=r[len(r) // 2], min_ms=r[0], max_ms=r[-1], spread_ms=r[-1] - r[0], rounds=ROUNDS, reps=REPS)
    return out


def shade_bench():
    from scipy.spatial.transform import Rotation as Rot
    L = _lib.lib()
    stage("marching a bumpy sphere at grid 256 and decimating it to about 100 k faces")
    mesh = D.simplify_to(bumpy_sphere(256, 0), 100_000)[0]
    F = len(mesh.faces)
    cell = 8
    width, height, _cols, _rows, corner_uv = M.texture_atlas_layout(F, cell)
    rng = np.random.default_rng(1)
    mesh = M.Mesh(mesh.vertices, mesh.faces, corner_uv=corner_uv, texture=rng.integers(0, 256, (height, width, 3)).astype(np.uint8))
    meshes = R.MeshSet({1: mesh}, device=DEV, textures=True, compute_normals=True)
    g = torch.Generator(device="cpu").manual_seed(5)
    meshes.colors = torch.rand(meshes.vertices.shape, generator=g).to(DEV)
    records = []
    for label, n_jobs, W, H, z in (("32 jobs at 640 x 480", 32, 640, 480, (0.5, 0.8)), ("one job at 2400 x 2400", 1, 2400, 2400, (0.42, 0.42))):
        K = np.array([[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1.0]])
        jobs = [(1, Rot.random(random_state=int(rng.integers(1 << 30))).as_matrix(),
                 np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(*z)])) for _ in range(n_jobs)]
        arr = R.mesh_jobs(meshes, jobs, K)
        mesh_args = (_lib.ptr(meshes.vertices), meshes.vertices.shape[0], _lib.ptr(meshes.faces), meshes.faces.shape[0], n_jobs, arr, W, H,
                     float(R.DEFAULT_NEAR))
        keys = torch.empty((n_jobs, H, W), dtype=torch.int64, device=DEV)
        count = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = _lib.workspace("pgr_mesh_visibility", DEV, n_jobs, arr)
        _lib.call("pgr_mesh_visibility", DEV, *mesh_args, _lib.ptr(keys), n_jobs, _lib.ptr(count), _lib.ptr(ws), ws.numel())
        rgb = torch.empty((n_jobs, H, W, 3), dtype=torch.float32, device=DEV)
        shade = _lib.PgrMeshShade(normals=_lib.ptr(meshes.normals), colors=_lib.ptr(meshes.colors), surf_colors=None,
                                  light=(C.c_float * 3)(0.0, 0.0, 0.0), ambient=0.5, bg=(C.c_float * 3)(0.0, 0.0, 0.0), rgb=_lib.ptr(rgb))
        table = (_lib.PgrMeshTexture * 1)(_lib.PgrMeshTexture(offset=0, width=width, height=height))
        which = (C.c_int32 * n_jobs)(*([0] * n_jobs))
        ws_plain = _lib.workspace("pgr_mesh_shade", DEV, n_jobs, arr)
        ws_tex = _lib.workspace("pgr_mesh_shade_textured", DEV, n_jobs, arr)

        def textured(filt):
            tex = _lib.PgrMeshTextures(corner_uv=_lib.ptr(meshes.corner_uv), texels=_lib.ptr(meshes.texels), texel_bytes=meshes.texels.numel(),
                                       n_textures=1, textures=table, job_texture=which, filter=filt, uv=None)
            return lambda: _lib.call("pgr_mesh_shade_textured", DEV, *mesh_args, _lib.ptr(keys), n_jobs, C.byref(shade), C.byref(tex),
                                     _lib.ptr(ws_tex), ws_tex.numel())

        fns = {"plain": lambda: _lib.call("pgr_mesh_shade", DEV, *mesh_args, _lib.ptr(keys), n_jobs, C.byref(shade), _lib.ptr(ws_plain),
                                          ws_plain.numel()),
               "nearest": textured(_lib.PGR_TEXTURE_NEAREST), "bilinear": textured(_lib.PGR_TEXTURE_BILINEAR)}
        rec = dict(workload=label, faces=F, atlas=[width, height], covered_share=float((keys != 0).float().mean()), **rounds_of(fns))
        for k in ("nearest", "bilinear"):
            rec[f"{k}_over_plain"] = rec[k]["median_ms"] / rec["plain"]["median_ms"]
        stage(f"shade: {json.dumps(rec)}")
        records.append(rec)
        del keys, rgb
    return records


def coloured_box_model(seed=11, n=40_000):
    """The test object of section 21: a box of opaque Gaussians, each coloured by the box face it lies on (channels 0.1 or 0.9)."""
    from pegasus_amd import scenes
    from pegasus_amd.gaussian_model import GaussianModel
    cloud = scenes.box_object(np.random.default_rng(seed), n, BOX_DIMS, math.log(0.002), 0.4, 0.15, object_id=1)
    half = 0.5 * np.asarray(BOX_DIMS)
    axis = np.abs(np.abs(cloud.xyz) - half[None, :]).argmin(axis=1)
    face = 2 * axis + (cloud.xyz[np.arange(n), axis] > 0)
    palette = np.array([[0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.1, 0.1, 0.9], [0.9, 0.9, 0.1], [0.9, 0.1, 0.9], [0.1, 0.9, 0.9]])
    f_dc = ((palette[face] - 0.5) / 0.28209479177387814).astype(np.float32).reshape(n, 1, 3)
    return GaussianModel.from_arrays(cloud.xyz, f_dc, np.zeros((n, 0, 3), np.float32), np.full((n, 1), 4.0, np.float32), cloud.scaling,
                                     cloud.rotation, sh_degree=0)


def held_out_view(image_size=320):
    from pegasus_amd import graphics as G
    from pegasus_amd.rasterizer import ViewSpec
    from pegasus_amd.scenes import make_view
    eye = 0.55 * np.array([0.55, -0.62, 0.56]) / np.linalg.norm([0.55, -0.62, 0.56])
    Rm, t = G.look_at_opencv(tuple(eye), (0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
    fov = math.radians(32.0)
    v = make_view(Rm, t, image_size, image_size, fovx=fov, fovy=fov)
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")
    spec = ViewSpec(image_size, image_size, v.tanfovx, v.tanfovy, dev(np.zeros(3)), dev(v.world_view_transform), dev(v.full_proj_transform),
                    dev(v.camera_center), depth_mode=1)
    f = image_size / (2.0 * v.tanfovx)
    K = np.array([[f, 0, image_size / 2.0], [0, f, image_size / 2.0], [0, 0, 1]])
    return spec, np.asarray(Rm, np.float64), np.asarray(t, np.float64), K


def bake_bench(model, full):
    stage("bake: decimating to about 25 k faces, rendering 97 views of 512 x 512")
    mesh = D.simplify_to(full, 25_000)[0]
    lo, hi = M._model_bounds(model, None)
    views, _r, _fov = M.sphere_views(0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo)), 97, 512)
    render_ms = {}
    depth, final_T, color = M.render_views(model, views, render_ms, want_color=True)
    tol = 2.0 * float((hi - lo).max()) / 255.0
    runs = []
    for _ in range(REPS + 1):
        ms, info = {}, {}
        M.bake_views(mesh, color, depth, final_T, views, cell=16, depth_tol=tol, stage_ms=ms, info=info)
        runs.append(ms)
    med = lambda k: sorted(r[k] for r in runs[1:])[REPS // 2]
    rec = dict(faces=len(mesh.faces), cell=16, atlas=list(info["atlas"]), views=97, image_size=512, render_ms=render_ms["render"],
               atlas_points_ms=med("atlas_points"), atlas_colors_ms=med("atlas_colors"), atlas_pack_ms=med("atlas_pack"), reps=REPS,
               faces_seen=int((info["face_seen"] > 0).sum()))
    stage(f"bake: {json.dumps(rec)}")
    return rec


def error_bench(model, full):
    from pegasus_amd.rasterizer import forward_views
    small = D.simplify_to(full, int(0.025 * len(full.faces)))[0]
    stage(f"error: {len(full.faces)} -> {len(small.faces)} faces")
    coloured = M.colorize(model, small)
    info = {}
    baked = M.bake_texture(model, M.Mesh(small.vertices, small.faces, normals=coloured.normals, colors=coloured.colors), cell=16, info=info)
    spec, Rm, t, K = held_out_view()
    r = forward_views(model.get_xyz.detach(), model.get_opacity.detach(), [spec], shs=model.get_features.detach(),
                      scales=model.get_scaling.detach(), rotations=model.get_rotation.detach(), sh_degree=0, want_radii=False, want_aux=True)[0]
    alpha = (1.0 - r["final_T"]).reshape(spec.image_height, spec.image_width)
    truth = (r["color"] / alpha.clamp_min(1e-6)[None]).permute(1, 2, 0)
    size = (spec.image_width, spec.image_height)
    rec = dict(faces_full=len(full.faces), faces=len(small.faces), cell=16, atlas=list(info["atlas"]), image_size=spec.image_width,
               faces_seen=int((info["face_seen"] > 0).sum()))
    grey = M.Mesh(small.vertices, small.faces, normals=coloured.normals)
    for label, mesh, textures, filt in (("grey", grey, False, "nearest"), ("vertex_colours", coloured, False, "nearest"),
                                        ("textured_nearest", baked, True, "nearest"), ("textured_bilinear", baked, True, "bilinear")):
        out = R.render(R.MeshSet({1: mesh}, device=DEV, textures=textures), [(1, Rm, t)], K, size, outputs=("rgb", "depth"), ambient=1.0,
                       texture_filter=filt)
        both = (out["depth"][0] > 0) & (alpha > 0.9)
        rec[label] = dict(mean_abs_error=float((out["rgb"][0][both] - truth[both]).abs().mean()), pixels=int(both.sum()))
    stage(f"error: {json.dumps(rec)}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=str(ROOT / "profiles" / "mesh_texture_bench.json"))
    ap.add_argument("--only", choices=("shade", "bake", "error"), default=None)
    a = ap.parse_args()
    _lib.lib()
    record = {}
    if a.only in (None, "shade"):
        record["shade"] = shade_bench()
    if a.only in (None, "bake", "error"):
        model = coloured_box_model()
        stage("extracting the box's mesh at grid 256")
        full = M.extract_mesh(model, resolution=256)
        if a.only in (None, "bake"):
            record["bake"] = bake_bench(model, full)
        if a.only in (None, "error"):
            record["error"] = error_bench(model, full)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()

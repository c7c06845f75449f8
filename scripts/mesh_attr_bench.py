"""Times the two vertex-attribute entries: pgr_mesh_vertex_normals and pgr_mesh_vertex_colors.

    python scripts/mesh_attr_bench.py [out.json]         (default: profiles/mesh_attr_bench.json)

Workload: the bumpy sphere of the other mesh benchmarks, marched at grid 256 (about 0.9 M faces, 0.2 units across), and the
views of 512^2 that extract_mesh renders by default (mesh.sphere_views(..., 96, 512) around the mesh's box: 97 views).  The images are made from the
mesh itself: depth by pgr_mesh_depth from every view, final_T 0 where the mesh is hit and 1 elsewhere, colour a smooth pattern
times alpha.  Tensors, cameras and the workspace are built beforehand; a figure is the median of 5 hipEvent pairs after a
warm-up around the library call alone.  Beside them stands the host rule the normals replace (mesh_render.vertex_normals:
float64, np.add.at), timed once on the same mesh, and how far the two results lie apart."""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from mesh_depth_bench import bumpy_sphere                 # noqa: E402
from pegasus_amd import _lib, mesh as M, mesh_render as R            # noqa: E402
from pegasus_amd.rasterizer import camera_structs         # noqa: E402

DEV = torch.device("cuda")
REPS = 5
GRID, VIEWS, SIZE = 256, 96, 512


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
    return dict(min_ms=out[0], median_ms=out[len(out) // 2], max_ms=out[-1], reps=REPS)


def images_of(mesh, views):
    """(color [V,3,H,W], depth [V,H,W], final_T [V,H,W]) of ``mesh`` seen from ``views``, on the device."""
    meshes = R.MeshSet({1: mesh}, device=DEV)
    jobs = []
    for v in views:
        m = v.viewmatrix.detach().cpu().numpy().astype(np.float64).reshape(4, 4)
        jobs.append((1, m[:3, :3].T, m[3, :3]))
    f = SIZE / (2.0 * float(views[0].tanfovx))
    K = np.array([[f, 0, SIZE / 2.0], [0, f, SIZE / 2.0], [0, 0, 1.0]])          # the mesh renderer's pixel i samples i + 0.5
    depth = R.render_depth(meshes, jobs, K, (SIZE, SIZE), near=0.05)
    alpha = (depth > 0).float()
    yy, xx = torch.meshgrid(torch.arange(SIZE, device=DEV), torch.arange(SIZE, device=DEV), indexing="ij")
    k = torch.arange(len(views), device=DEV).float()[:, None, None, None]
    c = torch.arange(3, device=DEV).float()[None, :, None, None]
    base = 0.5 + 0.4 * torch.sin(0.05 * xx[None, None] + 0.7 * c + 0.3 * k) * torch.cos(0.04 * yy[None, None] - 0.2 * c)
    return (alpha[:, None] * base).contiguous(), depth.contiguous(), (1.0 - alpha).contiguous()


def main():
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "mesh_attr_bench.json"
    L = _lib.lib()
    stage(f"marching the bumpy sphere at grid {GRID}")
    mesh = bumpy_sphere(GRID, 0)
    V, F = len(mesh.vertices), len(mesh.faces)
    lo, hi = mesh.vertices.min(axis=0).astype(np.float64), mesh.vertices.max(axis=0).astype(np.float64)
    views, radius, fov = M.sphere_views(0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo)), VIEWS, SIZE)
    rec = dict(vertices=V, faces=F, views=len(views), size=SIZE, view_radius=radius, fov_deg=float(np.degrees(fov)))
    stage(json.dumps(rec))
    stream = _lib.stream_ptr(DEV)
    vert = torch.from_numpy(mesh.vertices).to(DEV)
    face = torch.from_numpy(mesh.faces).to(DEV)
    normals = torch.empty((V, 3), dtype=torch.float32, device=DEV)
    nb = int(L.pgr_mesh_vertex_normals_workspace_bytes(V))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)

    def run_normals():
        _lib.check(L.pgr_mesh_vertex_normals(V, _lib.ptr(vert), F, _lib.ptr(face), _lib.ptr(normals), _lib.ptr(ws), nb, stream),
                   "pgr_mesh_vertex_normals")
    rec["normals"] = events(run_normals)
    rec["normals"]["atomics"] = 9 * F
    stage(f"normals {rec['normals']}")
    t0 = time.perf_counter()
    host = R.vertex_normals(mesh.vertices, mesh.faces)
    rec["host_vertex_normals_ms"] = 1e3 * (time.perf_counter() - t0)
    rec["normals_max_abs_difference_to_host"] = float(np.abs(normals.cpu().numpy().astype(np.float64) - host).max())
    stage(f"host vertex_normals {rec['host_vertex_normals_ms']:.1f} ms, "
          f"largest difference {rec['normals_max_abs_difference_to_host']:.3g}")

    color, depth, final_T = images_of(mesh, views)
    cams, keep = camera_structs(views, DEV)
    colors = torch.empty((V, 3), dtype=torch.float32, device=DEV)
    seen = torch.empty((V,), dtype=torch.int32, device=DEV)
    fill = (C.c_float * 3)(0.5, 0.5, 0.5)
    depth_tol = 2.0 * float((hi - lo).max()) / (GRID - 1)

    def run_colors(with_normals):
        def fn():
            _lib.check(L.pgr_mesh_vertex_colors(V, _lib.ptr(vert), _lib.ptr(normals) if with_normals else None, len(views), cams,
                                                _lib.ptr(color), _lib.ptr(depth), _lib.ptr(final_T), depth_tol, 0.5, 0.3, fill,
                                                _lib.ptr(colors), _lib.ptr(seen), stream), "pgr_mesh_vertex_colors")
        return fn
    for label, with_normals in (("colors", True), ("colors_without_normals", False)):
        rec[label] = events(run_colors(with_normals))
        s = seen.cpu().numpy()
        rec[label].update(unseen_share=float((s == 0).mean()), mean_views_per_vertex=float(s.mean()),
                          pairs_per_second=V * len(views) / (1e-3 * rec[label]["median_ms"]))
        stage(f"{label} {rec[label]}")
    del keep
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

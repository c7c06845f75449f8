"""Times the visibility pass and the resolve pass of the shaded mesh renderer against pgr_mesh_depth.

    python scripts/mesh_shade_bench.py [out.json] [--parent-lib <libpegasus_raster.so of the parent commit>]
                                       (default: profiles/mesh_shade_bench.json)

Workloads, as section 11's: 8 objects x 32 views at 800^2 = 256 jobs, two mesh sizes: marching-tetrahedra bumpy spheres
(mesh.march at grid 256, about 0.9 M faces each, 0.2 units across, seen from 0.8 to 1.3 units) and their decimations to about
35 k faces (decimate.simplify_to: a models_eval mesh).  Random unit normals and random colours per vertex.  Job arrays,
workspaces and outputs are built beforehand; a figure is the median of 5 hipEvent pairs after a warm-up around the library
calls of the whole batch alone.

  depth       pgr_mesh_depth, one canvas per job, 64 jobs per call (section 11's timing).  With --parent-lib the parent
              commit's library is loaded beside this one and the two are timed in turn, ROUNDS times each: the medians of
              the rounds and their spread (max - min) are recorded for both.
  visibility  pgr_mesh_visibility with the same jobs and canvases (uint64 keys), and its ratio to this build's depth.
  resolve     pgr_mesh_shade on those keys, rgb only and all six outputs, smooth normals and vertex colours.
  per_image   the same jobs with the 8 objects of a view sharing one canvas (32 canvases, one call of 256 jobs): visibility,
              resolve (rgb only / all outputs).
Prints every stage as it finishes."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from mesh_depth_bench import bumpy_sphere                 # noqa: E402
from pegasus_amd import _lib, decimate as D, mesh_render as R        # noqa: E402

DEV = torch.device("cuda")
REPS, ROUNDS = 5, 5
OBJECTS, VIEWS, SIZE, CHUNK = 8, 32, 800, 64
EVAL_FACES = 35_000
ALL = ("depth", "face_id", "job_id", "xyz", "normal", "rgb")


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


def parent_library(path):
    """The parent commit's build, bound for the two entries timed here only (it lacks the newer ones)."""
    lib = C.CDLL(str(path))
    size, arg = _lib.SYMBOLS["pgr_mesh_depth_workspace_bytes"], _lib.SYMBOLS["pgr_mesh_depth"]
    lib.pgr_mesh_depth_workspace_bytes.restype, lib.pgr_mesh_depth_workspace_bytes.argtypes = size
    lib.pgr_mesh_depth.restype, lib.pgr_mesh_depth.argtypes = arg
    return lib


def attributes(meshes, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = torch.randn(meshes.vertices.shape, generator=g)
    meshes.normals = (n / n.norm(dim=1, keepdim=True)).to(DEV)
    meshes.colors = torch.rand(meshes.vertices.shape, generator=g).to(DEV)


def make_jobs(seed=3):
    from scipy.spatial.transform import Rotation as Rot
    rng = np.random.default_rng(seed)
    jobs = []
    for _v in range(VIEWS):
        for k in range(OBJECTS):
            t = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(0.8, 1.3)])
            jobs.append((k + 1, Rot.random(random_state=int(rng.integers(1 << 30))).as_matrix(), t))
    return jobs


def measure(name, meshes, jobs, parent):
    L = _lib.lib()
    W = H = SIZE
    K = np.array([[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1.0]])
    stream = _lib.stream_ptr(DEV)
    near = float(R.DEFAULT_NEAR)
    mesh_args = (_lib.ptr(meshes.vertices), meshes.vertices.shape[0], _lib.ptr(meshes.faces), meshes.faces.shape[0])
    rec = dict(mesh=name, faces_per_mesh=int(np.mean([r[3] for r in meshes.ranges.values()])), jobs=len(jobs), size=SIZE)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)

    def calls_of(slots, chunk):
        out = []
        for j0 in range(0, len(jobs), chunk):
            part = jobs[j0:j0 + chunk]
            arr = R.mesh_jobs(meshes, part, K, (0, 0), slots=[s - slots[j0] for s in slots[j0:j0 + chunk]])
            nb = int(L.pgr_mesh_visibility_workspace_bytes(len(part), arr))
            nb2 = int(L.pgr_mesh_shade_workspace_bytes(len(part), arr))
            out.append((len(part), arr, torch.empty(nb, dtype=torch.uint8, device=DEV), nb, torch.empty(nb2, dtype=torch.uint8, device=DEV), nb2))
        return out

    def shade_struct(bufs):
        return _lib.PgrMeshShade(normals=_lib.ptr(meshes.normals), colors=_lib.ptr(meshes.colors), surf_colors=None,
                                 light=(C.c_float * 3)(0.0, 0.0, 0.0), ambient=0.5, bg=(C.c_float * 3)(0.0, 0.0, 0.0),
                                 **{k: _lib.ptr(v) for k, v in bufs.items()})

    def buffers(names, n_slots):
        shape = lambda ch: (n_slots, H, W) + ((ch,) if ch else ())
        return {k: torch.empty(shape(R.RENDER_OUTPUTS[k][1]), dtype=getattr(torch, R.RENDER_OUTPUTS[k][0]), device=DEV) for k in names}

    # one canvas per job, CHUNK jobs per call
    calls = calls_of(list(range(len(jobs))), CHUNK)
    depth = torch.empty((CHUNK, H, W), dtype=torch.float32, device=DEV)
    keys = torch.empty((CHUNK, H, W), dtype=torch.int64, device=DEV)

    def run_depth(lib):
        def fn():
            for n, arr, ws, nb, _ws2, _nb2 in calls:
                _lib.check(lib.pgr_mesh_depth(*mesh_args, n, arr, W, H, near, _lib.ptr(depth), CHUNK, _lib.ptr(count), _lib.ptr(ws), nb, stream),
                           "pgr_mesh_depth")
        return fn

    def run_visibility(cs, k, n_slots):
        def fn():
            for n, arr, ws, nb, _ws2, _nb2 in cs:
                _lib.check(L.pgr_mesh_visibility(*mesh_args, n, arr, W, H, near, _lib.ptr(k), n_slots, _lib.ptr(count), _lib.ptr(ws), nb, stream),
                           "pgr_mesh_visibility")
        return fn

    def run_shade(cs, k, n_slots, struct):
        def fn():
            for n, arr, _ws, _nb, ws2, nb2 in cs:
                _lib.check(L.pgr_mesh_shade(*mesh_args, n, arr, W, H, near, _lib.ptr(k), n_slots, C.byref(struct), _lib.ptr(ws2), nb2, stream),
                           "pgr_mesh_shade")
        return fn

    builds = [("this", L)] + ([("parent", parent)] if parent is not None else [])
    rounds = {b: [] for b, _ in builds}
    for _ in range(ROUNDS if parent is not None else 1):
        for b, lib in builds:
            rounds[b].append(events(run_depth(lib))["median_ms"])
    for b, _ in builds:
        r = sorted(rounds[b])
        rec[f"depth_{b}"] = dict(median_ms=r[len(r) // 2], min_ms=r[0], max_ms=r[-1], spread_ms=r[-1] - r[0], rounds=len(r))
    stage(f"{name}: depth {json.dumps({b: rec[f'depth_{b}'] for b, _ in builds})}")
    rec["visibility"] = events(run_visibility(calls, keys, CHUNK))
    rec["visibility_over_depth"] = rec["visibility"]["median_ms"] / rec["depth_this"]["median_ms"]
    if parent is not None:
        rec["visibility_over_parent_depth"] = rec["visibility"]["median_ms"] / rec["depth_parent"]["median_ms"]
        rec["depth_over_parent_depth"] = rec["depth_this"]["median_ms"] / rec["depth_parent"]["median_ms"]
    stage(f"{name}: visibility {rec['visibility']} = {rec['visibility_over_depth']:.3f} x depth")
    for label, names in (("resolve_rgb", ("rgb",)), ("resolve_all", ALL)):
        bufs = buffers(names, CHUNK)
        rec[label] = events(run_shade(calls, keys, CHUNK, shade_struct(bufs)))
        if label == "resolve_all":
            rec["covered_share_last_call"] = float((bufs["job_id"] >= 0).float().mean())
        del bufs
        stage(f"{name}: {label} {rec[label]}")
    del depth, keys
    # the objects of a view share a canvas: one call
    slots = [k // OBJECTS for k in range(len(jobs))]
    one = calls_of(slots, len(jobs))
    keys = torch.empty((VIEWS, H, W), dtype=torch.int64, device=DEV)
    per = dict(canvases=VIEWS, visibility=events(run_visibility(one, keys, VIEWS)))
    for label, names in (("resolve_rgb", ("rgb",)), ("resolve_all", ALL)):
        bufs = buffers(names, VIEWS)
        per[label] = events(run_shade(one, keys, VIEWS, shade_struct(bufs)))
        if label == "resolve_all":
            per["covered_share"] = float((bufs["job_id"] >= 0).float().mean())
        del bufs
    rec["per_image"] = per
    stage(f"{name}: per image {json.dumps(per)}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=str(ROOT / "profiles" / "mesh_shade_bench.json"))
    ap.add_argument("--parent-lib")
    a = ap.parse_args()
    _lib.lib()                                                   # after torch: one HIP runtime in the process
    parent = parent_library(a.parent_lib) if a.parent_lib else None
    stage("marching 8 bumpy spheres at grid 256")
    full = {k + 1: bumpy_sphere(256, k) for k in range(OBJECTS)}
    stage(f"decimating to about {EVAL_FACES} faces")
    small = {k: D.simplify_to(m, EVAL_FACES)[0] for k, m in full.items()}
    jobs = make_jobs()
    records = []
    for name, set_ in (("models_eval", small), ("extracted", full)):
        meshes = R.MeshSet(set_, device=DEV)
        attributes(meshes, 5)
        records.append(measure(name, meshes, jobs, parent))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(records, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Times of the environment field on one GPU ("Measured"): pgr_sdf_from_tsdf at 96^3 and at 200 x 200 x 104
(a carved volume that holds a floor slab with a box on it), and what the ground as a field costs per step against the plane on
the six-body worlds of scripts/rigid_bench.py (the bodies fall onto a flat field, z sampled on a 24 x 24 x 16 grid, which the
trilinear rule reproduces: the same contacts as the plane's).  Device events, medians of 7 after 2 warm-up calls, with the range.
These are recorded numbers, not thresholds.

    python scripts/environment_bench.py [--out profiles/environment_bench.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np


def timed(fn, warm, reps):
    import torch
    times = []
    for k in range(warm + reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        if k >= warm:
            times.append(start.elapsed_time(stop))
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), reps=reps), out


def slab_volume(shape, truncation_voxels=4.0):
    """float32 [nz,ny,nx]: clip(d / truncation) of a floor at a quarter of the height with a box on it, in voxel units, the
    outermost layer outside."""
    nx, ny, nz = shape
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float32), np.arange(ny, dtype=np.float32), np.arange(nx, dtype=np.float32), indexing="ij")
    floor = k - (0.25 * nz + 0.4)
    q = np.stack([np.abs(i - 0.5 * nx) - 0.2 * nx, np.abs(j - 0.5 * ny) - 0.15 * ny, np.abs(k - 0.25 * nz) - (0.3 * nz + 0.3)])
    box = np.linalg.norm(np.maximum(q, 0.0), axis=0) + np.minimum(q.max(0), 0.0)
    t = np.clip(np.minimum(floor, box) / truncation_voxels, -1.0, 1.0).astype(np.float32)
    t[[0, -1]], t[:, [0, -1]], t[:, :, [0, -1]] = 1.0, 1.0, 1.0
    return t


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "environment_bench.json"))
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("environment_bench needs a HIP device: there is no CPU path and no time to report without one")
    import dynamics_cases as DC
    from pegasus_amd import _lib, collision as COL, dynamics as DYN, environment as ENV
    from pegasus_amd.mesh import Grid, Mesh
    import ctypes as C

    fields = {}
    for shape in ((96, 96, 96), (200, 200, 104)):
        grid = Grid(*shape, (0.0, 0.0, 0.0), 0.01)
        t = torch.from_numpy(slab_volume(shape)).cuda()
        sdf = torch.empty_like(t)
        ws = _lib.workspace("pgr_sdf_from_tsdf", t.device, *shape)
        g = grid.struct()
        r, _ = timed(lambda: _lib.call("pgr_sdf_from_tsdf", t.device, C.byref(g), _lib.ptr(t), _lib.ptr(sdf), None, _lib.ptr(ws), ws.numel()),
                     a.warm, a.reps)
        r.update(shape=list(shape), points=int(np.prod(shape)), solid=int((t < 0).sum()), workspace_bytes=int(ws.numel()))
        fields["x".join(map(str, shape))] = r
        print(shape, r)

    def body(name):
        m = Mesh(*DC.mesh(name))
        return DYN.RigidBody.from_collision(COL.CollisionBody(m, COL.MeshSDF.from_mesh(m, resolution=DC.RESOLUTION), shell=DC.shell(name)))
    table = [body(n) for n in ("cube", "l_prism", "small_cube")]
    params = DYN.Params(gravity=DC.GRAVITY, slop=DC.SLOP, v_sleep=DC.V_SLEEP, w_sleep=DC.W_SLEEP, sleep_steps=DC.SLEEP_STEPS)
    # the field z on a grid that holds the whole drop: 24 x 24 x 16 points of 0.5
    grid = Grid(24, 24, 16, (-5.75, -5.75, -0.5), 0.5)
    z = torch.arange(16, dtype=torch.float32, device="cuda") * 0.5 - 0.5
    flat = ENV.EnvironmentField(z[:, None, None].expand(16, 24, 24).contiguous(), grid, friction=0.5)
    steps = {}
    for worlds in (1, 64, 1024):
        types = np.tile(np.array([0, 1, 2, 0, 1, 2], np.int32), (worlds, 1))
        poses = DYN.start_states(table, types, seed=0)
        row = dict(worlds=worlds, bodies=6, steps=a.steps)
        for what, ground in (("plane", None), ("field", flat)):
            r, (traj, rest, status) = timed(lambda: DYN.simulate(table, types, poses, a.steps, params, record_every=a.steps, ground=ground),
                                            a.warm, a.reps)
            rest = rest.cpu().numpy()
            r.update(us_per_step=1e3 * r["median_ms"] / a.steps, at_rest=int((rest >= 0).sum()), not_finite=int((status.cpu().numpy() != 0).sum()))
            row[what] = r
        row["field_over_plane"] = row["field"]["median_ms"] / row["plane"]["median_ms"]
        steps[str(worlds)] = row
        print(worlds, row)
    out = dict(device=torch.cuda.get_device_name(0), sdf_from_tsdf=fields, ground_per_step=steps,
               note="sdf_from_tsdf: events around the entry alone (4 launches); ground_per_step: the events bracket the host wrapper too, "
                    "as in rigid_bench.json")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1))
    print("wrote", a.out)


if __name__ == "__main__":
    main()

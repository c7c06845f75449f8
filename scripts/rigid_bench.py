"""Times of pgr_rigid_simulate on one GPU ("Measured"): 1, 64 and 1024 worlds of six bodies (two cubes, two
L-prisms, two small cubes of tests/dynamics_cases.py on 24^3 fields) for 1000 steps of 1 ms, from seeded start states.  Device
events around the library call, which enqueues all 2000 launches; medians after a warm-up, with the range.  A single world uses
one lane of the solver: its time is the launch-bound floor of a step.

    python scripts/rigid_bench.py [--out profiles/rigid_bench.json]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rigid_bench.json"))
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rigid_bench needs a HIP device: there is no CPU path and no time to report without one")
    import dynamics_cases as DC
    from pegasus_amd import collision as COL, dynamics as DYN
    from pegasus_amd.mesh import Mesh

    def body(name):
        m = Mesh(*DC.mesh(name))
        return DYN.RigidBody.from_collision(COL.CollisionBody(m, COL.MeshSDF.from_mesh(m, resolution=DC.RESOLUTION), shell=DC.shell(name)))
    table = [body(n) for n in ("cube", "l_prism", "small_cube")]
    params = DYN.Params(gravity=DC.GRAVITY, slop=DC.SLOP, v_sleep=DC.V_SLEEP, w_sleep=DC.W_SLEEP, sleep_steps=DC.SLEEP_STEPS)
    results = {}
    for worlds in (1, 64, 1024):
        types = np.tile(np.array([0, 1, 2, 0, 1, 2], np.int32), (worlds, 1))
        poses = DYN.start_states(table, types, seed=0)
        times, rest = [], None
        for k in range(a.warm + a.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            traj, rest, status = DYN.simulate(table, types, poses, a.steps, params, record_every=a.steps)
            stop.record()
            stop.synchronize()
            if k >= a.warm:
                times.append(start.elapsed_time(stop))
        rest, status = rest.cpu().numpy(), status.cpu().numpy()
        results[str(worlds)] = dict(worlds=worlds, bodies=6, steps=a.steps, median_ms=statistics.median(times), min_ms=min(times),
                                    max_ms=max(times), reps=a.reps, us_per_step=1e3 * statistics.median(times) / a.steps,
                                    world_steps_per_s=worlds * a.steps / (1e-3 * statistics.median(times)),
                                    at_rest=int((rest >= 0).sum()), median_rest_step=float(np.median(rest[rest >= 0])) if (rest >= 0).any() else None,
                                    not_finite=int((status != 0).sum()))
        print(worlds, results[str(worlds)])
    out = dict(device=torch.cuda.get_device_name(0), shells=[len(b.body.shell) for b in table], results=results,
               note="the events bracket the host wrapper too: state upload, workspace allocation and 2 launches per step")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1))
    print("wrote", a.out)


if __name__ == "__main__":
    main()

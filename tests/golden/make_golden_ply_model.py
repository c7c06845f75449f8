"""Generates tests/golden/bop_model.ply and bop_model.npz with the BOP toolkit's own writer:

    python tests/golden/make_golden_ply_model.py <checkout that holds submodules/bop_toolkit>

``inout.save_ply2`` writes an ASCII model with normals, uint8 colours and texture_u / texture_v (the layout of a downloaded
BOP ``models/obj_NNNNNN.ply``); the arrays handed to it go to the .npz.  Every coordinate is a multiple of 1/16, so the
writer's four decimals hold it exactly.  ``imageio`` and ``png``, which the module imports and the writer does not use, are
stubbed when missing.  Nothing at test time reads the toolkit; only the writer's output is stored."""
import sys
import types
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import mesh_raster_cases as MC          # noqa: E402


def main(checkout):
    sys.path.insert(0, str(checkout))
    sys.path.insert(0, str(Path(checkout) / "submodules" / "bop_toolkit"))
    for name in ("imageio", "png"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
    from submodules.bop_toolkit.bop_toolkit_lib import inout
    v, f = MC.icosphere(1, 1.0)
    rng = np.random.default_rng(20)
    pts = np.round(v.astype(np.float64) * 640.0) / 16.0                      # a 40 mm sphere on a 1/16 mm grid
    normals = np.round(v.astype(np.float64) * 16.0) / 16.0
    colors = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    uv = rng.integers(0, 17, (len(v), 2)) / 16.0
    inout.save_ply2(str(OUT / "bop_model.ply"), pts, pts_colors=colors, pts_normals=normals, faces=f, texture_uv=uv)
    np.savez(OUT / "bop_model.npz", pts=pts, normals=normals, colors=colors, faces=f.astype(np.int64), texture_uv=uv)
    print(f"{len(pts)} vertices, {len(f)} faces, {(OUT / 'bop_model.ply').stat().st_size} bytes")


if __name__ == "__main__":
    main(sys.argv[1])

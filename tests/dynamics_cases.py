"""Bodies, parameters and scenes of the dynamics tests: procedural, no fixture files.  The bodies are the unit-size meshes of
tests/collision_cases.py on 24^3 fields; the reference's objects are about a tenth of that, so gravity, slop and the linear sleep
threshold are ten times the defaults (the motion is then the same, in steps, as that of a 0.1 m object under g = 50).  Every
reference run (tests/dynamics_reference.py, float64) happens once per process and is shared, unchanged."""
import functools

import numpy as np

import collision_cases as CC
import collision_reference as CR
import dynamics_reference as DR

RESOLUTION = CC.DROP_RESOLUTION              # 24
SIZE = 10.0                                  # unit bodies over the reference's ~0.1 m objects
GRAVITY = (0.0, 0.0, -50.0 * SIZE)
SLOP = 2e-4 * SIZE
V_SLEEP, W_SLEEP, SLEEP_STEPS = 0.02 * SIZE, 0.4, 50
STEPS = 1500                                 # the step budget of every settling scene
MAX_WORD_EXEMPT = 0.02
MAX_ROW_EXEMPT = 0.05

MESHES = {"cube": CC.cube, "icosphere": CC.icosphere, "l_prism": CC.l_prism, "small_cube": lambda: CC.cube(0.6)}


@functools.lru_cache(maxsize=None)
def mesh(name):
    v, f = MESHES[name]()
    v.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def shell(name):
    """The body's shell points: the vertices of the icosphere (162); for the flat-faced bodies the vertices and a lattice of three
    subdivisions over every face (a flat face lying on a smaller one touches it between its corners)."""
    v, f = mesh(name)
    if name == "icosphere":
        return v
    k = 3
    tri = v.astype(np.float64)[f]
    pts = [v.astype(np.float64)]
    for i in range(k + 1):
        for j in range(k + 1 - i):
            pts.append((i * tri[:, 0] + j * tri[:, 1] + (k - i - j) * tri[:, 2]) / k)
    p = np.concatenate(pts)
    _, first = np.unique(np.round(p / 1e-6).astype(np.int64), axis=0, return_index=True)
    out = p[np.sort(first)].astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mass_properties(name, mass=1.0):
    """(com [3], inverse inertia [3,3]) of the uniform body, float64: ``Mesh.center_of_mass`` / ``Mesh.inertia``."""
    from pegasus_amd.mesh import Mesh
    m = Mesh(*mesh(name))
    return np.asarray(m.center_of_mass(), np.float64), np.linalg.inv(np.asarray(m.inertia(mass), np.float64))


@functools.lru_cache(maxsize=None)
def ref_body(name):
    return CR.RefBody(*mesh(name), RESOLUTION)


def ref_type(name, friction=0.5, field=None, grid=None):
    """The reference's type of a body: on the reference's own exact field, or on (field, grid) read back from the device."""
    com, iinv = mass_properties(name)
    if field is None:
        body = ref_body(name)
        field, grid = body.field, body.grid
    return DR.RefType(field, grid, shell(name), 1.0, com, iinv, friction)


def params(types, **kw):
    """DR.Params with the scaled values and the default margin: the largest voxel in play."""
    base = dict(gravity=GRAVITY, slop=SLOP, v_sleep=V_SLEEP, w_sleep=W_SLEEP, sleep_steps=SLEEP_STEPS,
                margin=max(t.grid.voxel for t in types))
    base.update(kw)
    return DR.Params(**base)


def package_params(p: DR.Params):
    """The package's Params with the same numbers."""
    from pegasus_amd.dynamics import Params
    return Params(h=p.h, gravity=tuple(p.gravity), plane=tuple(p.plane), plane_friction=p.plane_friction, lin_damp=p.lin_damp,
                  ang_damp=p.ang_damp, iterations=p.iterations, beta=p.beta, slop=p.slop, margin=p.margin, v_sleep=p.v_sleep,
                  w_sleep=p.w_sleep, sleep_steps=p.sleep_steps)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
SCENES = {"sphere": ("icosphere",), "cube_tilted": ("cube",), "column": ("cube", "l_prism", "small_cube")}
WORLDS = 8


def reference_quaternion(rng):
    q = rng.uniform(0.0, 1.0, 4)
    return q / np.linalg.norm(q)


def small_tilt(rng, angle=0.05):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-angle, angle)
    return np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])


def start_poses(name, world):
    """Mesh-frame start poses [B,7] of one world, from the generator seeded with (scene, world)."""
    rng = np.random.default_rng([sorted(SCENES).index(name), world])
    if name == "sphere":
        return np.array([np.concatenate([[0.02 * world, -0.01 * world, 0.7 + 0.03 * world], reference_quaternion(rng)])])
    if name == "cube_tilted":
        return np.array([np.concatenate([[0.0, 0.0, 1.1 + 0.02 * world], reference_quaternion(rng)])])
    off = rng.uniform(-0.04, 0.04, (3, 2))
    z = (0.65, 1.55, 2.25)
    return np.array([np.concatenate([[off[k, 0], off[k, 1], z[k]], small_tilt(rng)]) for k in range(3)])


def state_of(types, poses):
    """[B,13] float64 holding float32 numbers: the state of mesh-frame poses at rest (x = t + R com)."""
    out = np.zeros((len(types), 13))
    for k, (t, pose) in enumerate(zip(types, poses)):
        q = pose[3:] / np.linalg.norm(pose[3:])
        out[k, :3] = pose[:3] + DR.rotation(q) @ t.com
        out[k, 3:7] = q
    return DR.f32(out)


# With the default margin -- one voxel of a 24^3 field, a twentieth of the body -- the finely faceted sphere never rests: the
# seven words keep ONE deepest point and six points from the rim of the candidate cap, which are far above the plane, so the
# sphere rocks from facet corner to facet corner for ever ("limits").  A margin below the facets' sagitta
# makes the corners of the facet it lies on the candidates.  The boxes settle with the default.
SCENE_MARGIN_FRACTION = {"sphere": 0.125}


def scene_params(name, types, **kw):
    p = params(types, **kw)
    p.margin = float(np.float32(p.margin * SCENE_MARGIN_FRACTION.get(name, 1.0)))
    return p


@functools.lru_cache(maxsize=None)
def reference_run(name, world=0):
    """The reference's run of one world of a scene on its own fields: DR.simulate's result with every step's start state."""
    types = [ref_type(n) for n in SCENES[name]]
    return DR.simulate(types, list(range(len(types))), state_of(types, start_poses(name, world)), STEPS,
                       scene_params(name, types), snapshots=range(STEPS))


def steady_depth(run, p):
    """d: the reference run's own deepest penetration beyond slop over its last 50 moving steps (0 where it has no contact)."""
    last = run["rest_step"] if run["rest_step"] >= 0 else len(run["deepest"]) - 1
    deep = run["deepest"][max(0, last - 50):last + 1]
    deep = deep[np.isfinite(deep)]
    return max(0.0, float(-deep.min()) - p.slop) if len(deep) else 0.0


# A box lying flat on a box has the same field value all over the face: exact ties, which the exemption rule gives away.  These
# two worlds of the column scene hold few of them (6 of 504 words on the reference's fields; the cap is 10).
CONTACT_WORLDS = (1, 2)


@functools.lru_cache(maxsize=None)
def contact_states():
    """(type names, states [8,3,13] float64 of float32 numbers): the column scene's reference runs of two worlds at four moments
    each -- mid-air (step 0), first touch (the first step with a contact row), tumbling (halfway to rest) and at rest, stacked or
    fallen (the final state)."""
    states = []
    for world in CONTACT_WORLDS:
        run = reference_run("column", world)
        touched = np.flatnonzero(run["contacts"] > 0)
        first = int(touched[0]) if len(touched) else 0
        last = run["rest_step"] if run["rest_step"] >= 0 else STEPS - 1
        for k in (0, first, (first + last) // 2):
            states.append(run["snapshots"][k])
        states.append(run["state"])
    out = DR.f32(np.stack(states))
    out.setflags(write=False)
    return SCENES["column"], out


def word_exemptions(types, type_row, state, p):
    """(reference words [B*B][7], exempt [B*B][7] bool) of one world.  A word is exempt where another candidate's key is within
    twice the point bound of the winner's, where the pair's sphere test lies within 12 u P of its threshold, or where a point's
    phi <= margin test lies within its bound of the threshold."""
    words, info = DR.world_words(types, type_row, state, p, detail=True)
    B = len(type_row)
    exempt = np.zeros((B * B, DR.WORDS), bool)
    reach = max(1.0, float(np.abs(state[:, :3]).max()) + max(t.radius for t in types))
    for k, d in info.items():
        if d["sphere_gap"] <= 12.0 * DR.U * reach:
            exempt[k] = True
            continue
        if d["values"] is None:
            continue
        if (d["threshold_gap"] <= d["bound"]).any():
            exempt[k] = True
            continue
        cand = np.flatnonzero(d["candidate"])
        for j in range(DR.WORDS):
            if len(cand) < 2:
                break
            v = d["values"][cand, j]
            win = cand[np.lexsort((cand, v))[0]]
            others = cand[cand != win]
            gap = np.abs(d["values"][others, j] - d["values"][win, j])
            exempt[k, j] = bool((gap <= 2.0 * np.maximum(d["bound"][others], d["bound"][win])).any())
    return words, exempt


# ---- friction -------------------------------------------------------------------------------------------------------------------
TILT = np.deg2rad(20.0)
FRICTION_STEPS = 500
FRICTION_CASES = {"sticks": 1.0, "slides": 0.2}        # the cube's friction; the plane's is 0.5: mu = 0.5 and 0.1 (tan 20 deg = 0.364)


def friction_params(types):
    g = 50.0 * SIZE
    return params(types, gravity=(g * np.sin(TILT), 0.0, -g * np.cos(TILT)))


def friction_start():
    return np.array([[0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def friction_reference(case):
    types = [ref_type("cube", FRICTION_CASES[case])]
    return DR.simulate(types, [0], state_of(types, friction_start()), FRICTION_STEPS, friction_params(types))

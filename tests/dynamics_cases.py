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


# ---- edges: shells beyond one point block, a tie across blocks, a crowded world, the guard's triggers ---------------------------
POINT_BLOCK = 256                            # rigid_contacts_kernel's points per workgroup
SHELL_CASES = ((257, 513, 256), (300, 700, 64))        # shell sizes of (cube, L prism, small cube): see scattered_shell
MIN_HIGH_INDEX_WORDS = 20


@functools.lru_cache(maxsize=None)
def scattered_shell(name, n, seed):
    """float32 [n,3]: the mesh's vertices and n - len(vertices) random points on its faces -- area-weighted over the triangles,
    uniform in each -- shuffled as a whole, all from the generator seeded with ``seed`` (an int or a tuple of ints).  Random
    points tie far less often on a flat face than a lattice does, and any block of 256 holds points of every face."""
    v, f = mesh(name)
    rng = np.random.default_rng(list(seed) if isinstance(seed, tuple) else seed)
    tri = v.astype(np.float64)[f]
    m = n - len(v)
    if m < 0:
        raise ValueError("fewer points than vertices")
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    t = tri[rng.choice(len(tri), size=m, p=area / area.sum())]
    a, b = rng.uniform(size=m), rng.uniform(size=m)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    p = np.concatenate([v.astype(np.float64), t[:, 0] + a[:, None] * (t[:, 1] - t[:, 0]) + b[:, None] * (t[:, 2] - t[:, 0])])
    out = p[rng.permutation(n)].astype(np.float32)
    out.setflags(write=False)
    return out


def case_shells(case):
    """The scattered shells of the column's three bodies for one of SHELL_CASES: body k's from the generator seeded [k, n]."""
    return [scattered_shell(name, n, (k, n)) for k, (name, n) in enumerate(zip(SCENES["column"], case))]


def with_shell(t, points):
    """The reference's type ``t`` with another shell (the radius follows the shell, as RigidBody.from_collision's does)."""
    return DR.RefType(t.field, t.grid, points, t.mass, t.com, t.iinv, t.friction)


TIE_POINTS = 600


@functools.lru_cache(maxsize=None)
def tie_shell():
    """float32 [600,3]: a scattered shell of the cube without the side points a margin above the bottom face (the flat cube's
    candidates are then its bottom points alone, all with the same phi and r.z), ordered so that no bottom point (z = -0.5) has
    an index below 256, the lowest bottom index lies in point block 1 and further bottom points lie in block 2."""
    p = scattered_shell("cube", 800, 5)
    p = p[~((p[:, 2] > -0.5) & (p[:, 2] < -0.3))][:TIE_POINTS]
    bottom, other = np.flatnonzero(p[:, 2] == -0.5), np.flatnonzero(p[:, 2] != -0.5)
    half = len(bottom) // 2
    out = p[np.concatenate([other[:300], bottom[:half], other[300:], bottom[half:]])].copy()
    out.setflags(write=False)
    return out


def flat_cube_state(types):
    """[1,13]: the cube flat on the plane, as test_contact_ties_empty_slots_and_a_single_body puts it."""
    return state_of(types[:1], np.array([[0.0, 0.0, 0.5, 0, 0, 0, 1.0]]))


CROWD_SPACING, CROWD_CENTER = 0.58, (0.0, 0.0, 1.2)


def crowd(types):
    """[8,13] float64 of float32 numbers: eight small cubes (side 0.6, ``types`` = [the small cube's type]) at the corners of a
    2x2x2 lattice of spacing 0.58, so every neighbour overlaps by 0.02 and all 56 ordered pairs are in sphere range; each slightly
    tilted and moving.  The bottom cubes' spheres end 0.39 above the plane: no plane contact."""
    rng = np.random.default_rng(8)
    half = 0.5 * CROWD_SPACING
    corners = np.array([[x, y, z] for z in (-half, half) for y in (-half, half) for x in (-half, half)]) + np.asarray(CROWD_CENTER)
    poses = np.array([np.concatenate([c, small_tilt(rng, 0.03)]) for c in corners])
    state = state_of([types[0]] * 8, poses)
    state[:, 7:10] = DR.f32(rng.uniform(-0.5, 0.5, (8, 3)))
    state[:, 10:13] = DR.f32(rng.uniform(-1.0, 1.0, (8, 3)))
    return state


EMBEDDED_ROW = (-1, 0, -1, -1, 1, -1, -1, 2)            # the column in slots 1, 4 and 7 of eight
FULL_ROW = (2, 0, 1, 0, 1, 2, 0, 2)                     # .. and five flyers in the other slots
COLUMN_SLOTS, FLYER_SLOTS = (1, 4, 7), (0, 2, 3, 5, 6)


def flyers(types, type_row=FULL_ROW, slots=FLYER_SLOTS):
    """{slot: [13]}: bodies at rest, tens of units up and apart: 40 + 15 k above the plane and 15 k along x.  In 60 steps of free
    fall (|g| = 500, h = 1e-3) a body drops 0.92, so each stays out of sphere range of the plane and of everything else."""
    out = {}
    for k, a in enumerate(slots):
        out[a] = state_of([types[type_row[a]]], np.array([[15.0 * (k + 1), -20.0, 40.0 + 15.0 * k, 0, 0, 0, 1.0]]))[0]
    return out


# The guard's triggers.  A: a zero quaternion, whose normalisation divides 0 by 0 in the first step.  B: a lone body so far up and
# so fast that x.z = 3.394e38 + k h v passes float32's largest number 3.402823e38 in the third step (index 2) and in no earlier
# one: 3.397e38, 3.400e38 (2.8e35 below it), 3.403e38 (1.8e34 above it); |x_a - x_b|^2 overflows to +inf, which is out of sphere
# range, so nothing is NaN before the guard.
GUARD_STEP = {"A": 0, "B": 2}
FAR_Z, FAR_VZ = 3.394e38, 3e38


def far_body():
    """[13]: trigger B's body, at rest in everything but z."""
    s = np.zeros(13)
    s[2], s[6], s[9] = FAR_Z, 1.0, FAR_VZ
    return DR.f32(s)


def guard_state(column_state, trigger):
    """[4,13]: a world of the column's three bodies (``column_state`` [3,13]) and a fourth slot: empty for no trigger (None), with
    a zero quaternion in body 1 for trigger A, with the far body in slot 3 for trigger B."""
    s = np.zeros((4, 13))
    s[3, 6] = 1.0
    s[:3] = column_state
    if trigger == "A":
        s[1, 3:7] = 0.0
    elif trigger == "B":
        s[3] = far_body()
    return s


def guard_types(trigger):
    return [0, 1, 2, 0 if trigger == "B" else -1]


# ---- friction -------------------------------------------------------------------------------------------------------------------
TILT =np.deg2rad(20.0)
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

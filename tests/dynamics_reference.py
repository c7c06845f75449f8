"""NumPy float64 transcription of the rigid-body rule (pegasus_amd/csrc/rigid.hip.h): what the kernels
are held against.  It shares no code with the package; the field is sampled with collision_reference.sample.  Every input is
the float32 number the device gets, held as float64; everything after that is float64.

Counted bounds (u = 2^-24, P the largest coordinate in play):
  a shell point in the world, or in a target's frame: the affine maps of collision_reference's sweep bound, 36 u P on a field
    value, plus the sample bound, plus 2 u P for the float32 point collision_reference.sample takes; a component of
    r = p - x_a stays within 12 u P.  pair_points() returns the sum per point: what the tests call the bound of a contact key.
  integration x + h v: 2 u (|x| + h |v|) per step; the free-flight recursion v_k = (v_{k-1} + h g) f: 3 u |v| per step.
"""
import numpy as np

import collision_reference as CR

U = CR.U
WORDS = 7
EMPTY = 2 ** 64 - 1
PLANE = -1


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


class RefType:
    """One body type: field [nz,ny,nx] on a RefGrid, shell [n,3] (mesh frame), mass, com, inverse inertia, friction, radius."""

    def __init__(self, field, grid, shell, mass, com, inv_inertia, friction, radius=None):
        self.field = None if field is None else np.asarray(field, np.float64)
        self.grid = grid
        self.shell = f32(shell).reshape(-1, 3)
        self.mass = float(np.float32(mass))
        self.com = f32(com).reshape(3)
        self.iinv = f32(inv_inertia).reshape(3, 3)
        self.friction = float(np.float32(friction))
        r = np.linalg.norm(self.shell - self.com, axis=1).max() if radius is None and len(self.shell) else (radius or 0.0)
        self.radius = float(np.float32(r))


class Params:
    def __init__(self, h=1e-3, gravity=(0.0, 0.0, -50.0), plane=(0.0, 0.0, 1.0, 0.0), plane_friction=0.5, lin_damp=0.04,
                 ang_damp=0.04, iterations=10, beta=0.2, slop=2e-4, margin=0.0, v_sleep=0.02, w_sleep=0.4, sleep_steps=50):
        self.h = float(np.float32(h))
        self.gravity = f32(gravity)
        self.plane = f32(plane)
        self.plane_friction = float(np.float32(plane_friction))
        self.lin_damp, self.ang_damp = float(np.float32(lin_damp)), float(np.float32(ang_damp))
        self.iterations = int(iterations)
        self.beta, self.slop, self.margin = (float(np.float32(x)) for x in (beta, slop, margin))
        self.v_sleep, self.w_sleep = float(np.float32(v_sleep)), float(np.float32(w_sleep))
        self.sleep_steps = int(sleep_steps)

    @property
    def lin_factor(self):
        return float(np.float32((1.0 - self.lin_damp) ** self.h))

    @property
    def ang_factor(self):
        return float(np.float32((1.0 - self.ang_damp) ** self.h))


def rotation(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def frame(state_row, com):
    """(R, T = x - R c) of a body's state [13]."""
    R = rotation(state_row[3:7])
    return R, state_row[0:3] - R @ com


def mesh_pose(state_row, com):
    """[7]: the mesh-frame pose (T, q) a record holds."""
    return np.concatenate([frame(state_row, com)[1], state_row[3:7]])


def valid_type(t, n_types):
    return int(t) if 0 <= int(t) < n_types else -1


# ---- contacts -------------------------------------------------------------------------------------------------------------------
def pair_points(types, type_row, state, a, b, params, idx=None):
    """The shell points of mover a (all, or those of ``idx``) against b (PLANE: the plane): p [n,3], phi [n], normal [n,3],
    ok [n] (the gradient gives a normal), bound [n] (point_bound)."""
    A = types[type_row[a]]
    Ra, Ta = frame(state[a], A.com)
    s = A.shell if idx is None else A.shell[np.asarray(idx, np.int64)]
    p = s @ Ra.T + Ta
    reach = max(1.0, float(np.abs(p).max()) if len(p) else 1.0, float(np.abs(state[:, :3]).max()))
    if b == PLANE:
        n, d = params.plane[:3], params.plane[3]
        return p, p @ n - d, np.tile(n, (len(p), 1)), np.ones(len(p), bool), np.full(len(p), 36.0 * U * reach)
    Bt = types[type_row[b]]
    Rb, Tb = frame(state[b], Bt.com)
    y = (p - Tb) @ Rb
    phi, grad, info = CR.sample(Bt.field, Bt.grid, y, True)          # (it takes its points as float32: 1 u P more)
    gn = np.linalg.norm(grad, axis=1)
    ok = gn >= 1e-6
    normal = (grad / np.where(ok, gn, 1.0)[:, None]) @ Rb.T
    return p, phi, normal, ok, CR.sweep_step_bound(reach, CR.sample_bound(Bt.grid, info)) + 2.0 * U * reach


def words_of(phi, r, candidate):
    """The seven words of a pair from per-point phi [n], r = p - x_a [n,3] and the candidate mask: packed minima, EMPTY without
    a candidate."""
    idx = np.flatnonzero(candidate)
    if len(idx) == 0:
        return [EMPTY] * WORDS
    values = key_values(phi, r)
    return [min(CR.word(values[i, k], i) for i in idx) for k in range(WORDS)]


def key_values(phi, r):
    """[n,7]: phi, +x, -x, +y, -y, +z, -z of r."""
    return np.stack([phi, r[:, 0], -r[:, 0], r[:, 1], -r[:, 1], r[:, 2], -r[:, 2]], axis=1)


def contacts_of(words):
    """The distinct point indices of a pair's words, ascending (at most 7); none for an empty pair."""
    if int(words[0]) == EMPTY:
        return []
    return sorted({int(w) & 0xFFFFFFFF for w in words})


def pair_order(B):
    """(a, b) in list order: per mover the plane, then every b != a ascending.  slot(a, b) = a B + (a for the plane, else b)."""
    for a in range(B):
        yield a, PLANE
        for b in range(B):
            if b != a:
                yield a, b


def slot(a, b, B):
    return a * B + (a if b == PLANE else b)


def in_range(types, type_row, state, a, b, params):
    """(the sphere test lets the pair through, how far the test is from its threshold)."""
    A = types[type_row[a]]
    if b == PLANE:
        gap = (state[a, :3] @ params.plane[:3] - params.plane[3]) - A.radius
    else:
        gap = np.linalg.norm(state[a, :3] - state[b, :3]) - (A.radius + types[type_row[b]].radius)
    return not gap > params.margin, abs(gap - params.margin)


def world_words(types, type_row, state, params, detail=False):
    """uint64-valued ints [B*B][7] of one world; with ``detail`` also {slot: dict(values [n,7], candidate [n], bound [n],
    sphere_gap, threshold_gap)} for the pairs in sphere range."""
    B = len(type_row)
    type_row = [valid_type(t, len(types)) for t in type_row]
    out = [[EMPTY] * WORDS for _ in range(B * B)]
    info = {}
    for a, b in pair_order(B):
        if type_row[a] < 0 or (b != PLANE and type_row[b] < 0):
            continue
        near, sphere_gap = in_range(types, type_row, state, a, b, params)
        k = slot(a, b, B)
        if not near:
            info[k] = dict(sphere_gap=sphere_gap, values=None)
            continue
        if len(types[type_row[a]].shell) == 0:
            continue
        p, phi, _, ok, bound = pair_points(types, type_row, state, a, b, params)
        cand = ok & (phi <= params.margin)
        r = p - state[a, :3]
        out[k] = words_of(phi, r, cand)
        info[k] = dict(sphere_gap=sphere_gap, values=key_values(phi, r), candidate=cand, bound=bound,
                       threshold_gap=np.abs(phi - params.margin))
    return (out, info) if detail else out


def contact_list(words, B):
    """[(a, b, point index)] of one world's words in list order."""
    return [(a, b, i) for a, b in pair_order(B) for i in contacts_of(words[slot(a, b, B)])]


# ---- one step -------------------------------------------------------------------------------------------------------------------
def build_rows(types, type_row, state, contacts, params):
    rows = []
    for a, b, i in contacts:
        A = types[type_row[a]]
        p, phi, normal, ok, _ = pair_points(types, type_row, state, a, b, params, [i])
        if not ok[0]:
            continue
        p, phi, n = p[0], float(phi[0]), normal[0]
        Ra = rotation(state[a, 3:7])
        Wa = Ra @ A.iinv @ Ra.T
        ra = p - state[a, :3]
        e = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
        t1 = np.cross(n, e)
        t1 /= np.linalg.norm(t1)
        dirs = [n, t1, np.cross(n, t1)]
        ima, imb, mu = 1.0 / A.mass, 0.0, A.friction * params.plane_friction
        if b != PLANE:
            Bt = types[type_row[b]]
            Rb = rotation(state[b, 3:7])
            Wb = Rb @ Bt.iinv @ Rb.T
            rb = p - state[b, :3]
            imb, mu = 1.0 / Bt.mass, A.friction * Bt.friction
        row = dict(a=a, b=b, point=i, phi=phi, ima=ima, imb=imb, mu=mu, lam=[0.0, 0.0, 0.0], dirs=[], near_clamp=False,
                   bias=phi / params.h if phi > 0 else -params.beta * max(-phi - params.slop, 0.0) / params.h)
        for d in dirs:
            ca = np.cross(ra, d)
            wa = Wa @ ca
            k = ima + ca @ wa
            cb = wb = np.zeros(3)
            if b != PLANE:
                cb = np.cross(rb, d)
                wb = Wb @ cb
                k += imb + cb @ wb
            row["dirs"].append((d, ca, wa, cb, wb, 1.0 / k))
        rows.append(row)
    return rows


def solve(rows, V, params, clamp_rel=1e-4, scale=0.0):
    """Sequential impulses on V [B,6] (v, omega) in place.  Marks rows that come near a clamp in any sweep: a pre-clamp normal
    impulse within ``clamp_rel`` x ``scale`` of 0 (``scale``: a body's weight times h, the impulse that holds it), a friction
    impulse within ``clamp_rel`` x its limit of that limit."""
    for _ in range(params.iterations):
        for row in rows:
            a, b = row["a"], row["b"]
            for k, (d, ca, wa, cb, wb, meff) in enumerate(row["dirs"]):
                vrel = d @ V[a, :3] + ca @ V[a, 3:]
                if b != PLANE:
                    vrel -= d @ V[b, :3] + cb @ V[b, 3:]
                l0 = row["lam"][k]
                if k == 0:
                    pre = l0 - (vrel + row["bias"]) * meff
                    l1 = max(pre, 0.0)
                    if abs(pre) <= clamp_rel * scale:
                        row["near_clamp"] = True
                else:
                    lim = row["mu"] * row["lam"][0]
                    pre = l0 - vrel * meff
                    l1 = min(max(pre, -lim), lim)
                    if lim > 0.0 and abs(abs(pre) - lim) <= clamp_rel * lim:     # (lim = 0 gives 0 whatever pre is)
                        row["near_clamp"] = True
                dl = l1 - l0
                row["lam"][k] = l1
                V[a, :3] += dl * row["ima"] * d
                V[a, 3:] += dl * wa
                if b != PLANE:
                    V[b, :3] -= dl * row["imb"] * d
                    V[b, 3:] -= dl * wb


def integrate(state, params):
    h = params.h
    for s in state:
        s[0:3] += h * s[7:10]
        u, w, om = s[3:6].copy(), s[6], s[10:13]
        s[3:6] = u + 0.5 * h * (w * om + np.cross(om, u))
        s[6] = w - 0.5 * h * (om @ u)
        s[3:7] /= np.linalg.norm(s[3:7])


def step(types, type_row, state, params, contacts=None):
    """One step of one world from ``state`` [B,13] (not modified): (new state, rows, calm).  ``contacts``: the list to use
    (the device's), else the reference's own."""
    B = len(type_row)
    type_row = [valid_type(t, len(types)) for t in type_row]
    present = [a for a in range(B) if type_row[a] >= 0]
    if contacts is None:
        contacts = contact_list(world_words(types, type_row, state, params), B)
    new = np.array(state, np.float64)
    for a in present:
        new[a, 7:10] = (new[a, 7:10] + params.h * params.gravity) * params.lin_factor
        new[a, 10:13] = new[a, 10:13] * params.ang_factor
    rows = build_rows(types, type_row, state, contacts, params)
    V = new[:, 7:13].copy()
    scale = params.h * float(np.linalg.norm(params.gravity)) * max([types[type_row[a]].mass for a in present], default=0.0)
    solve(rows, V, params, scale=scale)
    new[:, 7:13] = V
    integrate([new[a] for a in present], params)
    calm = all(np.linalg.norm(new[a, 7:10]) < params.v_sleep and np.linalg.norm(new[a, 10:13]) < params.w_sleep for a in present)
    return new, rows, calm


def simulate(types, type_row, state0, n_steps, params, record_every=1, snapshots=()):
    """One world: dict(trajectory [n_records,B,7], rest_step, status, state: the final one, snapshots {step: state BEFORE that
    step}, deepest: the smallest phi of any contact row per step (nan without), contacts: the row count per step)."""
    B = len(type_row)
    types_of = [valid_type(t, len(types)) for t in type_row]
    state = np.array(state0, np.float64).reshape(B, 13)
    n_records = n_steps // record_every
    traj = np.zeros((n_records, B, 7))
    traj[:, :, 6] = 1.0
    rest_step, status, count, halted = -1, 0, 0, False
    deepest, n_rows, snaps = np.full(n_steps, np.nan), np.zeros(n_steps, np.int64), {}
    for k in range(n_steps):
        if k in snapshots:
            snaps[k] = state.copy()
        if not halted:
            new, rows, calm = step(types, types_of, state, params)
            n_rows[k] = len(rows)
            if rows:
                deepest[k] = min(r["phi"] for r in rows)
            with np.errstate(over="ignore"):
                finite = np.isfinite(new.astype(np.float32)).all()                # rule 7 judges the float32 state the device holds
            if not finite:
                status, halted = 1, True
            else:
                state = new
                count = count + 1 if calm else 0
                if params.sleep_steps > 0 and count >= params.sleep_steps:
                    for a in range(B):
                        if types_of[a] >= 0:
                            state[a, 7:13] = 0.0
                    rest_step, halted = k, True
        if (k + 1) % record_every == 0:
            for a in range(B):
                if types_of[a] >= 0:
                    traj[(k + 1) // record_every - 1, a] = mesh_pose(state[a], types[types_of[a]].com)
    return dict(trajectory=traj, rest_step=rest_step, status=status, state=state, snapshots=snaps, deepest=deepest, contacts=n_rows)


def free_flight(z0, v0, g, h, factor, k):
    """(z_k, v_k) of the closed recursion v_j = (v_{j-1} + h g) f, z_j = z_{j-1} + h v_j, in float64."""
    z, v = float(z0), float(v0)
    for _ in range(k):
        v = (v + h * g) * factor
        z = z + h * v
    return z, v

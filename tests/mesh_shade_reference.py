"""Two CPU versions of pgr_mesh_visibility + pgr_mesh_shade, written from the rules at the top of
pegasus_amd/csrc/meshraster.hip.h (the key rule) and above its mesh_shade_kernel (the resolve rule), on top of the
projection, snap, face setup and coverage walk of tests/mesh_raster_reference.py.

``visibility_f32`` / ``shade_f32``   the float32 transcription: the same operations in the same order; the kernels' outputs
                 equal it bit for bit.
``shade_f64``    a float64 oracle of the same rule, with a mask and derived bounds (its docstring).

A job is the dict of mesh_raster_reference plus, optionally, ``normals`` [V,3] and ``colors`` [V,3] (float32, per vertex) and
``surf_color`` [3].  Options: ``smooth`` (use the normals; else flat), ``use_colors`` (else surf_color, default 0.5 grey),
``light`` [3], ``ambient``, ``bg`` [3].

The rule (restated).  key = float_bits(z) << 32 | job << 22 | face, minimum per pixel, empty = 0.  For the winning face, with
a, b, c after the swap that makes area2 > 0 and the int64 edge values at the sample:
    la = f(E_bc) w_a, lb = f(E_ca) w_b, lc = f(E_ab) w_c, den = (la + lb) + lc, A = ((la A_a + lb A_b) + lc A_c) / den
    xyz = A(model vertices);  P = ((R0 x + R1 y) + R2 z) + t;  d = light - P;  L = d / sqrt((dx dx + dy dy) + dz dz)
    flat:   m = cross(P_b - P_a, P_c - P_a), n = m / sqrt((mx mx + my my) + mz mz), negated when (nx Px + ny Py) + nz Pz > 0
    smooth: a = A(model normals), m = (R0 ax + R1 ay) + R2 az, n = m / |m| alike, no flip
    |m| zero or not finite: n = 0, diffuse = 0;  else diffuse = fmax((Lx nx + Ly ny) + Lz nz, 0)
    light_w = fmin(ambient + diffuse, 1);  rgb = light_w * colour;  colour = A(colors) or the job's surf_color;  empty: bg
"""
import numpy as np

import mesh_raster_reference as MR

FACE_BITS = 22
FACE_MASK = (1 << FACE_BITS) - 1
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
EPS32 = MR.EPS32
MUTANTS = ("no_attribute_swap", "higher_index_wins", "screen_space_weights", "flat_normal_not_flipped", "light_w_not_clamped",
           "L_not_normalised")
DEFAULTS = dict(smooth=False, use_colors=False, light=(0.0, 0.0, 0.0), ambient=0.5, bg=(0.0, 0.0, 0.0))


def _n_slots(jobs, n_slots):
    return (max(j["slot"] for j in jobs) + 1 if jobs else 1) if n_slots is None else n_slots


def _setup(job, dtype, near, W, H):
    X, Y, Z, u, v = MR._project(job, dtype)
    sx, sy = MR._snap(u), MR._snap(v)
    status, x, y, vid, area2, box = MR._faces_setup(job, sx, sy, Z, dtype(near), W, H)
    with np.errstate(all="ignore"):
        inv = dtype(1) / Z
    return dict(cam=np.stack([X, Y, Z], 1) if len(X) else np.zeros((0, 3), dtype), inv=inv, status=status, x=x, y=y, vid=vid,
                area2=area2, box=box, sx=sx, sy=sy)


def _samples(jobs, W, H, near, dtype):
    """Every covered sample that counts, of all jobs: (slot, pixel, z in ``dtype``, id = job << 22 | face), and the number of
    faces dropped for straddling ``near``."""
    slot, pix, zs, ids, straddle = [], [], [], [], 0
    for k, job in enumerate(jobs):
        s = _setup(job, dtype, near, W, H)
        straddle += int((s["status"] == 2).sum())
        keep = np.nonzero(s["status"] == 1)[0]
        if not len(keep):
            continue
        x, y, area2 = s["x"][keep], s["y"][keep], s["area2"][keep]
        w = s["inv"][s["vid"][keep]]
        for f, i, j, ea, eb, ec in MR._covered_samples(x, y, tuple(b[keep] for b in s["box"])):
            with np.errstate(all="ignore"):
                den = (ea.astype(dtype) * w[f, 0] + eb.astype(dtype) * w[f, 1]) + ec.astype(dtype) * w[f, 2]
                z = area2[f].astype(dtype) / den
            good = (den > 0) & (z > 0) & (z < np.inf)
            slot.append(np.full(int(good.sum()), job["slot"], np.int64)); pix.append((j * W + i)[good])
            zs.append(z[good]); ids.append((k << FACE_BITS) | keep[f][good])
    cat = lambda l, dt: np.concatenate(l).astype(dt) if l else np.zeros(0, dt)
    return cat(slot, np.int64), cat(pix, np.int64), cat(zs, dtype), cat(ids, np.int64), straddle


def visibility_f32(jobs, width, height, near, n_slots=None, mutant=None):
    """(keys uint64 [n_slots,H,W], faces dropped for straddling ``near``): the transcription of pgr_mesh_visibility."""
    n_slots = _n_slots(jobs, n_slots)
    keys = np.full((n_slots, height * width), ALL_ONES, np.uint64)
    slot, pix, z, ids, straddle = _samples(jobs, width, height, near, np.float32)
    low = (0xFFFFFFFF - ids) if mutant == "higher_index_wins" else ids
    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)
    np.minimum.at(keys, (slot, pix), key)
    keys[keys == ALL_ONES] = 0
    if mutant == "higher_index_wins":
        hit = keys != 0
        keys[hit] = (keys[hit] & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - (keys[hit] & np.uint64(0xFFFFFFFF)))
    return keys.reshape(n_slots, height, width), straddle


def _attr(la, lb, lc, den, A, vid):
    """The attribute rule for per-vertex rows A [V,C] at the corners vid [N,3]: [N,C]."""
    a, b, c = A[vid[:, 0]], A[vid[:, 1]], A[vid[:, 2]]
    with np.errstate(all="ignore"):
        return ((la[:, None] * a + lb[:, None] * b) + lc[:, None] * c) / den[:, None]


def _rot(R, a, t=None):
    with np.errstate(all="ignore"):
        out = [(R[3 * d] * a[:, 0] + R[3 * d + 1] * a[:, 1]) + R[3 * d + 2] * a[:, 2] for d in range(3)]
        if t is not None:
            out = [o + t[d] for d, o in enumerate(out)]
    return np.stack(out, 1)


def _dot(a, b):
    with np.errstate(all="ignore"):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _resolve(job_id, face_id, jobs, width, height, near, dtype, opts, mutant=None):
    """The resolve rule in ``dtype`` for the winners job_id, face_id int [n_slots,H,W] (-1: empty).  Returns the outputs
    (without depth ids) plus ``z`` (the depth rule's value) and, for the oracle's bounds, ``mlen``, ``dlen``, ``flip_dot``,
    ``U`` (the longest flat-normal edge component)."""
    o = dict(DEFAULTS, **opts)
    n_slots = job_id.shape[0]
    shape = (n_slots, height, width)
    out = dict(xyz=np.zeros(shape + (3,), dtype), normal=np.zeros(shape + (3,), dtype),
               rgb=np.broadcast_to(np.asarray(o["bg"], np.float32).astype(dtype), shape + (3,)).copy(),
               z=np.zeros(shape, dtype), mlen=np.full(shape, np.nan), dlen=np.full(shape, np.nan),
               flip_dot=np.full(shape, np.nan), U=np.zeros(shape))
    light = np.asarray(o["light"], np.float32).astype(dtype)
    ambient = np.float32(o["ambient"]).astype(dtype)
    for k, job in enumerate(jobs):
        s_, jj, ii = np.nonzero(job_id == k)
        if not len(s_):
            continue
        f = face_id[s_, jj, ii]
        s = _setup(job, dtype, near, width, height)
        x, y, vid = s["x"][f], s["y"][f], s["vid"][f]
        w = s["inv"][vid]
        X, Y = ii.astype(np.int64) << 8, jj.astype(np.int64) << 8
        ea = MR._edge(x[:, 1], y[:, 1], x[:, 2], y[:, 2], X, Y)
        eb = MR._edge(x[:, 2], y[:, 2], x[:, 0], y[:, 0], X, Y)
        ec = MR._edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], X, Y)
        la, lb, lc = ea.astype(dtype) * w[:, 0], eb.astype(dtype) * w[:, 1], ec.astype(dtype) * w[:, 2]
        if mutant == "screen_space_weights":
            la, lb, lc = ea.astype(dtype), eb.astype(dtype), ec.astype(dtype)
        den = (la + lb) + lc
        with np.errstate(all="ignore"):
            out["z"][s_, jj, ii] = s["area2"][f].astype(dtype) / den
        avid = vid
        if mutant == "no_attribute_swap":                # the corners in the file's order, the weights in the swapped one
            avid = np.asarray(job["faces"], np.int64).reshape(-1, 3)[f]
        V = np.asarray(job["vertices"], np.float32).reshape(-1, 3).astype(dtype)
        R = MR._f32(job["R"]).reshape(9).astype(dtype)
        t = MR._f32(job["t"]).reshape(3).astype(dtype)
        xyz = _attr(la, lb, lc, den, V, avid)
        P = _rot(R, xyz, t)
        if o["smooth"]:
            a = _attr(la, lb, lc, den, np.asarray(job["normals"], np.float32).reshape(-1, 3).astype(dtype), avid)
            m = _rot(R, a)
        else:
            cam = s["cam"]
            u, v = cam[vid[:, 1]] - cam[vid[:, 0]], cam[vid[:, 2]] - cam[vid[:, 0]]
            with np.errstate(all="ignore"):
                m = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                              u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
            out["U"][s_, jj, ii] = np.maximum(np.abs(u).max(1), np.abs(v).max(1))
        with np.errstate(all="ignore"):
            mlen = np.sqrt(_dot(m, m))
            ok = (mlen > 0) & (mlen < np.inf)
            n = np.where(ok[:, None], m / mlen[:, None], dtype(0))
            if not o["smooth"]:
                fd = _dot(n, P)
                out["flip_dot"][s_, jj, ii] = fd
                if mutant != "flat_normal_not_flipped":
                    n = np.where((fd > 0)[:, None], -n, n)
            d = light[None, :] - P
            dlen = np.sqrt(_dot(d, d))
            L = d if mutant == "L_not_normalised" else d / dlen[:, None]
            diffuse = np.where(ok, np.fmax(_dot(L, n), dtype(0)), dtype(0))
            light_w = ambient + diffuse
            if mutant != "light_w_not_clamped":
                light_w = np.fmin(light_w, dtype(1))
        if o["use_colors"]:
            col = _attr(la, lb, lc, den, np.asarray(job["colors"], np.float32).reshape(-1, 3).astype(dtype), avid)
        else:
            col = np.broadcast_to(np.asarray(job.get("surf_color", (0.5, 0.5, 0.5)), np.float32).astype(dtype), (len(f), 3))
        out["xyz"][s_, jj, ii] = xyz
        out["normal"][s_, jj, ii] = n
        out["rgb"][s_, jj, ii] = light_w[:, None] * col
        out["mlen"][s_, jj, ii] = mlen
        out["dlen"][s_, jj, ii] = dlen
    return out


def decode(keys):
    """(depth float32, job_id int32, face_id int32) of a key canvas; -1 ids where empty."""
    hit = keys != 0
    low = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return depth, np.where(hit, low >> FACE_BITS, -1).astype(np.int32), np.where(hit, low & FACE_MASK, -1).astype(np.int32)


def shade_f32(jobs, width, height, near, n_slots=None, mutant=None, **opts):
    """The transcription of both passes: dict(keys, depth, face_id, job_id, xyz, normal, rgb, straddle)."""
    keys, straddle = visibility_f32(jobs, width, height, near, n_slots, mutant)
    depth, job_id, face_id = decode(keys)
    r = _resolve(job_id, face_id, jobs, width, height, np.float32(near), np.float32, opts, mutant)
    return dict(keys=keys, depth=depth, face_id=face_id, job_id=job_id, xyz=r["xyz"], normal=r["normal"], rgb=r["rgb"],
                straddle=straddle)


def shade_f64(jobs, width, height, near, keys32, n_slots=None, **opts):
    """The oracle: dict(depth, face_id, job_id, xyz, normal, rgb) in float64, ``masked`` bool [n_slots,H,W] and the bounds
    ``depth_rel`` (render_f64's), ``xyz`` (one number), ``normal`` and ``rgb`` (per pixel, [n_slots,H,W]): outside the mask the
    ids equal the transcription's and every float32 output lies within its bound of the oracle's, per component.

    Masked: (1) as render_f64, the boxes of the faces whose float64 snap or near-plane status differs from the float32 one;
    (2) the pixels whose float32 winner (``keys32``) is not the oracle's: that happens only where two depths lie within the
    depth bound of each other, which is asserted here; (3) flat shading: the pixels where the sign test dot(n, P) > 0 lies
    within its own error of 0.

    Bounds, first order in eps = 2^-24, each doubled for slack as render_f64's.  r = the largest S / Z of render_f64 (6 r eps
    bounds a camera coordinate's relative error), Smax = the largest S over the three rows and all vertices, rho = the largest
    row sum of |R|.
      weights  l = fl(fl(E) w): E's conversion, w = 1 / Z ((6 r + 1) eps) and the product:  dl = (6 r + 3) eps, all l >= 0.
      attribute  the numerator's terms carry dl + eps (product) + 2 eps (two sums), the denominator dl + 2 eps without
               cancellation, the division eps:  |A - A*| <= (2 dl + 6 eps) max|A| = (12 r + 12) eps max|A| =: b_A max|A|.
      xyz      b_A max|vertex coordinate|.
      P        e_P = rho e_xyz + 4 eps Smax (three products, three sums);  d = light - P:  e_d = e_P + eps |d|.
      unit     v / |v| for a vector with component error e:  sqrt(3) e / |v| (the direction's sensitivity) + 4 eps (three
               squares and two sums of one sign, the root, the division).
      smooth   a = A(normals): b_A max|normal|;  m = R a:  e_m = rho (e_a + 3 eps max|normal|);  n: unit(e_m, |m|).
      flat     the camera vertices carry 6 eps Smax each, u = P_b - P_a: e_u = 12 eps Smax + eps U with U the largest |u|, |v|
               component;  m = u x v: e_m = 4 U e_u + 6 eps U^2;  n: unit(e_m, |m|).
      L        unit(e_d, |d|).
      rgb      diffuse: e_f = 3 (e_L + e_n) + 3 eps (|L|, |n| components <= 1; max and min are 1-Lipschitz);  light_w:
               e_w = e_f + (|ambient| + 1) eps;  colour: e_c = b_A max|colour| (0 for a surf_color);
               rgb = light_w colour:  e_w max|colour| + max(1, |ambient|) e_c + eps max|colour|."""
    o = dict(DEFAULTS, **opts)
    n_slots = _n_slots(jobs, n_slots)
    depth64, masked, rel = MR.render_f64(jobs, width, height, near, n_slots)
    slot, pix, z, ids, _ = _samples(jobs, width, height, near, np.float64)
    order = np.lexsort((ids, z, pix, slot))
    slot, pix, z, ids = slot[order], pix[order], z[order], ids[order]
    cell = slot * (height * width) + pix
    first = np.ones(len(cell), bool)
    first[1:] = cell[1:] != cell[:-1]
    job_id = np.full(n_slots * height * width, -1, np.int64)
    face_id = job_id.copy()
    job_id[cell[first]] = ids[first] >> FACE_BITS
    face_id[cell[first]] = ids[first] & FACE_MASK
    job_id, face_id = job_id.reshape(n_slots, height, width), face_id.reshape(n_slots, height, width)
    # (2) the float32 winner against the oracle's
    _d32, j32, f32 = decode(keys32)
    differ = (j32 != job_id) | (f32 != face_id)
    free = differ & ~masked
    if free.any():
        assert ((j32 >= 0) == (job_id >= 0))[free].all(), "coverage differs outside the oracle's mask"
        table = np.sort(cell * (1 << 32) + ids)                    # every (pixel, id) sample, to look its float64 depth up
        zs = z[np.argsort(cell * (1 << 32) + ids)]
        cells = np.nonzero(free.reshape(-1))[0]
        want = cells * (1 << 32) + ((j32.reshape(-1)[cells].astype(np.int64) << FACE_BITS) | f32.reshape(-1)[cells])
        at = np.searchsorted(table, want)
        assert (at < len(table)).all() and (table[np.minimum(at, len(table) - 1)] == want).all(), \
            "the float32 winner is not a float64 sample of its pixel"
        zw = depth64.reshape(-1)[cells]
        assert (np.abs(zs[at] - zw) <= 2 * rel * zw).all(), "winners differ although their depths lie apart"
    masked = masked | differ
    r = _resolve(job_id, face_id, jobs, width, height, float(np.float32(near)), np.float64, opts)
    # bounds
    eps = EPS32
    worst, Smax, rho, vmax, nmax, cmax = 1.0, 0.0, 0.0, 0.0, 0.0, 0.0
    for job in jobs:
        s = _setup(job, np.float64, float(np.float32(near)), width, height)
        keep = s["status"] == 1
        if not keep.any():
            continue
        R = np.abs(MR._f32(job["R"]).reshape(3, 3).astype(np.float64))
        t = np.abs(MR._f32(job["t"]).reshape(3).astype(np.float64))
        p = np.abs(np.asarray(job["vertices"], np.float64).reshape(-1, 3))
        used = np.unique(s["vid"][keep])
        S = p[used] @ R.T + t[None, :]
        worst = max(worst, float((S[:, 2] / s["cam"][used, 2]).max()))
        Smax, rho, vmax = max(Smax, float(S.max())), max(rho, float(R.sum(1).max())), max(vmax, float(p[used].max()))
        if o["smooth"]:
            nmax = max(nmax, float(np.abs(np.asarray(job["normals"], np.float64)).max()))
        cmax = max(cmax, float(np.abs(np.asarray(job["colors"] if o["use_colors"] else job.get("surf_color", (0.5,) * 3),
                                                np.float64)).max()))
    b_A = (12.0 * worst + 12.0) * eps
    e_xyz = b_A * vmax
    e_P = rho * e_xyz + 4 * eps * Smax
    with np.errstate(all="ignore"):
        unit = lambda e, length: np.sqrt(3.0) * e / length + 4 * eps
        if o["smooth"]:
            e_n = unit(rho * (b_A * nmax + 3 * eps * nmax), r["mlen"])
        else:
            e_u = 12 * eps * Smax + eps * r["U"]
            e_n = unit(4 * r["U"] * e_u + 6 * eps * r["U"] ** 2, r["mlen"])
            Pmax = np.abs(_rot_all(r, jobs, job_id)).max(-1)
            margin = 2 * 3 * (e_n * Pmax + e_P)
            masked = masked | ((job_id >= 0) & ~(np.abs(r["flip_dot"]) > margin))       # (3); a NaN is masked too
        e_L = unit(e_P + eps * r["dlen"], r["dlen"])
        e_w = 3 * (e_L + e_n) + 3 * eps + (abs(float(o["ambient"])) + 1) * eps
        e_c = b_A * cmax if o["use_colors"] else 0.0
        e_rgb = e_w * cmax + max(1.0, abs(float(o["ambient"]))) * e_c + eps * cmax
    fill = lambda b: np.where(job_id >= 0, np.nan_to_num(b, nan=np.inf), 0.0)
    return dict(depth=depth64, face_id=face_id, job_id=job_id, xyz=r["xyz"], normal=r["normal"], rgb=r["rgb"],
                masked=masked, bounds=dict(depth_rel=rel, xyz=2 * e_xyz, normal=fill(2 * e_n), rgb=fill(2 * e_rgb)))


def _rot_all(r, jobs, job_id):
    """The eye point P = R xyz + t of every pixel in float64 (0 where empty)."""
    P = np.zeros(job_id.shape + (3,))
    for k, job in enumerate(jobs):
        sel = job_id == k
        if sel.any():
            P[sel] = _rot(MR._f32(job["R"]).reshape(9).astype(np.float64), r["xyz"][sel], MR._f32(job["t"]).reshape(3).astype(np.float64))
    return P


def compare(got, oracle):
    """Asserts, outside the oracle's mask, equal ids, the depth bound and the bounds of xyz, normal and rgb of ``got`` (the
    transcription's or the kernel's outputs); returns the largest masked share of a canvas."""
    free = ~oracle["masked"]
    b = oracle["bounds"]
    assert (got["face_id"] == oracle["face_id"])[free].all() and (got["job_id"] == oracle["job_id"])[free].all()
    err = np.abs(got["depth"].astype(np.float64) - oracle["depth"])[free]
    assert (err <= b["depth_rel"] * oracle["depth"][free]).all(), "depth beyond its bound"
    for name in ("xyz", "normal", "rgb"):
        err = np.abs(got[name].astype(np.float64) - oracle[name]).max(-1)
        bound = b[name] if np.ndim(b[name]) == 0 else b[name][free]
        worst = float((err[free] / np.maximum(bound, 1e-300)).max()) if free.any() else 0.0
        assert (err[free] <= bound).all(), f"{name} off by {worst:.3g} times its bound"
    return max(float(m.mean()) for m in oracle["masked"])

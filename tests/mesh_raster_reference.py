"""Two CPU rasterizers for pgr_mesh_depth, both written from the rules at the top of pegasus_amd/csrc/meshraster.hip.h.

``render_f32``   the float32 transcription: the same operations in the same order, so the kernel's output equals it bit
                 for bit (coverage and depth).
``render_f64``   a float64 oracle.  It projects, snaps and interpolates depth in float64 (the integer edge test on the
                 snapped coordinates is exact in both and shared; tests/test_mesh_raster_host.py pins it by hand); where a face's float64 snap (or its near-plane decision) differs from the float32
                 one, the pixels of the face's box (either version) are masked: there the two may legitimately disagree.
                 Outside the mask the coverage is equal and the depth agrees within ``rel_bound`` (derived below).

A job is a dict(vertices [V,3] f32, faces [F,3] i32, R [3,3], t [3], fx, fy, cx, cy, slot)."""
import numpy as np

SNAP_LIMIT = float(2 ** 30)
EMPTY = np.uint32(0xFFFFFFFF)
EPS32 = 2.0 ** -24


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _project(job, dtype):
    """Camera coordinates and image coordinates of every vertex in ``dtype`` arithmetic, in the header's order."""
    v = np.asarray(job["vertices"], np.float32).reshape(-1, 3).astype(dtype)
    R = _f32(job["R"]).reshape(9).astype(dtype)
    t = _f32(job["t"]).reshape(3).astype(dtype)
    fx, fy, cx, cy = (_f32(job[k]).astype(dtype) for k in ("fx", "fy", "cx", "cy"))
    px, py, pz = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        X = ((R[0] * px + R[1] * py) + R[2] * pz) + t[0]
        Y = ((R[3] * px + R[4] * py) + R[5] * pz) + t[1]
        Z = ((R[6] * px + R[7] * py) + R[8] * pz) + t[2]
        u = (fx * X) / Z + cx
        w = (fy * Y) / Z + cy
    return X, Y, Z, u, w


def _snap(u):
    with np.errstate(all="ignore"):
        q = u * u.dtype.type(256) - u.dtype.type(128)
        return np.rint(np.fmin(np.fmax(q, u.dtype.type(-SNAP_LIMIT)), u.dtype.type(SNAP_LIMIT))).astype(np.int64)


def _edge(px, py, qx, qy, x, y):
    return (qx - px) * (y - py) - (qy - py) * (x - px)


def _bias(px, py, qx, qy):
    dx, dy = qx - px, qy - py
    return np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, 1)


def _faces_setup(job, sx, sy, Z, near, W, H):
    """Per face: status (0 dropped, 1 rasterise, 2 straddles), oriented integer vertices [F,3], vertex order [F,3], box."""
    f = np.asarray(job["faces"], np.int64).reshape(-1, 3)
    nv = len(sx)
    ok = ((f >= 0) & (f < nv)).all(1)
    fi = np.where(ok[:, None], f, 0)
    behind = (Z[fi] < near).sum(1) if nv else np.zeros(len(f), np.int64)
    x, y = (sx[fi], sy[fi]) if nv else (np.zeros((len(f), 3), np.int64),) * 2
    area2 = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    order = np.where((area2 < 0)[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    x, y = np.take_along_axis(x, order, 1), np.take_along_axis(y, order, 1)
    i0 = np.maximum(0, (x.min(1) + 255) >> 8); i1 = np.minimum(W - 1, x.max(1) >> 8)
    j0 = np.maximum(0, (y.min(1) + 255) >> 8); j1 = np.minimum(H - 1, y.max(1) >> 8)
    status = np.where(~ok | (behind == 3), 0, np.where(behind > 0, 2, np.where((area2 == 0) | (i0 > i1) | (j0 > j1), 0, 1)))
    return status, x, y, np.take_along_axis(fi, order, 1), np.abs(area2), (i0, i1, j0, j1)


def _covered_samples(x, y, box, small=8):
    """Yields (face indices, i, j, ea, eb, ec) of all covered samples: faces with a small box together, one box offset at
    a time; the others one by one."""
    i0, i1, j0, j1 = box
    ba = _bias(x[:, 1], y[:, 1], x[:, 2], y[:, 2]); bb = _bias(x[:, 2], y[:, 2], x[:, 0], y[:, 0])
    bc = _bias(x[:, 0], y[:, 0], x[:, 1], y[:, 1])

    def test(idx, i, j):
        X, Y = i << 8, j << 8
        ea = _edge(x[idx, 1], y[idx, 1], x[idx, 2], y[idx, 2], X, Y)
        eb = _edge(x[idx, 2], y[idx, 2], x[idx, 0], y[idx, 0], X, Y)
        ec = _edge(x[idx, 0], y[idx, 0], x[idx, 1], y[idx, 1], X, Y)
        hit = (ea >= ba[idx]) & (eb >= bb[idx]) & (ec >= bc[idx])
        return hit, ea, eb, ec
    bw, bh = i1 - i0 + 1, j1 - j0 + 1
    is_small = (bw <= small) & (bh <= small)
    idx = np.nonzero(is_small)[0]
    if len(idx):
        for dj in range(int(bh[idx].max())):
            for di in range(int(bw[idx].max())):
                sel = idx[(di < bw[idx]) & (dj < bh[idx])]
                if not len(sel):
                    continue
                i, j = i0[sel] + di, j0[sel] + dj
                hit, ea, eb, ec = test(sel, i, j)
                yield sel[hit], i[hit], j[hit], ea[hit], eb[hit], ec[hit]
    for f in np.nonzero(~is_small)[0]:
        jj, ii = np.meshgrid(np.arange(j0[f], j1[f] + 1), np.arange(i0[f], i1[f] + 1), indexing="ij")
        ii, jj = ii.ravel(), jj.ravel()
        fidx = np.full(len(ii), f)
        hit, ea, eb, ec = test(fidx, ii, jj)
        yield fidx[hit], ii[hit], jj[hit], ea[hit], eb[hit], ec[hit]


def render_f32(jobs, width, height, near, n_slots=None):
    """(depth float32 [n_slots,H,W], faces dropped for straddling ``near``): the transcription."""
    n_slots = (max(j["slot"] for j in jobs) + 1 if jobs else 1) if n_slots is None else n_slots
    out = np.full((n_slots, height * width), EMPTY, np.uint32)
    straddle = 0
    near = np.float32(near)
    for job in jobs:
        _X, _Y, Z, u, v = _project(job, np.float32)
        sx, sy = _snap(u), _snap(v)
        with np.errstate(all="ignore"):
            inv = np.float32(1) / Z
        status, x, y, vid, area2, box = _faces_setup(job, sx, sy, Z, near, width, height)
        straddle += int((status == 2).sum())
        keep = np.nonzero(status == 1)[0]
        if not len(keep):
            continue
        x, y, vid, area2 = x[keep], y[keep], vid[keep], area2[keep]
        box = tuple(b[keep] for b in box)
        w = inv[vid]
        for f, i, j, ea, eb, ec in _covered_samples(x, y, box):
            with np.errstate(all="ignore"):
                den = (ea.astype(np.float32) * w[f, 0] + eb.astype(np.float32) * w[f, 1]) + ec.astype(np.float32) * w[f, 2]
                z = area2[f].astype(np.float32) / den
            good = (den > 0) & (z > 0) & (z < np.inf)
            np.minimum.at(out[job["slot"]], (j * width + i)[good], z[good].view(np.uint32))
    out[out == EMPTY] = 0
    return out.view(np.float32).reshape(n_slots, height, width), straddle


def render_f64(jobs, width, height, near, n_slots=None):
    """(depth float64 [n_slots,H,W], masked bool [n_slots,H,W], rel_bound): the oracle.

    rel_bound: outside the mask a float32 depth may differ from the oracle's by rel_bound * depth.  The float32 pipeline
    rounds (a) each camera Z: three products and three sums, at most 6 eps (|R6 x| + |R7 y| + |R8 z| + |t2|) absolute,
    i.e. 6 eps S / Z relative with S that sum -- the largest S / Z over all vertices enters; (b) w = 1 / Z: eps; (c) the
    three int64 -> float32 conversions, the three products and two sums of den, all of one sign (E >= 0, w > 0: no
    cancellation): 3 eps on every term; (d) the conversion of area2 and the division: 2 eps.  Sum: (6 S/Z + 6) eps, doubled
    for slack in the first-order bookkeeping; eps = 2^-24."""
    n_slots = (max(j["slot"] for j in jobs) + 1 if jobs else 1) if n_slots is None else n_slots
    depth = np.full((n_slots, height * width), np.inf)
    masked = np.zeros((n_slots, height, width), bool)
    worst = 1.0
    for job in jobs:
        _X, _Y, Z, u, v = _project(job, np.float64)
        _, _, Z32, u32, v32 = _project(job, np.float32)
        sx, sy = _snap(u), _snap(v)
        tx, ty = _snap(u32), _snap(v32)
        status, x, y, vid, area2, box = _faces_setup(job, sx, sy, Z, float(np.float32(near)), width, height)
        status32, _x32, _y32, _vid32, _a32, box32 = _faces_setup(job, tx, ty, Z32, np.float32(near), width, height)
        f = np.asarray(job["faces"], np.int64).reshape(-1, 3)
        valid = ((f >= 0) & (f < len(sx))).all(1)
        fi = np.where(valid[:, None], f, 0)
        differs = valid & (((sx[fi] != tx[fi]) | (sy[fi] != ty[fi])).any(1) | (status != status32))
        for k in np.nonzero(differs)[0]:
            for b in (box, box32):
                if b[0][k] <= b[1][k] and b[2][k] <= b[3][k]:
                    masked[job["slot"], b[2][k]:b[3][k] + 1, b[0][k]:b[1][k] + 1] = True
        keep = np.nonzero(status == 1)[0]
        if not len(keep):
            continue
        R, t = _f32(job["R"]).reshape(9).astype(np.float64), _f32(job["t"]).reshape(3).astype(np.float64)
        p = np.abs(np.asarray(job["vertices"], np.float64).reshape(-1, 3))
        S = np.abs(R[6]) * p[:, 0] + np.abs(R[7]) * p[:, 1] + np.abs(R[8]) * p[:, 2] + abs(t[2])
        used = np.unique(vid[keep])
        worst = max(worst, float((S[used] / Z[used]).max()))
        x, y, vid, area2 = x[keep], y[keep], vid[keep], area2[keep]
        inv = 1.0 / Z[vid]
        for ff, i, j, ea, eb, ec in _covered_samples(x, y, tuple(b[keep] for b in box)):
            z = area2[ff] / (ea * inv[ff, 0] + eb * inv[ff, 1] + ec * inv[ff, 2])
            np.minimum.at(depth[job["slot"]], j * width + i, z)
    depth[np.isinf(depth)] = 0.0
    return depth.reshape(n_slots, height, width), masked, 2.0 * (6.0 * worst + 6.0) * EPS32


def compare(depth32, depth64, masked, rel_bound):
    """Asserts coverage equality and the depth bound outside the mask; returns the masked share."""
    free = ~masked
    assert ((depth32 > 0) == (depth64 > 0))[free].all(), "coverage differs outside the oracle's mask"
    err = np.abs(depth32.astype(np.float64) - depth64)[free]
    assert (err <= rel_bound * depth64[free]).all(), f"depth off by {float((err / np.maximum(depth64[free], 1e-300)).max()):.3g} relative, bound {rel_bound:.3g}"
    return float(masked.mean())

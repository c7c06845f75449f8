"""NumPy restatements of the three texture rules, written from the comments above the kernels:

``shade_textured_f32``   pgr_mesh_shade_textured (above mesh_shade_kernel in pegasus_amd/csrc/meshraster.hip.h), on top of the
                         transcription of pgr_mesh_visibility + pgr_mesh_shade in tests/mesh_shade_reference.py.
``atlas_points_f32``     pgr_mesh_atlas_points (pegasus_amd/csrc/meshattr.hip.h).
``atlas_pack``           pgr_mesh_atlas_pack (same header).

The kernels' outputs equal these bit for bit (a NaN equals a NaN whatever its payload).  ``atlas_layout`` restates the layout of
pegasus_amd.mesh.texture_atlas_layout independently, and ``footprint`` lists the texels a sample reads with their weights.

The rules (restated).
  uv        (u, v) = ((la A_a + lb A_b) + lc A_c) / den on the face's corner values, b's and c's swapped when the face was
            flipped; la, lb, lc, den as in mesh_shade_reference.
  texture   W x H texels, stored row 0 is the image's top row, v = 0 its bottom row: texel (i, j) is stored row H - 1 - j.
            clamp(x, n) = x >= 0 ? (x < n ? (int)x : n - 1) : 0.
  nearest   i = clamp(floor(u W), W), j = clamp(floor(v H), H), colour = texel / 255.
  bilinear  x = u W - 0.5, x0 = floor(x), fx = x - x0 (0 when NaN), i0 = clamp(x0), i1 = clamp(x0 + 1); y alike;
            top = (1 - fx) c00 + fx c10, bot = (1 - fx) c01 + fx c11, colour = (1 - fy) top + fy bot.
  rgb       light_w * colour; a job with texture -1 keeps pgr_mesh_shade's rgb.
  atlas     cell side s, leg L = s - 3, cells = ceil(F / 2), cols = ceil(sqrt(cells)), rows = ceil(cells / cols); face f in cell
            f >> 1, half f & 1; texel (i, j) of a cell belongs to half 0 when i + j <= s - 1; (di, dj) = (i, j) in half 0 and
            (s - 1 - i, s - 1 - j) in half 1; beta = di / L, gamma = dj / L; p = (A + beta (B - A)) + gamma (C - A).
  pack      q = rint(255 c) for seen texels; a face's unseen texels get (2 sum + cnt) / (2 cnt) of its seen ones, or its
            face_fill row (or fill) when it has none; texels of no face get fill.
"""
import numpy as np

import mesh_raster_reference as MR
import mesh_shade_reference as SR

F32 = np.float32
SHADE_MUTANTS = ("v_not_flipped", "uv_not_swapped_on_flip", "screen_space_uv", "wrap_repeat", "nearest_rounds",
                 "bilinear_no_half_texel", "texture_offset_ignored")
ATLAS_MUTANTS = ("half1_not_mirrored", "antidiagonal_to_half1", "unseen_mean_truncates")
MUTANTS = SHADE_MUTANTS + ATLAS_MUTANTS


def pack_textures(images, lead=5, gap=1):
    """(texels uint8 [n], table [(offset, width, height)]) of uint8 [h,w,3] images: ``lead`` bytes in front of the first and
    ``gap`` between two, so that no texture starts at 0 or on a 4-byte boundary by construction."""
    parts, table, at = [np.full(lead, 0xEE, np.uint8)], [], lead
    for im in images:
        im = np.ascontiguousarray(im, np.uint8)
        table.append((at, im.shape[1], im.shape[0]))
        parts += [im.reshape(-1), np.full(gap, 0xEE, np.uint8)]
        at += im.size + gap
    return np.concatenate(parts), table


def _clamp(x, n, mutant=None):
    """clamp(x, n) of the rule as int64; x float32."""
    safe = np.clip(np.nan_to_num(x, nan=0.0, posinf=float(n), neginf=-1.0), -1.0, float(n)).astype(np.int64)
    if mutant == "wrap_repeat":
        return np.mod(safe, n)
    return np.where(x >= 0, np.where(x < F32(n), safe, n - 1), 0)


def _texel(texels, entry, i, j, mutant=None):
    """Texel (i, j) / 255 in float32 [N,3]; j counts from the image's bottom row."""
    off, w, h = entry
    if mutant == "texture_offset_ignored":
        off = 0
    row = j if mutant == "v_not_flipped" else h - 1 - j
    at = off + (row * w + i) * 3
    return texels[at[:, None] + np.arange(3)[None, :]].astype(F32) / F32(255.0)


def sample(texels, entry, u, v, bilinear, mutant=None):
    """The colour float32 [N,3] the rule reads at (u, v) float32 [N] from texture ``entry`` = (offset, width, height)."""
    _off, w, h = entry
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    with np.errstate(all="ignore"):
        if not bilinear:
            rnd = np.rint if mutant == "nearest_rounds" else np.floor
            i, j = _clamp(rnd(u * F32(w)), w, mutant), _clamp(rnd(v * F32(h)), h, mutant)
            return _texel(texels, entry, i, j, mutant)
        half = F32(0.0) if mutant == "bilinear_no_half_texel" else F32(0.5)
        x, y = u * F32(w) - half, v * F32(h) - half
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = x - x0, y - y0
        fx, fy = np.where(np.isnan(fx), F32(0), fx)[:, None], np.where(np.isnan(fy), F32(0), fy)[:, None]
        i0, i1 = _clamp(x0, w, mutant), _clamp(x0 + F32(1), w, mutant)
        j0, j1 = _clamp(y0, h, mutant), _clamp(y0 + F32(1), h, mutant)
        one = F32(1)
        top = (one - fx) * _texel(texels, entry, i0, j0, mutant) + fx * _texel(texels, entry, i1, j0, mutant)
        bot = (one - fx) * _texel(texels, entry, i0, j1, mutant) + fx * _texel(texels, entry, i1, j1, mutant)
        return ((one - fy) * top + fy * bot).astype(F32)


def footprint(entry, u, v, bilinear):
    """[(i, j, weight)] of the texels one sample reads (j from the bottom row), weights in float32 as the rule forms them;
    texels that coincide after the clamp are listed once with their weights added in float64."""
    _off, w, h = entry
    u, v = np.asarray([u], F32), np.asarray([v], F32)
    if not bilinear:
        return [(int(_clamp(np.floor(u * F32(w)), w)[0]), int(_clamp(np.floor(v * F32(h)), h)[0]), 1.0)]
    x, y = u * F32(w) - F32(0.5), v * F32(h) - F32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = float((x - x0)[0]), float((y - y0)[0])
    out = {}
    for i, wx in ((int(_clamp(x0, w)[0]), 1.0 - fx), (int(_clamp(x0 + F32(1), w)[0]), fx)):
        for j, wy in ((int(_clamp(y0, h)[0]), 1.0 - fy), (int(_clamp(y0 + F32(1), h)[0]), fy)):
            out[(i, j)] = out.get((i, j), 0.0) + wx * wy
    return [(i, j, wgt) for (i, j), wgt in out.items()]


def shade_textured_f32(jobs, width, height, near, texels, table, n_slots=None, bilinear=False, mutant=None, **opts):
    """The transcription of pgr_mesh_visibility + pgr_mesh_shade_textured: the dict of mesh_shade_reference.shade_f32 plus
    ``uv`` float32 [n_slots,H,W,2].  A job may carry ``corner_uv`` float32 [F,3,2] (else zeros) and ``texture`` (an index into
    ``table``, default -1)."""
    out = SR.shade_f32(jobs, width, height, near, n_slots, **opts)
    job_id, face_id = out["job_id"], out["face_id"]
    # light_w of every covered pixel: the rgb of a white surf colour
    white = [dict(j, surf_color=(1.0, 1.0, 1.0)) for j in jobs]
    light_w = SR._resolve(job_id, face_id, white, width, height, F32(near), F32, dict(opts, use_colors=False))["rgb"][..., 0]
    uv = np.zeros(job_id.shape + (2,), F32)
    rgb = out["rgb"].copy()
    for k, job in enumerate(jobs):
        s_, jj, ii = np.nonzero(job_id == k)
        if not len(s_):
            continue
        f = face_id[s_, jj, ii]
        s = SR._setup(job, F32, F32(near), width, height)
        x, y, vid = s["x"][f], s["y"][f], s["vid"][f]
        w = s["inv"][vid]
        X, Y = ii.astype(np.int64) << 8, jj.astype(np.int64) << 8
        ea = MR._edge(x[:, 1], y[:, 1], x[:, 2], y[:, 2], X, Y)
        eb = MR._edge(x[:, 2], y[:, 2], x[:, 0], y[:, 0], X, Y)
        ec = MR._edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], X, Y)
        la, lb, lc = ea.astype(F32) * w[:, 0], eb.astype(F32) * w[:, 1], ec.astype(F32) * w[:, 2]
        if mutant == "screen_space_uv":
            la, lb, lc = ea.astype(F32), eb.astype(F32), ec.astype(F32)
        den = (la + lb) + lc
        raw = np.asarray(job["faces"], np.int64).reshape(-1, 3)[f]
        flipped = MR._edge(s["sx"][raw[:, 0]], s["sy"][raw[:, 0]], s["sx"][raw[:, 1]], s["sy"][raw[:, 1]], s["sx"][raw[:, 2]],
                           s["sy"][raw[:, 2]]) < 0
        if mutant == "uv_not_swapped_on_flip":
            flipped = np.zeros_like(flipped)
        cuv = np.asarray(job.get("corner_uv", np.zeros((len(job["faces"]), 3, 2))), F32).reshape(-1, 3, 2)[f]
        a, b, c = cuv[:, 0], np.where(flipped[:, None], cuv[:, 2], cuv[:, 1]), np.where(flipped[:, None], cuv[:, 1], cuv[:, 2])
        with np.errstate(all="ignore"):
            val = ((la[:, None] * a + lb[:, None] * b) + lc[:, None] * c) / den[:, None]
        uv[s_, jj, ii] = val
        t = int(job.get("texture", -1))
        if t >= 0:
            col = sample(texels, table[t], val[:, 0], val[:, 1], bilinear, mutant)
            with np.errstate(all="ignore"):
                rgb[s_, jj, ii] = light_w[s_, jj, ii][:, None] * col
    return dict(out, rgb=rgb, uv=uv)


def same_bits(a, b):
    """Element-wise: equal bits, or both NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a == b
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- the per-face atlas -----------------------------------------------------------------------------------------------
def atlas_layout(n_faces, cell):
    """(width, height, cols, rows, corner_xy float64 [F,3,2] in atlas texel-centre coordinates, corner_uv float32 [F,3,2]),
    restated face by face from the rule."""
    cells = -(-n_faces // 2)
    cols = 1
    while cols * cols < cells:
        cols += 1
    rows = -(-cells // cols)
    width, height, s, L = cols * cell, rows * cell, cell, cell - 3
    xy = np.zeros((n_faces, 3, 2))
    for f in range(n_faces):
        c, half = f >> 1, f & 1
        ox, oy = (c % cols) * s, (c // cols) * s
        if half == 0:
            local = [(0.5, 0.5), (0.5 + L, 0.5), (0.5, 0.5 + L)]
        else:
            local = [(s - 0.5, s - 0.5), (s - 0.5 - L, s - 0.5), (s - 0.5, s - 0.5 - L)]
        xy[f] = [(ox + x, oy + y) for x, y in local]
    uv = np.stack([xy[..., 0] / width, 1.0 - xy[..., 1] / height], -1).astype(F32)
    return width, height, cols, rows, xy, uv


def atlas_owner(n_faces, cell, mutant=None):
    """(face int64 [H,W] by the layout alone (may be >= n_faces), half, i, j) of every atlas texel."""
    width, height, cols, _rows, _xy, _uv = atlas_layout(n_faces, cell)
    Y, X = np.mgrid[0:height, 0:width]
    i, j = X % cell, Y % cell
    limit = cell - 2 if mutant == "antidiagonal_to_half1" else cell - 1
    half = (i + j > limit).astype(np.int64)
    return 2 * ((Y // cell) * cols + X // cell) + half, half, i, j


def atlas_points_f32(vertices, faces, cell, mutant=None):
    """The restatement of pgr_mesh_atlas_points: (points float32 [H*W,3], normals float32 [H*W,3], face_of_texel int32 [H*W])."""
    V = np.asarray(vertices, F32).reshape(-1, 3)
    Fc = np.asarray(faces, np.int64).reshape(-1, 3)
    nF, L = len(Fc), cell - 3
    f, half, i, j = (a.reshape(-1) for a in atlas_owner(nF, cell, mutant))
    n = len(f)
    points, normals, owner = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.full(n, -1, np.int32)
    inside = f < nF
    fi = np.where(inside, f, 0)
    ok = inside & ((Fc[fi] >= 0) & (Fc[fi] < len(V))).all(1)
    idx = np.where(ok[:, None], Fc[fi], 0)
    if len(V) == 0:
        return points, normals, owner
    A, B, C = V[idx[:, 0]], V[idx[:, 1]], V[idx[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = B - A, C - A
        m = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        ok &= (length > 0) & (length < np.inf)
        mirrored = (half == 1) & (mutant != "half1_not_mirrored")
        di, dj = np.where(mirrored, cell - 1 - i, i), np.where(mirrored, cell - 1 - j, j)
        beta, gamma = (di.astype(F32) / F32(L))[:, None], (dj.astype(F32) / F32(L))[:, None]
        p = (A + beta * e1) + gamma * e2
        nrm = m / length[:, None]
    points[ok], normals[ok], owner[ok] = p[ok], nrm[ok], f[ok].astype(np.int32)
    return points, normals, owner


def quantise(c):
    """(uint8) rintf(255 c), a NaN gives 0."""
    with np.errstate(all="ignore"):
        v = F32(255.0) * np.asarray(c, F32)
    return np.where(np.isnan(v), 0, np.clip(np.rint(np.nan_to_num(v, nan=0.0)), 0, 255)).astype(np.uint8)


def atlas_pack(n_faces, cell, face_of_texel, colors, seen, face_fill=None, fill=(128, 128, 128), mutant=None):
    """The restatement of pgr_mesh_atlas_pack: (texture uint8 [H,W,3], face_seen int32 [F])."""
    width, height = atlas_layout(n_faces, cell)[:2]
    layout_face = atlas_owner(n_faces, cell)[0].reshape(-1)
    owner = np.asarray(face_of_texel, np.int64).reshape(-1)
    owned = owner == layout_face
    seen = np.asarray(seen).reshape(-1) > 0
    q = quantise(np.asarray(colors, F32).reshape(-1, 3))
    fill = np.asarray(fill, np.uint8)
    out = np.broadcast_to(fill, (width * height, 3)).copy()
    face_seen = np.zeros(n_faces, np.int32)
    for f in range(n_faces):
        mine = owned & (layout_face == f)
        lit = mine & seen
        cnt = int(lit.sum())
        face_seen[f] = cnt
        if cnt:
            total = q[lit].astype(np.int64).sum(0)
            mean = total // cnt if mutant == "unseen_mean_truncates" else (2 * total + cnt) // (2 * cnt)
        else:
            mean = fill if face_fill is None else np.asarray(face_fill, np.uint8).reshape(-1, 3)[f]
        out[mine] = mean
        out[lit] = q[lit]
    return out.reshape(height, width, 3), face_seen

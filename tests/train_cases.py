"""Seeded inputs of the training-step and kNN kernel tests (test_train_kernels_host.py, test_train_kernels_gpu.py): small
shapes at which the kernels can go wrong, and the content the trainer feeds them (flat backgrounds, renders close to their
target), not only noise.

Every loss case keeps x - y' (and alpha - mask), taken in float64 from the float32 inputs, either exactly 0 or at least
SEPARATION in magnitude, so that the L1 sign is the same in float32 and float64 and no element has to be left out of a
comparison.  test_train_kernels_host.py checks that on every case.
"""
import zlib

import numpy as np

F32 = np.float32
SEPARATION = 1e-4

# (H, W): one pixel, thin both ways, smaller than the 11-tap window, exactly the window, a tile minus / exactly / plus one
# row, two tiles, ragged in both axes inside the 5-pixel window radius of a tile edge (21 = 16 + 5, 27 = 32 - 5), the
# 26-sample halo, and ragged tiles with more than two tiles per axis
SHAPES = [(1, 1), (1, 300), (300, 1), (5, 6), (11, 11), (15, 16), (16, 16), (17, 16), (16, 32), (21, 27), (26, 26), (33, 47),
          (64, 48)]
ALL_LAMBDAS = [(1, 300), (5, 6), (17, 16), (33, 47)]           # lambda in {0, 0.2, 1}; 0.2 elsewhere
FAMILIES = ("noise", "texture_impulses", "flat_object", "constant", "near_target", "out_of_range", "partly_equal")
WELL_CONDITIONED = ("noise", "texture_impulses")               # elsewhere flat regions: sxx cancels against C2 = 9e-4
FAMILY_SHAPES = {
    "noise": SHAPES,
    "texture_impulses": SHAPES,
    "flat_object": [(1, 300), (11, 11), (17, 16), (21, 27), (33, 47), (64, 48)],
    "constant": [(1, 1), (300, 1), (5, 6), (16, 16), (21, 27), (33, 47)],
    "near_target": [(1, 300), (15, 16), (16, 32), (26, 26), (33, 47), (64, 48)],
    "out_of_range": [(1, 1), (300, 1), (5, 6), (17, 16), (21, 27), (33, 47)],
    "partly_equal": [(1, 300), (5, 6), (16, 16), (21, 27), (33, 47), (64, 48)],
}
CONSTANTS = (0.25, 0.5, 1.0, 0.0)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def separate(x, yt):
    """x with every element that is closer than 2 SEPARATION to yt (but not equal to it) moved to 2 SEPARATION from it."""
    d = x.astype(np.float64) - yt.astype(np.float64)
    close = (d != 0.0) & (np.abs(d) < 2 * SEPARATION)
    out = x.copy()
    out[close] = (yt[close].astype(np.float64) + np.where(d[close] >= 0, 2 * SEPARATION, -2 * SEPARATION)).astype(F32)
    return out


def _smooth(rng, H, W, passes=1):
    """Noise in 0..1 correlated over a few pixels (3x3 box filter, edge padded), stretched back to the full range."""
    t = rng.random((3, H, W))
    for _ in range(passes):
        p = np.pad(t, ((0, 0), (1, 1), (1, 1)), mode="edge")
        t = sum(p[:, i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    lo, hi = t.min(), t.max()
    return ((t - lo) / (hi - lo) if hi > lo else t).astype(F32)


def _object(H, W, dy=0, dx=0):
    """Boolean rectangle covering the middle of the image (at least one pixel), shifted by (dy, dx)."""
    r = np.zeros((H, W), bool)
    y0, y1 = H // 4, max(H // 4 + 1, (3 * H) // 4)
    x0, x1 = W // 4, max(W // 4 + 1, (3 * W) // 4)
    r[max(0, y0 + dy):max(0, y1 + dy), max(0, x0 + dx):max(0, x1 + dx)] = True
    return r


def impulse_pixels(H, W):
    """(channel, row, column) of the single-pixel steps of texture_impulses: tile corners, the image corners, and 5 and 6
    pixels from a tile edge (the window radius is 5), where they fit."""
    want = [(0, 0), (15, 15), (16, 16), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (5, 5), (6, 6), (10, 10), (11, 11), (21, 21),
            (22, 22), (16, 5), (6, 16), (15, 0), (0, 16), (31, 26), (32, 37)]
    seen, out = set(), []
    for r, q in want:
        if 0 <= r < H and 0 <= q < W and (r, q) not in seen:
            seen.add((r, q))
            out.append((len(out) % 3, r, q))
    return out


def image_pair(family, H, W, variant=0):
    """(x, y) float32 [3,H,W] of a content family."""
    rng = _rng(family, H, W, variant)
    if family == "noise":                                  # the existing test's content
        x = rng.random((3, H, W)).astype(F32)
        y = np.clip(x + (0.15 * rng.standard_normal((3, H, W))).astype(F32), 0, 1).astype(F32)
    elif family == "texture_impulses":
        y = _smooth(rng, H, W)
        x = np.clip(y + (0.1 * (_smooth(rng, H, W) - 0.5)).astype(F32), 0, 1).astype(F32)
        x = separate(x, y)
        for c, r, q in impulse_pixels(H, W):
            x[c, r, q] = y[c, r, q] + F32(0.5)
    elif family == "flat_object":
        y = np.ones((3, H, W), F32)
        y[:, _object(H, W)] = 0.3
        x = np.ones((3, H, W), F32)
        x[:, _object(H, W, 2, 2)] = 0.3
        if H > W:
            x[:, : max(1, H // 8), :] = 0.98               # one band, along the short axis
        else:
            x[:, :, : max(1, W // 8)] = 0.98
    elif family == "constant":
        c = F32(CONSTANTS[variant])
        x = np.full((3, H, W), c, F32)
        y = x.copy()
        y[:, (H + 1) // 2:, :] = F32(0.999) * c if c != 0 else c
        if H == 1:
            y[:, :, (W + 1) // 2:] = F32(0.999) * c
    elif family == "near_target":
        y = np.ones((3, H, W), F32)
        y[:, _object(H, W)] = np.array([0.3, 0.55, 0.8], F32)[:, None]
        step = (0.2 + 0.8 * rng.random((3, H, W))) * rng.choice([-1.0, 1.0], size=(3, H, W))
        x = (y + (1e-3 * step).astype(F32)).astype(F32)
    elif family == "out_of_range":
        x = rng.uniform(-1.0, 2.0, size=(3, H, W)).astype(F32)
        y = rng.random((3, H, W)).astype(F32)
    elif family == "partly_equal":
        y = rng.random((3, H, W)).astype(F32)
        x = np.clip(y + (0.15 * rng.standard_normal((3, H, W))).astype(F32), 0, 1).astype(F32)
        x[:, :, : W // 2] = y[:, :, : W // 2]
    else:
        raise KeyError(family)
    return separate(x, y), y


def loss_cases():
    """[dict(name, family, H, W, variant, lams)] of the unmasked loss; image_pair(...) makes the images."""
    out = []
    for fam in FAMILIES:
        for H, W in FAMILY_SHAPES[fam]:
            for variant in range(len(CONSTANTS) if fam == "constant" else 1):
                if fam == "constant" and variant and (H, W) not in ((5, 6), (21, 27)):
                    continue
                lams = (0.0, 0.2, 1.0) if (H, W) in ALL_LAMBDAS else (0.2,)
                name = f"{fam}-{H}x{W}" + (f"-c{CONSTANTS[variant]}" if fam == "constant" else "")
                out.append(dict(name=name, family=fam, H=H, W=W, variant=variant, lams=lams))
    return out


# ---- masked loss ------------------------------------------------------------------------------------------------------------
BACKGROUNDS = ((1.0, 1.0, 1.0), (0.25, 0.6, 0.1))
MASKED_SHAPES = [(1, 300), (5, 6), (17, 16), (21, 27), (33, 47), (64, 48)]


def masked_inputs(kind, H, W, bg):
    """dict(x, y, mask, alpha, bg) float32 of a masked case.
    binary: a 0/1 mask (an object rectangle and scattered pixels); x equals y' bit for bit outside the mask (the render has
            converged to the background there) and differs inside; alpha equals the mask bit for bit on the upper rows / left
            columns, where its sign is 0.
    soft:   the existing test's mask: clamp(1.6 u - 0.3, 0, 1), with exact 0s and 1s and everything between."""
    rng = _rng("masked", kind, H, W, bg)
    bgv = np.asarray(bg, F32)
    y = rng.random((3, H, W)).astype(F32)
    if kind == "binary":
        m = (_object(H, W) | (rng.random((H, W)) < 0.1)).astype(F32)
        yt = np.where(m[None] > 0, y, bgv[:, None, None]).astype(F32)
        x = np.clip(yt + (0.2 * rng.standard_normal((3, H, W))).astype(F32), 0, 1).astype(F32)
        x = np.where(m[None] > 0, x, yt)
    elif kind == "soft":
        m = np.clip(rng.random((H, W)) * 1.6 - 0.3, 0.0, 1.0).astype(F32)
        yt = y.astype(np.float64) * m[None] + bgv.astype(np.float64)[:, None, None] * (1.0 - m.astype(np.float64)[None])
        x = rng.random((3, H, W)).astype(F32)
    else:
        raise KeyError(kind)
    x = separate(x, yt)
    a = np.clip(m + rng.uniform(0.01, 0.9, size=(H, W)).astype(F32) * np.where(m > 0.5, -1, 1).astype(F32), 0, 1).astype(F32)
    a = separate(a, m)
    if kind == "binary":
        if H > 1:
            a[: (H + 1) // 2] = m[: (H + 1) // 2]
        else:
            a[:, : W // 2] = m[:, : W // 2]
    return dict(x=x, y=y, mask=m, alpha=a, bg=bgv)


def masked_cases():
    """[dict(name, kind, H, W, bg, lam, lam_a, use_alpha, want_grad, want_grad_alpha)]: lambda_alpha in {0, 0.5}, with and
    without alpha, with and without the gradients."""
    out = []
    k = 0
    for kind in ("binary", "soft"):
        for H, W in MASKED_SHAPES:
            for bg in BACKGROUNDS:
                use_alpha = k % 4 != 3
                lam_a = 0.5 if (use_alpha and k % 2 == 0) else 0.0
                lam = (0.2, 0.0, 1.0)[k % 3] if (H, W) in ALL_LAMBDAS else 0.2
                out.append(dict(name=f"{kind}-{H}x{W}-bg{bg[0]}-la{lam_a}" + ("" if use_alpha else "-noalpha"), kind=kind,
                                H=H, W=W, bg=bg, lam=lam, lam_a=lam_a, use_alpha=use_alpha, want_grad=k % 5 != 4,
                                want_grad_alpha=use_alpha and k % 7 != 6))
                k += 1
    return out


# ---- Adam -------------------------------------------------------------------------------------------------------------------
ADAM_EDGE_SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]   # around ADAM_BLOCK_ELEMS = 1024
ADAM_START_STEPS = [0, 1, 999, 29998]           # the first step() is step 1, 2, 1000, 29999 (1 - 0.9^29999 rounds to 1)
ADAM_STEPS = 3
GRAD_KINDS = ("wide", "zero", "zero_later", "tiny", "huge", "unit")


def adam_layouts():
    """{name: [group]}, group = dict(sizes, lr, betas, eps, kinds): one optimizer each.
    sixteen          16 non-empty parameters, one per group: ONE launch whose table is full (the first-block search walks
                     all 16 entries)
    sixteen_empties  the same with empty parameters first, in the middle and last (19 entries: the table skips them)
    seventeen        17 parameters with a gradient, two launches; one group holds three parameters; an eighteenth has none
    thirty_three     33 parameters, three launches, two pairs of betas / eps (each pair its own launches)"""
    extra = [3, 512, 64, 3000, 1]
    sizes16 = ADAM_EDGE_SIZES + extra
    kinds = lambda n, k0=0: [GRAD_KINDS[(k0 + i) % len(GRAD_KINDS)] for i in range(n)]
    lrs = [1e-3, 0.05, 0.0, 1.6e-4, 0.0025, 1e-2]
    one_per_group = lambda sizes, **kw: [dict(sizes=[n], lr=lrs[i % len(lrs)], betas=(0.9, 0.999), eps=1e-15,
                                              kinds=kinds(1, i), **kw) for i, n in enumerate(sizes)]
    with_empties = [0] + sizes16[:8] + [0] + sizes16[8:] + [0]
    seventeen = one_per_group(sizes16[:14])
    seventeen.append(dict(sizes=[1025, 7, 2048], lr=0.01, betas=(0.9, 0.999), eps=1e-15, kinds=["wide", "zero", "huge"]))
    seventeen.append(dict(sizes=[300], lr=0.01, betas=(0.9, 0.999), eps=1e-15, kinds=["none"]))
    thirty_three = one_per_group((ADAM_EDGE_SIZES * 2)[:20])
    thirty_three += [dict(sizes=[n], lr=0.02, betas=(0.8, 0.99), eps=1e-8, kinds=kinds(1, i))
                     for i, n in enumerate(ADAM_EDGE_SIZES + [5, 1024])]
    assert sum(len(g["sizes"]) for g in seventeen) == 18 and sum(len(g["sizes"]) for g in thirty_three) == 33
    return {"sixteen": one_per_group(sizes16), "sixteen_empties": one_per_group(with_empties), "seventeen": seventeen,
            "thirty_three": thirty_three}


def adam_gradient(kind, n, step_index, rng):
    """float32 [n] gradient of one step (None: the parameter has no gradient).  Every element is 0 or at least 1e-15 in
    magnitude, so that no intermediate of the update is subnormal."""
    if kind == "none":
        return None
    sign = rng.choice([-1.0, 1.0], size=n)
    if kind == "zero" or (kind == "zero_later" and step_index >= 1):
        g = np.zeros(n)
    elif kind == "wide":
        g = sign * 10.0 ** rng.uniform(-12.0, 6.0, size=n)
    elif kind == "tiny":
        g = sign * 10.0 ** rng.uniform(-12.0, -9.0, size=n)
    elif kind == "huge":
        g = sign * 10.0 ** rng.uniform(4.0, 6.0, size=n)
    else:
        g = rng.standard_normal(n) * 10.0 ** ((step_index % 5) - 3)
        g = np.where(np.abs(g) < 1e-15, 1e-15, g)
    g = g.astype(F32)
    assert ((g == 0) | (np.abs(g) >= F32(1e-15))).all()
    return g


def adam_history(kind, n, start_step, rng):
    """(exp_avg, exp_avg_sq) float32 [n] of a state preset at ``start_step`` (zeros for a fresh state and for the
    all-zero-gradient parameter, which must then never move)."""
    if start_step == 0 or kind == "zero":
        return np.zeros(n, F32), np.zeros(n, F32)
    scale = {"tiny": 1e-10, "huge": 1e5}.get(kind, 1.0)
    m = (rng.standard_normal(n) * scale).astype(F32)
    v = ((0.1 + 0.9 * rng.random(n)) * scale * scale).astype(F32)
    return m, v


# ---- densification statistics ---------------------------------------------------------------------------------------------
DENSIFY_N = [1, 255, 256, 257, 1000]
DENSIFY_COLUMNS = [2, 3, 4]


def densify_inputs(n, columns, variant=0):
    """dict(vgrad [n,columns], radii [n] int32, accum [n,1], denom [n,1], max_r [n]): radii among 0, negatives, 1, ordinary
    values and 2^24 + 1; rows with radii <= 0 hold NaN and inf gradients and arbitrary bit patterns (NaN payloads among them)
    in the three accumulators, which the kernel must leave as they are."""
    rng = _rng("densify", n, columns, variant)
    radii = rng.choice(np.array([0, -1, -(2 ** 31), 1, 2, 29, 2 ** 24 + 1], np.int64), size=n).astype(np.int32)
    if n == 1:
        radii[0] = 1 if variant == 0 else 0
    else:
        radii[0], radii[-1] = 2 ** 24 + 1, 0
        radii[n // 2] = 1
    vis = radii > 0
    vgrad = (rng.standard_normal((n, columns)) * 10.0 ** rng.uniform(-6, 2, size=(n, 1))).astype(F32)
    accum = rng.random((n, 1)).astype(F32)
    denom = rng.integers(0, 5, size=(n, 1)).astype(F32)
    max_r = (rng.random(n) * 40).astype(F32)
    hostile = np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000, 0x7f800001, 0x00000001, 0x80000000,
                        0xdeadbeef, 0x7fffffff], np.uint32)
    k = int((~vis).sum())
    if k:
        vgrad[~vis] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1.0], F32), size=(k, columns))
        accum[~vis, 0] = rng.choice(hostile, size=k).view(F32)
        denom[~vis, 0] = rng.choice(hostile, size=k).view(F32)
        max_r[~vis] = rng.choice(hostile, size=k).view(F32)
    return dict(vgrad=vgrad, radii=radii, accum=accum, denom=denom, max_r=max_r)


# ---- kNN --------------------------------------------------------------------------------------------------------------------
LATTICE_H = 2.0 ** -3
KNN_BIG_N = 4_096_767                       # the smallest n at which the host picks KNN_MAX_GRID = 128 cells per axis
KNN_BIG_LO, KNN_BIG_EXT = -8.3, 18.6
KNN_CASES = ("n2", "n3", "n4", "n5", "lattice5", "lattice9", "lattice5_far", "lattice9_far", "line_x", "line_z", "plane",
             "identical", "two_groups", "long_box", "one_cell", "uniform5000", "uniform150000")


def knn_grid_target(n):
    """Cells along the longest axis, as knn_layout picks them (about two points per cell, 128 at most)."""
    t = 1
    while t < 128 and float(t) ** 3 < 0.5 * n:
        t += 1
    return t


def lattice(k, offset=(0.0, 0.0, 0.0)):
    g = np.arange(k, dtype=np.float64) * LATTICE_H
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(offset, np.float64)
    return p.astype(F32)


def knn_points(name):
    """float32 [n,3] of a kNN case."""
    rng = _rng("knn", name)
    far = (1024.0, -2048.0, 512.0)
    if name in ("n2", "n3", "n4", "n5"):
        p = rng.uniform(-1, 1, size=(int(name[1:]), 3))
    elif name.startswith("lattice"):
        p = lattice(int(name[7]), far if name.endswith("_far") else (0.0, 0.0, 0.0))
        p = p[rng.permutation(len(p))]
    elif name in ("line_x", "line_z"):
        p = np.zeros((3000, 3))
        p[:, 0 if name == "line_x" else 2] = rng.uniform(-2, 5, size=3000)
    elif name == "plane":
        p = np.concatenate([rng.uniform(-1, 1, size=(3000, 1)), np.full((3000, 1), 0.75), rng.uniform(-1, 1, size=(3000, 1))], 1)
    elif name == "identical":
        p = np.tile(np.array([[0.3, -1.7, 2.9]]), (300, 1))
    elif name == "two_groups":
        p = np.repeat(np.array([[0.3, -1.7, 2.9], [0.4, -1.5, 2.0]]), 32, axis=0)[rng.permutation(64)]
    elif name == "long_box":
        p = rng.random((20_000, 3)) * np.array([1000.0, 1.0, 0.001])
    elif name == "one_cell":
        p = np.concatenate([rng.uniform(-1e-3, 1e-3, size=(20_000, 3)), np.array([[1e6, 1e6, 1e6]])])
    elif name == "uniform5000":
        p = rng.uniform(-1, 1, size=(5000, 3))
    elif name == "uniform150000":
        p = rng.uniform(-1, 1, size=(150_000, 3))
    elif name == "big":
        p = rng.random((KNN_BIG_N, 3), dtype=np.float32) * F32(KNN_BIG_EXT) + F32(KNN_BIG_LO)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(p, F32)


def knn_big_queries(pts, sampled=2000, near_faces=2000):
    """Indices the 4 M-point case checks: ``sampled`` seeded points, and the points within 1e-4 of the extent from a face of
    the bounding box (``near_faces`` at most, spread over the six faces)."""
    rng = _rng("knn", "big", "queries")
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    margin = 1e-4 * (hi - lo)
    near = np.nonzero(((pts - lo <= margin) | (hi - pts <= margin)).any(axis=1))[0]
    if len(near) > near_faces:
        near = np.sort(rng.choice(near, size=near_faces, replace=False))
    return np.sort(rng.choice(len(pts), size=sampled, replace=False)), near

"""No GPU: are the block-cull fixtures (tests/block_cull_cases.py) testing the edges they claim to, and does the float64
restatement of the listing rule (tests/block_cull_reference.py) agree with the C oracle wherever it claims anything?

If a sweep has no listed and no unlisted Gaussian within a pixel of the deciding edge, or a control block is not so far
outside that the documented bound of blockcull.hip.h must cull it, the GPU test's pass would mean nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import block_cull_cases as cases
import block_cull_reference as ref


@pytest.mark.parametrize("name", cases.NAMES)
def test_reference_agrees_with_the_oracle_and_sweeps_sit_on_their_edges(oracle, name):
    case = cases.get(name)
    assert 3 <= len(case.views) <= 15                   # the shape at which a batch call runs the block test
    assert case.n <= 20000
    radii = cases.oracle_radii(case, oracle)
    listing = cases.reference_listing(case)
    if listing is None:
        return
    claimed = 0
    for v, (r, o) in enumerate(zip(listing, radii)):
        ok = ref.claims(r)
        claimed += int(ok.sum())
        bad = np.flatnonzero(ok & (r["listed"] != (o != 0)))
        assert bad.size == 0, (name, v, bad[:5], r["margin"][bad[:5]], r["radius"][bad[:5]], o[bad[:5]])
    assert claimed > 0.5 * case.n * len(case.views) or "huge" in name or "negdef" in name or "indef" in name or "near" in name, claimed
    r0 = listing[0]
    for label, blocks in case.exact.items():
        members = (blocks[:, None] * 64 + np.arange(64)[None]).ravel()
        members = members[members < case.n]
        raw = ref.outside_distance({k: a[members] for k, a in r0.items()}, case.views[0]) - r0["radius"][members]
        if "huge" in name or "negdef" in name:
            continue                                    # no radius in float64: the windows are aimed with radius 0
        near = np.abs(raw) < 1.0
        assert (near & r0["listed"][members]).any() and (near & ~r0["listed"][members]).any(), (name, label)


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n[:2] in ("c1", "c2", "c3")])
def test_control_blocks_must_be_culled_by_the_documented_bound(name):
    """Control blocks: one point, isotropic, rigid view, FOV <= 60 degrees, further outside the image than ten float64
    radii + 16 px in EVERY view -- and the bound the kernel documents stays below that distance, so a correct block test
    has to clear their bits."""
    case = cases.get(name)
    assert case.controls.size >= 2 and case.non_vacuous
    S, sig2 = case.cov3d(), case.sig2()
    for v in case.views:
        assert max(v.fovx, v.fovy) <= np.radians(60.0) + 1e-12
        assert np.allclose(v.M3 @ v.M3.T, np.eye(3), atol=1e-12)
        r = ref.listing(case.means, S, v)
        out = ref.outside_distance(r, v)
        for b in case.controls:
            m = slice(64 * b, min(64 * b + 64, case.n))
            assert np.ptp(case.means[m], axis=0).max() == 0.0                                  # one point
            ev = np.linalg.eigvalsh(S[m][0])
            assert ev.min() > 0 and ev.max() / ev.min() < 1.0 + 1e-5                          # isotropic
            assert (out[m] > 10.0 * r["radius"][m] + 16.0).all(), (name, b)
            rmax = ref.documented_rmax(sig2[m].max(), v, r["z"][m].min() * (1 - 1e-4))
            mx = 1.0 + 1e-4 * max(np.abs(r["pix_x"][m]).max(), np.abs(r["pix_y"][m]).max())
            assert rmax + mx < out[m].min(), (name, b, rmax, out[m].min())


def test_every_sweep_is_aimed_at_both_windows():
    """C1-C3: the second window is placed where the documented bound flips, so a sweep's blocks reach from further out
    than rmax to inside the exact edge (what the device must confirm with one set and one clear bit)."""
    for name in cases.NAMES:
        if name[:2] not in ("c1", "c3"):
            continue
        case = cases.get(name)
        r0 = ref.listing(case.means, case.cov3d(), case.views[0])
        out = ref.outside_distance(r0, case.views[0])
        sig2 = case.sig2()
        for label, blocks in case.sweeps.items():
            first = blocks * 64
            rmax = ref.documented_rmax(sig2[first], case.views[0], cases.Z0 - 1e-3)
            assert (out[first] > rmax + 1.2).any() and (out[first] < rmax).any(), (name, label)


def test_accessor_reports_the_call_shapes_that_cull():
    """pgr_workspace_block_visibility is host only (a made-up workspace pointer is never followed) and answers NULL exactly
    for PGR_BLOCK_CULL=0, one- and two-view calls and the split-views shape -- the forward call asks the same function."""
    from pegasus_amd import _lib
    lib = _lib.lib()
    fake, huge = C.c_void_p(0x10000), 1 << 60

    def culls(n, nv, w=48, h=32, cap=1 << 16):
        ptr, words = C.c_void_p(), C.c_int32(-1)
        rc = lib.pgr_workspace_block_visibility(fake, huge, n, w, h, cap, nv, C.byref(ptr), C.byref(words))
        assert rc == _lib.PGR_OK and words.value == (nv + 31) // 32
        if ptr.value is not None:
            off = ptr.value - fake.value
            assert 0 < off < lib.pgr_batch_workspace_bytes(n, w, h, cap, nv) and off % 16 == 0
        return ptr.value is not None

    old = os.environ.pop("PGR_BLOCK_CULL", None)
    try:
        assert [culls(5000, nv) for nv in (1, 2, 3, 15)] == [False, False, True, True]
        small_many = culls(5000, 70)
        n_min = smallest_culling_n(70)
        assert culls(n_min, 70) and (n_min == 1 or not culls(n_min - 1, 70))
        assert small_many == (n_min == 1)
        os.environ["PGR_BLOCK_CULL"] = "0"
        assert not culls(5000, 5) and not culls(n_min, 70)
    finally:
        os.environ.pop("PGR_BLOCK_CULL", None)
        if old is not None:
            os.environ["PGR_BLOCK_CULL"] = old
    bad = lib.pgr_workspace_block_visibility(fake, 16, 5000, 48, 32, 1 << 16, 5, C.byref(C.c_void_p()), C.byref(C.c_int32()))
    assert bad == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert lib.pgr_workspace_block_visibility(None, huge, 5000, 48, 32, 1 << 16, 5, C.byref(C.c_void_p()),
                                              C.byref(C.c_int32())) == _lib.PGR_ERR_INVALID_ARGUMENT


def smallest_culling_n(n_views, width=48, height=32, limit=1 << 24):
    """The smallest n at which a batch call of ``n_views`` views runs the block test, asked of the accessor (the threshold's
    value is the library's business; monotone in n).  Fails if there is none below ``limit``."""
    from pegasus_amd import _lib
    lib = _lib.lib()

    def culls(n):
        ptr, words = C.c_void_p(), C.c_int32()
        rc = lib.pgr_workspace_block_visibility(C.c_void_p(0x10000), 1 << 60, n, width, height, 1 << 16, n_views,
                                                C.byref(ptr), C.byref(words))
        assert rc == _lib.PGR_OK
        return ptr.value is not None
    assert culls(limit), f"no scene below {limit} Gaussians culls at {n_views} views"
    lo, hi = 0, limit                  # culls(hi), not culls(lo) (n = 0 never does)
    while hi - lo > 1:
        m = (lo + hi) // 2
        lo, hi = (lo, m) if culls(m) else (m, hi)
    return hi

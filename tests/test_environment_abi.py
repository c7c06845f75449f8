"""pgr_sdf_from_tsdf and the *_ground entries without a device: the symbols and struct layouts stand in the header, the library
and _lib alike; every misuse is PGR_ERR_INVALID_ARGUMENT from host-side checks before any launch (fake non-NULL device pointers
are never dereferenced); the existing entries' checks hold for the new ones."""
import ctypes as C
import re

import test_dynamics_abi as TA

FAKE, OTHER = C.c_void_p(0x1000), C.c_void_p(0x2000)
NAMES = ("pgr_sdf_from_tsdf_workspace_bytes", "pgr_sdf_from_tsdf", "pgr_rigid_contacts_ground", "pgr_rigid_simulate_ground")


def test_symbols_and_layouts_stand_in_the_header_the_library_and_the_binding():
    L = TA._lib()
    header = (TA.ROOT / "include" / "pegasus_raster.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in L.SYMBOLS and hasattr(L.lib(), name)
    assert L.lib().pgr_abi_version() == 4
    assert TA._header_struct(code, "PgrRigidGround") == [f[0] for f in L.PgrRigidGround._fields_]
    G = L.PgrRigidGround
    assert C.sizeof(G) == 48 and [getattr(G, f).offset for f, _ in G._fields_] == [0, 32, 40]
    # the ground entries take the existing entries' arguments behind the ground
    for old, new in (("pgr_rigid_contacts", "pgr_rigid_contacts_ground"), ("pgr_rigid_simulate", "pgr_rigid_simulate_ground")):
        a, b = L.SYMBOLS[old][1], L.SYMBOLS[new][1]
        assert b[0] is a[0] and b[2:] == a[1:] and b[1]._type_ is L.PgrRigidGround
    # what must not change
    assert C.sizeof(L.PgrRigidType) == 112 and C.sizeof(L.PgrRigidParams) == 72


def _field(L, grid=None, tsdf=FAKE, sdf=OTHER, dist2=None, ws=FAKE, ws_bytes=None, no_grid=False):
    g = TA._grid(L, **(grid or {}))
    if ws_bytes is None:
        ws_bytes = L.lib().pgr_sdf_from_tsdf_workspace_bytes(4, 5, 6)
    return L.lib().pgr_sdf_from_tsdf(None if no_grid else C.byref(g), tsdf, sdf, dist2, ws, ws_bytes, None)


def test_field_entry_rejects_misuse_before_any_launch():
    L = TA._lib()
    lib, bad = L.lib(), L.PGR_ERR_INVALID_ARGUMENT
    need = lib.pgr_sdf_from_tsdf_workspace_bytes(4, 5, 6)
    assert need >= 2 * 4 * 5 * 6 * 4
    for shape in ((1, 5, 6), (4, 0, 6), (4, 5, -1), (1025, 5, 6), (4, 1025, 6), (4, 5, 1025)):
        assert lib.pgr_sdf_from_tsdf_workspace_bytes(*shape) == 0, shape
    assert lib.pgr_sdf_from_tsdf_workspace_bytes(1024, 1024, 1024) >= 2 * 4 * 1024 ** 3
    assert _field(L, no_grid=True) == bad
    nan, inf = float("nan"), float("inf")
    for grid in (dict(nx=1), dict(ny=1025), dict(nz=0), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan), dict(voxel=inf)):
        assert _field(L, grid=grid, ws_bytes=1 << 40) == bad, grid
    for kw in (dict(tsdf=None), dict(sdf=None), dict(sdf=FAKE), dict(ws=None), dict(ws=C.c_void_p(0x1004)), dict(ws_bytes=need - 1),
               dict(ws_bytes=0)):
        assert _field(L, **kw) == bad, kw


def _ground(L, **kw):
    a = dict(sdf=FAKE, friction=0.5, grid={})
    a.update(kw)
    return L.PgrRigidGround(grid=TA._grid(L, **a["grid"]), sdf=a["sdf"], friction=a["friction"])


def _simulate(L, ground, **kw):
    a = dict(S=2, B=3, type_=FAKE, state=FAKE, n_steps=4, record_every=1, traj=FAKE, rest=FAKE, status=FAKE, ws=FAKE, ws_bytes=None,
             params=None, types=None)
    a.update(kw)
    types = [TA._type(L)] if a["types"] is None else a["types"]
    table = (L.PgrRigidType * len(types))(*types)
    p = TA._params(L) if a["params"] is None else a["params"]
    ws_bytes = L.lib().pgr_rigid_workspace_bytes(max(a["S"], 0), max(min(a["B"], 8), 0)) if a["ws_bytes"] is None else a["ws_bytes"]
    return L.lib().pgr_rigid_simulate_ground(C.byref(p), None if ground is None else C.byref(ground), len(types), table, a["S"],
                                             a["B"], a["type_"], a["state"], a["n_steps"], a["record_every"], a["traj"], a["rest"],
                                             a["status"], a["ws"], ws_bytes, None)


def _contacts(L, ground, **kw):
    a = dict(S=2, B=3, type_=FAKE, state=FAKE, words=FAKE, ws=FAKE, params=None)
    a.update(kw)
    table = (L.PgrRigidType * 1)(TA._type(L))
    p = TA._params(L) if a["params"] is None else a["params"]
    return L.lib().pgr_rigid_contacts_ground(C.byref(p), None if ground is None else C.byref(ground), 1, table, a["S"], a["B"],
                                             a["type_"], a["state"], a["words"], a["ws"],
                                             L.lib().pgr_rigid_workspace_bytes(max(a["S"], 0), max(min(a["B"], 8), 0)), None)


def test_ground_entries_reject_every_bad_ground_before_any_launch():
    L = TA._lib()
    bad = L.PGR_ERR_INVALID_ARGUMENT
    nan, inf = float("nan"), float("inf")
    for kw in (dict(sdf=None), dict(friction=-0.1), dict(friction=nan), dict(friction=inf), dict(grid=dict(nx=1)),
               dict(grid=dict(nz=1025)), dict(grid=dict(voxel=0.0)), dict(grid=dict(voxel=nan))):
        assert _simulate(L, _ground(L, **kw)) == bad, kw
        assert _contacts(L, _ground(L, **kw)) == bad, kw
    # a bad ground is refused even where there is nothing to do; a good one is then a no-op
    assert _simulate(L, _ground(L, sdf=None), S=0, type_=None, state=None, traj=None, rest=None, status=None, ws=None) == bad
    assert _simulate(L, _ground(L), S=0, type_=None, state=None, traj=None, rest=None, status=None, ws=None) == L.PGR_OK
    assert _contacts(L, _ground(L), B=0, type_=None, state=None, words=None, ws=None) == L.PGR_OK


def test_ground_entries_keep_the_existing_checks_with_and_without_a_ground():
    L = TA._lib()
    bad = L.PGR_ERR_INVALID_ARGUMENT
    for ground in (None, _ground(L)):
        for kw in (dict(type_=None), dict(state=None), dict(traj=None), dict(rest=None), dict(status=None), dict(ws=None),
                   dict(S=-1), dict(B=9), dict(n_steps=-1), dict(record_every=0), dict(ws=C.c_void_p(0x1004)),
                   dict(params=TA._params(L, plane=(0, 0, 2, 0))), dict(params=TA._params(L, plane=(0, 0, 1, float("nan")))),
                   dict(params=TA._params(L, h=0.0)), dict(types=[TA._type(L, mass=float("inf"))])):
            assert _simulate(L, ground, **kw) == bad, kw
        assert _simulate(L, ground, ws_bytes=16) == L.PGR_ERR_WORKSPACE_TOO_SMALL
        for kw in (dict(type_=None), dict(state=None), dict(words=None), dict(ws=None), dict(S=-1), dict(B=9),
                   dict(params=TA._params(L, margin=-1.0))):
            assert _contacts(L, ground, **kw) == bad, kw

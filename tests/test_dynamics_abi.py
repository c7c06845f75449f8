"""pgr_rigid_workspace_bytes, pgr_rigid_contacts, pgr_rigid_simulate without a device: the symbols, constants and struct layouts
stand in the header, the library and _lib alike; every misuse is PGR_ERR_INVALID_ARGUMENT from host-side checks before any launch
(fake non-NULL device pointers are never dereferenced); empty inputs answer PGR_OK."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("pgr_rigid_workspace_bytes", "pgr_rigid_contacts", "pgr_rigid_simulate")
FAKE = C.c_void_p(0x1000)


def _lib():
    from pegasus_amd import _lib as L
    return L


def _header_struct(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*", "", part.strip().split()[-1].lstrip("*")) for part in decl.split(",")]
    return fields


def test_symbols_constants_and_layouts_stand_in_the_header_the_library_and_the_binding():
    L = _lib()
    header = (ROOT / "include" / "pegasus_raster.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in L.SYMBOLS and hasattr(L.lib(), name)
    assert L.SYMBOLS["pgr_rigid_contacts"][1][-1] is C.c_void_p and L.SYMBOLS["pgr_rigid_simulate"][1][-1] is C.c_void_p
    assert L.lib().pgr_abi_version() == 4
    for macro, value in (("PGR_RIGID_MAX_BODIES", L.PGR_RIGID_MAX_BODIES), ("PGR_RIGID_MAX_TYPES", L.PGR_RIGID_MAX_TYPES),
                         ("PGR_RIGID_WORDS", L.PGR_RIGID_WORDS), ("PGR_RIGID_STATE", L.PGR_RIGID_STATE)):
        assert f"#define {macro} {value}\n" in header
    assert (L.PGR_RIGID_MAX_BODIES, L.PGR_RIGID_WORDS, L.PGR_RIGID_STATE) == (8, 7, 13)
    # the structs are the header's: the same fields in the same order, a 28-byte grid, then pointers at 8-byte alignment
    assert _header_struct(code, "PgrRigidType") == [f[0] for f in L.PgrRigidType._fields_]
    assert _header_struct(code, "PgrRigidParams") == [f[0] for f in L.PgrRigidParams._fields_]
    T, P = L.PgrRigidType, L.PgrRigidParams
    assert C.sizeof(T) == 112 and [getattr(T, f).offset for f, _ in T._fields_] == [0, 32, 40, 48, 52, 56, 68, 104, 108]
    assert C.sizeof(P) == 72 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 16, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68]


def _grid(L, **kw):
    a = dict(nx=4, ny=5, nz=6, voxel=0.1)
    a.update(kw)
    return L.PgrGrid(nx=a["nx"], ny=a["ny"], nz=a["nz"], origin=(C.c_float * 3)(0, 0, 0), voxel=a["voxel"])


def _type(L, **kw):
    a = dict(sdf=FAKE, shell=FAKE, n_shell=10, mass=1.0, friction=0.5, radius=0.9, com=(0, 0, 0), grid={},
             inv_inertia=(6, 0, 0, 0, 6, 0, 0, 0, 6))
    a.update(kw)
    return L.PgrRigidType(grid=_grid(L, **a["grid"]), sdf=a["sdf"], shell=a["shell"], n_shell=a["n_shell"], mass=a["mass"],
                          com=(C.c_float * 3)(*a["com"]), inv_inertia=(C.c_float * 9)(*a["inv_inertia"]), friction=a["friction"],
                          radius=a["radius"])


def _params(L, **kw):
    a = dict(h=1e-3, gravity=(0, 0, -50), plane=(0, 0, 1, 0), plane_friction=0.5, lin_damp=0.04, ang_damp=0.04, iterations=10,
             beta=0.2, slop=2e-4, margin=1e-3, v_sleep=0.02, w_sleep=0.4, sleep_steps=50)
    a.update(kw)
    a["gravity"], a["plane"] = (C.c_float * 3)(*a["gravity"]), (C.c_float * 4)(*a["plane"])
    return L.PgrRigidParams(**a)


def _simulate(L, params=None, types=None, S=2, B=3, n_types=None, type_=FAKE, state=FAKE, n_steps=4, record_every=1, traj=FAKE,
              rest=FAKE, status=FAKE, ws=FAKE, ws_bytes=None, no_params=False, no_table=False):
    types = [_type(L)] if types is None else types
    table = (L.PgrRigidType * max(1, len(types)))(*types)
    p = _params(L) if params is None else params
    if ws_bytes is None:
        ws_bytes = L.lib().pgr_rigid_workspace_bytes(max(S, 0), max(min(B, 8), 0))
    return L.lib().pgr_rigid_simulate(None if no_params else C.byref(p), len(types) if n_types is None else n_types,
                                      None if no_table else table, S, B, type_, state, n_steps, record_every, traj, rest, status, ws,
                                      ws_bytes, None)


def _contacts(L, params=None, types=None, S=2, B=3, type_=FAKE, state=FAKE, words=FAKE, ws=FAKE):
    types = [_type(L)] if types is None else types
    table = (L.PgrRigidType * max(1, len(types)))(*types)
    p = _params(L) if params is None else params
    return L.lib().pgr_rigid_contacts(C.byref(p), len(types), table, S, B, type_, state, words, ws,
                                      L.lib().pgr_rigid_workspace_bytes(max(S, 0), max(min(B, 8), 0)), None)


def test_workspace_bytes_refuses_bad_sizes():
    lib = _lib().lib()
    assert lib.pgr_rigid_workspace_bytes(-1, 3) == 0 and lib.pgr_rigid_workspace_bytes(4, 9) == 0
    assert lib.pgr_rigid_workspace_bytes(4, -1) == 0 and lib.pgr_rigid_workspace_bytes((1 << 20) + 1, 1) == 0
    small, big = lib.pgr_rigid_workspace_bytes(1, 1), lib.pgr_rigid_workspace_bytes(64, 8)
    assert 0 < small < big and big >= 64 * 64 * 7 * (8 + 56 * 4)                 # the words and the rows of every pair


def test_simulate_rejects_misuse_before_any_launch():
    L = _lib()
    bad = L.PGR_ERR_INVALID_ARGUMENT
    assert _simulate(L, no_params=True) == bad and _simulate(L, no_table=True) == bad
    for kw in (dict(type_=None), dict(state=None), dict(traj=None), dict(rest=None), dict(status=None), dict(ws=None),
               dict(S=-1), dict(B=-1), dict(B=9), dict(S=(1 << 20) + 1), dict(n_types=0), dict(n_types=-1), dict(n_types=17),
               dict(n_steps=-1), dict(record_every=0), dict(ws=C.c_void_p(0x1004))):
        assert _simulate(L, **kw) == bad, kw
    assert _simulate(L, ws_bytes=16) == L.PGR_ERR_WORKSPACE_TOO_SMALL
    nan, inf = float("nan"), float("inf")
    for kw in (dict(h=0.0), dict(h=-1e-3), dict(h=nan), dict(h=inf), dict(iterations=0), dict(iterations=-2),
               dict(gravity=(0, nan, -50)), dict(plane=(0, 0, 2, 0)), dict(plane=(0, 0, 0, 0)), dict(plane=(0, 0, 1, nan)),
               dict(plane_friction=-0.1), dict(lin_damp=1.0), dict(ang_damp=-0.1), dict(beta=nan), dict(slop=-1e-4),
               dict(margin=inf), dict(v_sleep=-1.0), dict(w_sleep=nan)):
        assert _simulate(L, params=_params(L, **kw)) == bad, kw
    for kw in (dict(mass=0.0), dict(mass=-1.0), dict(mass=nan), dict(mass=inf), dict(friction=-0.5), dict(friction=nan),
               dict(radius=-1.0), dict(radius=inf), dict(com=(0, nan, 0)), dict(inv_inertia=(6, 0, 0, 0, inf, 0, 0, 0, 6)),
               dict(n_shell=-1), dict(shell=None), dict(sdf=None), dict(grid=dict(ny=1)), dict(grid=dict(voxel=0.0))):
        assert _simulate(L, types=[_type(L), _type(L, **kw)]) == bad, kw
        assert _contacts(L, types=[_type(L), _type(L, **kw)]) == bad, kw


def test_contacts_rejects_misuse_before_any_launch():
    L = _lib()
    bad = L.PGR_ERR_INVALID_ARGUMENT
    for kw in (dict(type_=None), dict(state=None), dict(words=None), dict(ws=None), dict(S=-1), dict(B=9)):
        assert _contacts(L, **kw) == bad, kw
    assert _contacts(L, params=_params(L, plane=(0, 1, 1, 0))) == bad and _contacts(L, params=_params(L, margin=-1.0)) == bad


def test_empty_inputs_are_no_ops():
    L = _lib()
    ok = L.PGR_OK
    assert _simulate(L, S=0, type_=None, state=None, traj=None, rest=None, status=None, ws=None) == ok
    assert _simulate(L, B=0, type_=None, state=None, traj=None, rest=None, status=None, ws=None) == ok
    assert _contacts(L, S=0, type_=None, state=None, words=None, ws=None) == ok
    assert _contacts(L, B=0, type_=None, state=None, words=None, ws=None) == ok
    # a single slot never is a target: its type needs no field
    assert _simulate(L, S=0, B=1, types=[_type(L, sdf=None)], type_=None, state=None, traj=None, rest=None, status=None, ws=None) == ok


def test_wrappers_take_their_arguments_apart_on_the_host():
    from pegasus_amd import dynamics as DYN
    assert DYN.Params().struct([]).margin == 0.0 and abs(DYN.Params(margin=0.25).struct([]).margin - 0.25) < 1e-7
    assert tuple(DYN.Params().struct([]).gravity) == (0.0, 0.0, -50.0) and abs(DYN.Params().struct([]).h - 1e-3) < 1e-9
    with pytest.raises(ValueError):
        DYN.Params(plane=(0, 0, 0, 0)).struct([])
    with pytest.raises(ValueError):
        DYN._table([])

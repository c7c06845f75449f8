#!/usr/bin/env python3
"""Machine code of every gfx950 kernel of two builds of libpegasus_raster.so, compared by symbol name: what a refactor that
must not change a kernel is checked with (profiles/r08_source_split.txt).  No GPU needed.
    python scripts/compare_kernel_code.py OLD.so NEW.so
Reads the code objects out of .hip_fatbin (one uncompressed offload bundle per translation unit) and compares, per function
symbol, the bytes of its code and, per kernel, its descriptor (NAME.kd) without the layout-dependent offset to the code.
A difference is printed with the dwords that differ."""
import struct
import sys
from pathlib import Path

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def elf_sections(b):
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = []
    for i in range(shnum):
        name, typ, _, addr, off, size, link, _, _, _ = struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize)
        secs.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link))
    names = secs[shstrndx]["off"]
    for s in secs:
        s["name"] = b[names + s["name"]:b.index(b"\0", names + s["name"])].decode()
    return secs


def code_objects(lib):
    b = Path(lib).read_bytes()
    fat = next(s for s in elf_sections(b) if s["name"] == ".hip_fatbin")
    blob = b[fat["off"]:fat["off"] + fat["size"]]
    out, at = [], blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + 24)
        p = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            if b"gfx950" in blob[p + 24:p + 24 + tl]:
                out.append(blob[at + off:at + off + size])
            p += 24 + tl
        at = blob.find(MAGIC, at + 24)
    assert out, f"{lib}: no uncompressed gfx950 code object"
    return out


def kernels(lib):
    found = {}
    for co in code_objects(lib):
        secs = elf_sections(co)
        symtab = next(s for s in secs if s["name"] == ".symtab")
        strs = secs[symtab["link"]]["off"]
        for i in range(symtab["size"] // 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", co, symtab["off"] + 24 * i)
            if shndx == 0 or shndx >= len(secs):
                continue
            nm = co[strs + name:co.index(b"\0", strs + name)].decode()
            at = secs[shndx]["off"] + value - secs[shndx]["addr"]
            if info & 0xF == 2:                                  # STT_FUNC: the code
                found.setdefault(nm, []).append(co[at:at + size])
            elif nm.endswith(".kd"):                             # the kernel descriptor; bytes 16..23: offset to the code
                found.setdefault(nm, []).append(co[at:at + 16] + co[at + 24:at + 64])
    return found


def main(old_lib, new_lib):
    old, new = kernels(old_lib), kernels(new_lib)
    names = sorted(set(old) | set(new))
    bad = 0
    for nm in names:
        a, b = old.get(nm), new.get(nm)
        if a is None or b is None:
            why = "only in the " + ("new" if a is None else "old") + " library"
        elif len(a) != 1 or len(b) != 1:
            why = f"defined {len(a)} times in the old library, {len(b)} times in the new"
        elif a[0] != b[0]:
            why = f"differs ({len(a[0])} and {len(b[0])} bytes)"
        else:
            continue
        bad += 1
        print(f"{nm}: {why}")
        if a and b and len(a[0]) == len(b[0]):
            for i in range(0, len(a[0]) - 3, 4):
                if a[0][i:i + 4] != b[0][i:i + 4]:
                    print(f"    +{i:#07x}  after {a[0][max(i - 8, 0):i].hex()}:  {struct.unpack_from('<i', a[0], i)[0]} -> "
                          f"{struct.unpack_from('<i', b[0], i)[0]}")
    n_kd = sum(n.endswith(".kd") for n in names)
    print(f"{len(names) - n_kd} function symbols and {n_kd} kernel descriptors compared by name: {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))

"""The size functions of the C ABI under AddressSanitizer + UndefinedBehaviorSanitizer, without a device and without Python in
the sanitised process: writes a C++ program that calls every size function over the grid of tests/test_abi_layouts.py, builds
it together with the library's host code (-Xarch_host -fsanitize=address,undefined), runs it and holds what it prints against
tests/golden/abi_sizes.json.

    python scripts/abi_sizes_sanitized.py [build directory]
"""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import test_abi_layouts as T            # noqa: E402
from pegasus_amd import build           # noqa: E402


def program() -> str:
    lines = ['#include <cstdio>', '#include "pegasus_raster.h"', "int main() {"]
    for name, arg_list in T.cases().items():
        for args in arg_list:
            if name in T.JOB_FIELD:
                struct, fld = T.JOB_FIELD[name]
                sets = " ".join(f"j[{k}].{fld} = {c};" for k, c in enumerate(args))
                lines.append(f'    {{ {struct} j[{len(args)}] = {{}}; {sets} std::printf("%zu\\n", {name}({len(args)}, j)); }}')
            elif name == "pgr_frame_record_layout":
                lines.append(f'    {{ PgrRecordLayout r; {name}({", ".join(map(str, args))}, &r); std::printf("%lld %lld %lld %lld\\n", '
                             "(long long)r.off_rgb, (long long)r.off_depth, (long long)r.off_masks, (long long)r.bytes); }")
            else:
                lines.append(f'    std::printf("%zu\\n", {name}({", ".join(f"{a}LL" for a in args)}));')
    return "\n".join(lines + ["    return 0;", "}", ""])


def main(out_dir) -> int:
    out_dir = Path(out_dir)
    (out_dir / "abi_sizes_main.cpp").write_text(program())
    srcs, _ = build.sources()
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC", "-O3")]
    subprocess.run(["hipcc", *flags, "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    f"-I{ROOT / 'include'}", str(out_dir / "abi_sizes_main.cpp"), *map(str, srcs), "-o",
                    str(out_dir / "abi_sizes_san")], check=True, cwd=str(build.CSRC))
    run = subprocess.run([str(out_dir / "abi_sizes_san")], capture_output=True, text=True, timeout=600)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0 and "Sanitizer" not in report and "runtime error" not in report, report
    got, golden = iter(run.stdout.splitlines()), json.loads(T.GOLDEN.read_text())
    for name, arg_list in T.cases().items():
        rows = [[int(v) for v in next(got).split()] for _ in arg_list]
        if name in T.SHRUNK:                         # recorded before the dead per-view slots went (see the test)
            continue
        assert [r if len(r) > 1 else r[0] for r in rows] == golden[name], name
    print("sanitised size functions: clean, and equal to", T.GOLDEN.relative_to(ROOT))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1:
        raise SystemExit(main(sys.argv[1]))
    with tempfile.TemporaryDirectory() as tmp:
        raise SystemExit(main(tmp))

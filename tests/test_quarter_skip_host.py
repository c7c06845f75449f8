"""The compositor's own skip test (quarter_may_contribute, csrc/cull.hip.h) as HOST code, in a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/quarter_skip_sweep.cpp sweeps it over (splat, box) cases -- isotropic
splats, 1000:1 splats at 0 / 45 / 135 degrees, op in {0, denormal, 1/255 (1 +- 1e-3), 0.5, 0.99, 1, 1e30}, centres inside,
on an edge and 1 / 8 / 1e6 pixels outside, boxes 1x1 .. 8x8 including the clipped last column and row, conics with A <= 0,
C <= 0, A C < B^2, NaN and +-Inf in every field, and 400 000 random splats placed around the threshold -- and checks every
`false` against a float64 evaluation at every pixel centre of the box: power > 0 or op exp(power) < (1/255)(1 - 1e-5).
The function may be looser or tighter than the binning predicate; how often each keeps what the other rejects is printed,
not asserted."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from pegasus_amd import build  # noqa: E402


def test_quarter_skip_is_conservative_on_the_sweep(tmp_path):
    exe = tmp_path / "quarter_skip_sweep"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC", "-O3")]
    subprocess.run(["hipcc", *flags, "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    f"-I{build.CSRC}", str(ROOT / "tests" / "quarter_skip_sweep.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    report = run.stdout[-3000:] + run.stderr[-4000:]
    print(report)
    assert run.returncode == 0 and "Sanitizer" not in report and "runtime error" not in report, report
    m = re.search(r"cases (\d+) skipped (\d+) wrong (\d+) new_keeps_old_rejects (\d+) old_keeps_new_rejects (\d+)", run.stdout)
    assert m, report
    cases, skipped, wrong = (int(m.group(i)) for i in (1, 2, 3))
    assert cases >= 200_000
    assert wrong == 0, report
    assert 0 < skipped < cases          # the sweep reaches both verdicts

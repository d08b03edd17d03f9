"""The CPU twin of the cross-based cost aggregation under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/mccbca_host_main.cpp): a stand-alone program built with the host
compiler's sanitizers, run as a child process; the test preloads nothing.  It runs the arms and the
aggregation on odd shapes (one pixel, one row, one column, l1 = 32 on a 3 x 5 image, strided rows,
a batch, offsets at the ends of int) in exact-size heap blocks."""
import os
import subprocess
import sys

import pytest

from test_pngdec_sanitize import CSRC, ROOT, compilers

MAIN = os.path.join(ROOT, "tools", "mccbca_host_main.cpp")


def test_twin_under_asan_and_ubsan(tmp_path):
    ok, why = compilers(str(tmp_path))
    if not ok:
        print("\n".join(why))
        pytest.skip("neither compiler links the sanitizer runtime: " + " | ".join(why))
    name, cmd = ok[0]
    exe = str(tmp_path / "mccbca_host")
    r = subprocess.run(cmd + ["-I" + CSRC, "-o", exe, MAIN], capture_output=True, text=True)
    assert r.returncode == 0, f"{name} links the sanitizer runtime but does not build {MAIN}:\n" + r.stderr[-4000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0"
    r = subprocess.run([exe, "7"], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "cases ok 10" in r.stdout

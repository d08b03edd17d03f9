"""The bf16 twin of the accurate MC-CNN scorer and ac_bf16 under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/mcacc16_host_main.cpp): a stand-alone program built with the host
compiler's sanitizers, run as a child process; the test preloads nothing.  It runs the bf16 join on
odd shapes (one pixel, one row, one column, batches, 1 to 4 hidden layers, both roles, more planes
than columns, offsets at the ends of int) in exact-size heap blocks, the weight packing of the
device path, and the rounding on its special values."""
import os
import subprocess
import sys

import pytest

from test_pngdec_sanitize import CSRC, ROOT, compilers

MAIN = os.path.join(ROOT, "tools", "mcacc16_host_main.cpp")


def test_bf16_twin_under_asan_and_ubsan(tmp_path):
    ok, why = compilers(str(tmp_path))
    if not ok:
        print("\n".join(why))
        pytest.skip("neither compiler links the sanitizer runtime: " + " | ".join(why))
    name, cmd = ok[0]
    exe = str(tmp_path / "mcacc16_host")
    r = subprocess.run(cmd + ["-I" + CSRC, "-o", exe, MAIN], capture_output=True, text=True)
    assert r.returncode == 0, f"{name} links the sanitizer runtime but does not build {MAIN}:\n" + r.stderr[-4000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0"
    r = subprocess.run([exe, "7"], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "cases ok 8" in r.stdout and "bf16(7f7f8000) = 7f80" in r.stdout

"""The JPEG decoder's CPU twin under AddressSanitizer and UndefinedBehaviorSanitizer
(tools/jpegdec_fuzz_main.cpp): a stand-alone program built with the host compiler's sanitizers, run
as a child process; the test preloads nothing.  It replays truncations at every length and 2000
single-byte mutations of five small files: gray, 4:2:0, 4:2:0 with restart markers, optimised
tables (Pillow's, from the fixtures) and a 16-bit quantiser.  This is the only place mutated files
are swept."""
import os
import subprocess
import sys

import pytest

import jpeg_cases as C
from test_pngdec_sanitize import CSRC, ROOT, compilers

MAIN = os.path.join(ROOT, "tools", "jpegdec_fuzz_main.cpp")


def build(tmp):
    ok, why = compilers(tmp)
    if not ok:
        return None, why
    name, cmd = ok[0]
    exe = os.path.join(tmp, "jpegdec_fuzz")
    r = subprocess.run(cmd + ["-I" + CSRC, "-o", exe, MAIN], capture_output=True, text=True)
    assert r.returncode == 0, f"{name} links the sanitizer runtime but does not build {MAIN}:\n" + r.stderr[-4000:]
    return exe, why


def test_decoder_twin_under_asan_and_ubsan(tmp_path):
    exe, why = build(str(tmp_path))
    if exe is None:
        print("\n".join(why))
        pytest.skip("neither compiler links the sanitizer runtime: " + " | ".join(why))
    cases = {"gray.jpg": C.grid_file(None, 17, 9), "c420.jpg": C.grid_file((2, 2), 17, 9),
             "c420_rst.jpg": C.grid_file((2, 2), 33, 17, ri=1), "optimised.jpg": C.pillow_fixtures()["c420_q95_opt"][0],
             "dqt16.jpg": C.handmade()["dqt16"], "wild.jpg": C.handmade()["wild"]}
    files = []
    for name, data in cases.items():
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(data)
        files.append(path)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0"
    r = subprocess.run([exe, "2024"] + files, capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count("mutations rejected") == len(files)

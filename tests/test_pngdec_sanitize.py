"""The PNG decoder's CPU twin under AddressSanitizer and UndefinedBehaviorSanitizer
(tools/pngdec_fuzz_main.cpp): a stand-alone program built with the host compiler's sanitizers, run
as a child process; the test preloads nothing.  It replays truncations at every length and 2000
single-byte mutations (CRCs recomputed) of small files: our own (chunk-parallel path) and foreign
ones written here with zlib (serial path)."""
import os
import shutil
import subprocess
import sys
import zlib

import pytest

import png_np
import pngdec_np as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_match_amd", "csrc")
MAIN = os.path.join(ROOT, "tools", "pngdec_fuzz_main.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


PROBE = "int main() { return 0; }\n"


def compilers(tmp):
    """The command prefixes that can link the sanitizer runtime here (a trivial program built
    with the same sanitizer flags), and why the others cannot."""
    ok, why = [], []
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write(PROBE)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    cands = []
    if os.path.exists(hipcc):
        cands.append(("hipcc", [hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950"]
                      + [x for f in SAN for x in ("-Xarch_host", f)]))
    else:
        why.append("no hipcc")
    gxx = shutil.which("g++")
    if gxx and os.path.isdir(hip_inc):
        cands.append(("g++", [gxx, "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-D__host__=", "-D__device__=",
                              "-I" + hip_inc] + SAN))
    else:
        why.append("no g++ with the HIP headers")
    for name, cmd in cands:
        r = subprocess.run(cmd + ["-o", os.path.join(tmp, "probe_" + name), probe], capture_output=True, text=True)
        if r.returncode == 0:
            ok.append((name, cmd))
        else:
            why.append(f"{name} cannot link the sanitizer runtime: " + r.stderr.strip()[-300:])
    return ok, why


def build(tmp):
    """The program, built by the first compiler that links the sanitizer runtime; (None, reasons)
    only when none does.  A compiler that passed the probe must build the program."""
    ok, why = compilers(tmp)
    if not ok:
        return None, why
    name, cmd = ok[0]
    exe = os.path.join(tmp, "pngdec_fuzz")
    r = subprocess.run(cmd + ["-I" + CSRC, "-o", exe, MAIN], capture_output=True, text=True)
    assert r.returncode == 0, f"{name} links the sanitizer runtime but does not build {MAIN}:\n" + r.stderr[-4000:]
    return exe, why


def test_decoder_twin_under_asan_and_ubsan(tmp_path):
    exe, why = build(str(tmp_path))
    if exe is None:
        print("\n".join(why))
        pytest.skip("neither compiler links the sanitizer runtime: " + " | ".join(why))
    files = []
    gray = png_np.runny(3, (17, 29))
    rgb = png_np.runny(4, (9, 11, 3))
    cases = {"level6.png": P.write_png(gray, level=6), "split1.png": P.write_png(rgb, level=9, idat_split=1),
             "stored.png": P.write_png(gray, level=0), "fixed.png": P.write_png(rgb, strategy=zlib.Z_FIXED, idat_split=40),
             "sync.png": P.write_png(gray, filters=0, pieces=[100, 5], flush=zlib.Z_SYNC_FLUSH)}
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
    assert r.stdout.count("mutations rejected") == 4 + len(files)

"""Device time of the PNG decoder: HIP events on one stream around
sm_png_decode_batch_device (files already in device memory), 5 warm-up launches + 30 timed, the
median reported; the wall time of file in host memory -> pixels on the device (imdecode with
as_tensor=True: staging, upload, decode, status read-back) likewise.
    python tools/pngdec_bench.py [--out profiles/pngdec/pngdec_bench.jsonl]
Workloads: this package's own files of a 1280x720 BGR frame, a 1280x720 gray frame and a 1242x375
KITTI 16-bit map (chunk-parallel inflate), 16 BGR frames in one call, and the same BGR pixels as a
foreign file (the same filtered stream through zlib level 6, IDAT chunks of 8192 bytes as libpng
writes them: serial inflate), single and x 16.  The images are png_bench.py's.
Per-kernel times come from a kernel trace of one step of this tool (--one), kept beside the
output.  On the same machine's CPU in the same run, one thread:
  zlib_ms     zlib.decompress of the joined IDAT data alone (no unfilter)
  pillow_ms   Pillow's full decode of the same file (inflate + unfilter), where it imports
A numpy unfilter is not timed: Average and Paeth rows are per-byte recurrences, which numpy runs
in the interpreter (seconds per frame), so the figure would say nothing about a CPU decoder.
Every GPU step is a child process of its own under a time limit; the first one that fails ends
the run.  One JSON object per line."""
import argparse
import io
import json
import os
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = ("bgr_720p", "gray_720p", "kitti_map", "bgr_720p_x16", "bgr_720p_level6", "bgr_720p_level6_x16")
WARMUP, TIMED = 5, 30
STEP_TIMEOUT_S = 240


def chunks_of(png: bytes):
    pos, out = 8, []
    while pos < len(png):
        n = int.from_bytes(png[pos:pos + 4], "big")
        out.append((png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def as_level6(png: bytes) -> bytes:
    """The same pixels as a foreign file: the filtered stream through zlib level 6, IDAT chunks of
    8192 bytes."""
    ch = chunks_of(png)
    z = zlib.compress(zlib.decompress(b"".join(d for t, d in ch if t == b"IDAT")), 6)

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))

    return (png[:8] + chunk(b"IHDR", ch[0][1]) + b"".join(chunk(b"IDAT", z[i:i + 8192]) for i in range(0, len(z), 8192))
            + chunk(b"IEND", b""))


def cpu_times(png: bytes):
    out = {}

    def best(fn, reps=3):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(min(ts), 2)

    z = b"".join(d for t, d in chunks_of(png) if t == b"IDAT")
    out["zlib_ms"] = best(lambda: zlib.decompress(z))
    try:
        from PIL import Image
    except Exception:
        return out

    def pil():
        im = Image.open(io.BytesIO(png))
        im.load()

    out["pillow_ms"] = best(pil)
    return out


def one(name):
    """One GPU step: prints its JSON line."""
    import torch

    import png_bench
    import stereo_match_amd as sma
    from stereo_match_amd import _lib, png

    dev = torch.device("cuda", 0)
    nimg = 16 if name.endswith("_x16") else 1
    if name.startswith("bgr"):
        imgs = [png_bench.frame(k) for k in range(nimg)]
        files = [sma.imencode_png_host(im) for im in imgs]
        if "level6" in name:
            files = [as_level6(f) for f in files]
        flags, want = 1, imgs
    elif name.startswith("gray"):
        imgs = [png_bench.frame()[:, :, 1].copy()]
        files, flags, want = [sma.imencode_png_host(imgs[0])], 0, imgs
    else:
        d = png_bench.kitti_map()
        files, flags = [sma.encode_disparity_png(d, "kitti", host=True)], -1
        want = [np.where(d < 0, 0, d.astype(np.int32) << 4).astype(np.uint16)]
    info = _lib.png_info(files[0])
    H, W = info[:2]
    prm, shape, dt = png._dec_params(info, flags)
    prm.max_chunks = max(len(f) for f in files) // 12 + 1
    prm.max_file_bytes = max(len(f) for f in files)
    eng = _lib.engine(0)
    st = torch.cuda.Stream(device=dev)

    def timed(fn):
        ts = []
        for it in range(WARMUP + TIMED):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ts.append(a.elapsed_time(b) * 1e3)
        return round(float(np.median(ts)), 1), round(float(np.min(ts)), 1)

    with torch.cuda.stream(st):
        eng.set_stream(st.cuda_stream)
        sizes = np.array([len(f) for f in files], np.int64)
        offs = np.concatenate([[0], np.cumsum((sizes + 15) & ~15)[:-1]]).astype(np.int64)
        blob = np.zeros(int(offs[-1] + sizes[-1]), np.uint8)
        for f, o in zip(files, offs):
            blob[o:o + len(f)] = np.frombuffer(f, np.uint8)
        d_blob = torch.from_numpy(blob).to(dev)
        d_tab = torch.from_numpy(np.stack([offs, sizes])).to(dev)
        out = torch.empty((nimg,) + shape, dtype=png._torch_dtype(dt), device=dev)
        status = torch.empty(nimg, dtype=torch.int32, device=dev)

        def dec():
            eng.png_decode_batch_device(d_blob.data_ptr(), d_tab[0].data_ptr(), d_tab[1].data_ptr(), nimg, H, W, prm,
                                        out.data_ptr(), out.stride(0) * out.element_size(),
                                        out.stride(1) * out.element_size(), status.data_ptr())

        full = timed(dec)
        dec()
        ok = status.cpu().tolist() == [0] * nimg
        paths = eng.png_decode_stats()
        got = out.cpu().numpy()
        equal = ok and all(np.array_equal(got[i], want[i]) for i in range(nimg))
        walls = []
        for _ in range(10):
            st.synchronize()
            t0 = time.perf_counter()
            t = sma.imdecode_batch(files, flags) if nimg > 1 else sma.imdecode(files[0], flags, as_tensor=True)
            st.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        del t
    eng.set_stream(None)
    res = dict(what="pngdec", workload=name, H=int(H), W=int(W), images=nimg, file_bytes=len(files[0]),
               idat_chunks=sum(1 for t, _ in chunks_of(files[0]) if t == b"IDAT"), parallel=paths[0], serial=paths[1],
               device_us=full[0], device_us_min=full[1], device_us_per_image=round(full[0] / nimg, 1),
               wall_host_file_to_tensor_ms=round(float(np.median(walls)), 3), pixels_equal=bool(equal))
    res.update(cpu_times(files[0]))
    if "pillow_ms" in res:
        res["pillow_all_images_over_device"] = round(res["pillow_ms"] * nimg * 1e3 / full[0], 2)
    res["zlib_all_images_over_device"] = round(res["zlib_ms"] * nimg * 1e3 / full[0], 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--one", metavar="WORKLOAD", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(args.one)
        return
    lines = []
    for name in WORKLOADS:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
        if r.returncode != 0:
            sys.exit(f"pngdec_bench: the step {name} ended with status {r.returncode}; stopping")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln)
                print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

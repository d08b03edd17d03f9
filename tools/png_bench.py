"""Device time of the PNG encoder: HIP events on one stream around
sm_png_encode_batch_device, 5 warm-up launches + 30 timed, the median reported; the wall time of
device image -> file in pinned host memory (encode + size read-back + copy + sync) likewise.
    python tools/png_bench.py [--out profiles/png/png_bench.jsonl]
Workloads: a 1280x720 BGR frame, a 1280x720 gray frame, a 1242x375 int16 disparity map as the
KITTI 16-bit file, and a batch of 16 BGR frames in one call.  The images are synthetic: a
random-dot frame under a smooth ramp (the frame), the matcher's kind of map with one pixel in ten
invalid (the map).
  device_us       all launches (filter, deflate, assemble, scatter)
  sizes_only_us   the same without the scatter of the chunks to their places (d_out NULL)
  fixed_none_us   with filter 0 instead of the adaptive choice (one pass over the rows less)
Per-kernel times come from a kernel trace of one step of this tool (--one), kept beside the
output.  On the same machine's CPU in the same run, where they import:
  pillow_ms       Image.save(..., "PNG") of the same pixels (zlib level 6 inside)
  zlib6_ms        zlib.compress(stream, 6) of the same filtered stream
  zlib_rle_ms     level 1 with Z_RLE (runs at distance 1 only, the closest to this coder)
zlib and Pillow compress on one thread; the job's 16 CPUs do not change them.
Every GPU step is a child process of its own under a time limit; the first one that fails ends
the run.  One JSON object per line."""
import argparse
import io
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("bgr_720p", "gray_720p", "kitti_map", "bgr_720p_x16")
WARMUP, TIMED = 5, 30
STEP_TIMEOUT_S = 240


def frame(seed=0):
    from stereo_match_amd import synthetic

    left, right, _ = synthetic.random_dot_pair(720, 1280, 64, seed=seed)
    yy, xx = np.mgrid[0:720, 0:1280]
    ramp = ((xx + 2 * yy) // 8 % 256).astype(np.uint8)
    return np.stack([left // 2 + ramp // 2, ramp, right // 2 + ramp // 2], -1).astype(np.uint8)


def kitti_map(seed=0):
    rng = np.random.default_rng(seed)
    H, W = 375, 1242
    base = np.linspace(40, 900, W)[None, :] + np.linspace(0, 300, H)[:, None]
    d = (base + rng.integers(-3, 4, (H, W))).astype(np.int16)
    d[rng.random((H, W)) < 0.1] = -16
    return d


def stream_of(png: bytes) -> bytes:
    """The filtered stream inside one of our files."""
    pos, idat = 8, []
    while pos < len(png):
        n = int.from_bytes(png[pos:pos + 4], "big")
        if png[pos + 4:pos + 8] == b"IDAT":
            idat.append(png[pos + 8:pos + 8 + n])
        pos += 12 + n
    return zlib.decompress(b"".join(idat))


def cpu_times(pixels, stream):
    out = {}

    def best(fn, reps=3):
        ts, r = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(min(ts), 2), r

    def rle():
        c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        return c.compress(stream) + c.flush()

    out["zlib6_ms"], z6 = best(lambda: zlib.compress(stream, 6))
    out["zlib_rle_ms"], zr = best(rle)
    out["zlib6_bytes"], out["zlib_rle_bytes"] = len(z6), len(zr)
    try:
        from PIL import Image
    except Exception:
        return out

    def pil():
        f = io.BytesIO()
        Image.fromarray(pixels).save(f, "PNG")
        return f.getvalue()

    out["pillow_ms"], p = best(pil)
    out["pillow_bytes"] = len(p)
    return out


def one(name):
    """One GPU step: prints its JSON line."""
    import torch

    import stereo_match_amd as sma
    from stereo_match_amd import _lib, png

    dev = torch.device("cuda", 0)
    nimg = 16 if name.endswith("_x16") else 1
    if name.startswith("bgr"):
        imgs = np.stack([frame(k) for k in range(nimg)])
        prm = png._image_params("uint8", imgs.shape[1:], None, False)
        pixels = np.ascontiguousarray(imgs[0][..., ::-1])
    elif name.startswith("gray"):
        imgs = frame()[None, :, :, 1].copy()
        prm = png._image_params("uint8", imgs.shape[1:], None, False)
        pixels = imgs[0]
    else:
        imgs = kitti_map()[None]
        prm = png._disp_params("int16", imgs.shape[1:], "kitti", None, None, None)
        pixels = np.where(imgs[0] < 0, 0, imgs[0].astype(np.int32) << 4).astype(np.uint16)
    H, W = imgs.shape[1:3]
    eng = _lib.engine(0)
    st = torch.cuda.Stream(device=dev)
    cap = (_lib.load().sm_png_bound(H, W, *_lib.png_file_geometry(prm)) + 15) & ~15

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
        t = torch.from_numpy(imgs).to(dev)
        row, istr = t.stride(1) * t.element_size(), t.stride(0) * t.element_size()
        out = torch.empty((nimg, cap), dtype=torch.uint8, device=dev)
        nb = torch.zeros(nimg, dtype=torch.int64, device=dev)
        nb_h = torch.zeros(nimg, dtype=torch.int64, pin_memory=True)
        host = torch.empty((nimg, cap), dtype=torch.uint8, pin_memory=True)

        def enc(p=prm, o=out):
            eng.png_encode_batch_device(t.data_ptr(), istr, row, nimg, H, W, p, cap if o is not None else 0,
                                        o.data_ptr() if o is not None else 0, nb.data_ptr())

        full = timed(enc)
        sizes_only = timed(lambda: enc(o=None))
        p0 = type(prm).from_buffer_copy(prm)
        p0.filter = 0
        fixed = timed(lambda: enc(p=p0))
        enc()
        sizes = [int(x) for x in nb.cpu()]
        walls = []
        for _ in range(10):
            st.synchronize()
            t0 = time.perf_counter()
            enc()
            nb_h.copy_(nb, non_blocking=True)
            st.synchronize()
            m = int(nb_h.max())
            host[:, :m].copy_(out[:, :m], non_blocking=True)
            st.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
    eng.set_stream(None)
    file0 = host[0, :sizes[0]].numpy().tobytes()
    host_equal = file0 == (sma.imencode_png_host(imgs[0]) if name != "kitti_map"
                           else sma.encode_disparity_png(imgs[0], "kitti", host=True))
    stream = stream_of(file0)
    res = dict(what="png", workload=name, H=int(H), W=int(W), images=nimg, stream_bytes=len(stream), file_bytes=sizes[0],
               device_us=full[0], device_us_min=full[1], sizes_only_us=sizes_only[0], fixed_none_us=fixed[0],
               wall_to_pinned_ms=round(float(np.median(walls)), 3), host_twin_equal=bool(host_equal))
    res.update(cpu_times(pixels, stream))
    if "zlib6_ms" in res:
        res["zlib6_over_wall"] = round(res["zlib6_ms"] * nimg / res["wall_to_pinned_ms"], 1)
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
            sys.exit(f"png_bench: the step {name} ended with status {r.returncode}; stopping")
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

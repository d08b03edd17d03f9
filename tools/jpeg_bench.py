"""Device time of the JPEG decoder: HIP events on one stream around
sm_jpeg_decode_batch_device (files and descriptors already in device memory), 5 warm-up launches +
30 timed, the median reported; the wall time of file in host memory -> pixels on the device
(imdecode with as_tensor=True, or imdecode_batch: parse, staging, upload, decode, status read-back)
likewise.
    python tools/jpeg_bench.py [--out profiles/jpeg/jpeg_bench.jsonl] [--label TEXT] [--only NAME,NAME]
Workloads: 1280x720 and 1920x1440 4:2:0 frames at quality 90 written by Pillow (libjpeg-turbo),
without restart markers and with one per MCU row, a single frame and a batch of 16 different
frames.  The pictures are random-dot stereo frames over a ramp (png_bench.py's recipe at either
size): busy content, so the files are large for their size.  On the same machine's CPU in the same
run, one thread: pillow_ms, Pillow's full decode of the same bytes (best of 3, one file).
The library under STEREO_MATCH_AMD_LIB is the one measured (builds with another SM_JD_SUBSEQ for
the sub-sequence study); --label goes into every line.  Per-kernel times come from a kernel trace
of one step of this tool (--one), kept beside the output.  Every GPU step is a child process of
its own under a time limit; the first one that fails ends the run.  One JSON object per line."""
import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"720p": (720, 1280), "1440p": (1440, 1920)}
WORKLOADS = tuple(f"{s}{r}{b}" for s in SIZES for r in ("", "_rst") for b in ("", "_x16"))
WARMUP, TIMED = 5, 30
STEP_TIMEOUT_S = 240


def frame(H, W, seed=0):
    from stereo_match_amd import synthetic

    left, right, _ = synthetic.random_dot_pair(H, W, 64, seed=seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = ((xx + 2 * yy) // 8 % 256).astype(np.uint8)
    return np.stack([left // 2 + ramp // 2, ramp, right // 2 + ramp // 2], -1).astype(np.uint8)


def one(name, label):
    """One GPU step: prints its JSON line."""
    import torch
    from PIL import Image

    import stereo_match_amd as sma
    from stereo_match_amd import _lib, jpeg

    dev = torch.device("cuda", 0)
    nimg = 16 if name.endswith("_x16") else 1
    H, W = SIZES[name.split("_")[0]]
    kw = dict(quality=90, subsampling=2)
    if "_rst" in name:
        kw["restart_marker_rows"] = 1
    files, want = [], []
    for k in range(nimg):
        b = io.BytesIO()
        Image.fromarray(frame(H, W, k)).save(b, "JPEG", **kw)
        files.append(b.getvalue())
        want.append(np.asarray(Image.open(io.BytesIO(files[-1]))))

    def pil():
        im = Image.open(io.BytesIO(files[0]))
        im.load()

    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        pil()
        ts.append((time.perf_counter() - t0) * 1e3)
    pillow_ms = round(min(ts), 2)

    arrs = [np.frombuffer(f, np.uint8) for f in files]
    info = _lib.jpeg_info(arrs[0])
    prm, shape = jpeg._params(info, 1, False)
    descs = [_lib.jpeg_parse(f) for f in arrs]
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
        dsz = descs[0].size
        sizes = np.array([len(f) for f in files], np.int64)
        base = (nimg * dsz + 15) & ~15
        offs = (base + np.concatenate([[0], np.cumsum((sizes + 15) & ~15)[:-1]])).astype(np.int64)
        blob = np.zeros(int(offs[-1] + sizes[-1]), np.uint8)
        for i, (f, o) in enumerate(zip(arrs, offs)):
            blob[i * dsz:(i + 1) * dsz] = descs[i]
            blob[o:o + f.size] = f
        d_blob = torch.from_numpy(blob).to(dev)
        d_tab = torch.from_numpy(np.stack([offs, sizes])).to(dev)
        out = torch.empty((nimg,) + shape, dtype=torch.uint8, device=dev)
        status = torch.empty(nimg, dtype=torch.int32, device=dev)
        prm.max_file_bytes = int(sizes.max())
        prm.d_desc = d_blob.data_ptr()

        def dec():
            eng.jpeg_decode_batch_device(d_blob.data_ptr(), d_tab[0].data_ptr(), d_tab[1].data_ptr(), nimg, H, W, prm,
                                         out.data_ptr(), out.stride(0), out.stride(1), status.data_ptr())

        full = timed(dec)
        dec()
        ok = status.cpu().tolist() == [0] * nimg
        lanes, rounds = eng.jpeg_decode_stats()
        got = out.cpu().numpy()
        equal = ok and all(np.array_equal(got[i][:, :, ::-1], want[i]) for i in range(nimg))
        walls = []
        for _ in range(10):
            st.synchronize()
            t0 = time.perf_counter()
            t = sma.imdecode_batch(files, 1) if nimg > 1 else sma.imdecode(files[0], 1, as_tensor=True)
            st.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        del t
    eng.set_stream(None)
    res = dict(what="jpegdec", label=label, workload=name, H=H, W=W, images=nimg, file_bytes=len(files[0]),
               restart_markers="_rst" in name, lanes=lanes, lanes_per_image=lanes // nimg, max_sync_rounds=rounds,
               device_us=full[0], device_us_min=full[1], device_us_per_image=round(full[0] / nimg, 1),
               wall_host_file_to_tensor_ms=round(float(np.median(walls)), 3), pixels_equal_pillow=bool(equal),
               pillow_ms=pillow_ms, pillow_all_images_over_device=round(pillow_ms * nimg * 1e3 / full[0], 2),
               pillow_all_images_over_wall=round(pillow_ms * nimg / float(np.median(walls)), 2))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--label", default="default")
    ap.add_argument("--only", default="")
    ap.add_argument("--one", metavar="WORKLOAD", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(args.one, args.label)
        return
    names = [n for n in WORKLOADS if not args.only or n in args.only.split(",")]
    lines = []
    for name in names:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--label", args.label]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
        if r.returncode != 0:
            sys.exit(f"jpeg_bench: the step {name} ended with status {r.returncode}; stopping")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln)
                print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

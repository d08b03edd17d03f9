"""Device time of the point-cloud tail: HIP events on one stream around
sm_cloud_extract_batch_device, sm_ply_format_device and sm_cloud_ply_batch_device (maps -> PLY
bytes), 5 warm-up launches + 50 timed, the median reported; the device-to-host copy of the body
into pinned memory likewise.  The formatter's write pass is timed in both its forms (a block's rows
staged in LDS, the default; rows straight to global memory, SM_TUNE_PLY_STAGE -1) and their bytes
compared.
    python tools/ply_bench.py [--out profiles/ply/ply_bench.jsonl] [--no-parent]
Per frame size (1280x720, the reference's, and 1242x375) and mask:
  all                    no bounds, every pixel a row
  disparity_calculation  int16 x16 map, 10 < disp < 20, non-finite zeroed  (:302-320)
  disparity_test         float32 / 16, disp > 2, non-finite zeroed         (:230-265)
  try_try                float32 / 16, disp > disp.min()                   (:90-96)
on a synthetic map (uniform 0..39 in x16 units, one pixel in ten invalid).
  parent   the path this replaces, timed on the same machine in the same run for the same inputs:
           sma.reprojectImageTo3D -> numpy mask -> sma.write_ply into a file in memory (/dev/shm
           where there is one); the new path's bytes are compared with that file
  new      wall time of device maps -> body in pinned host memory (fused call + copy + sync)
Every GPU step is a child process of its own under a time limit; the first one that fails ends
the run.  One JSON object per line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(720, 1280), (375, 1242)]
MASKS = ("all", "disparity_calculation", "disparity_test", "try_try")
WARMUP, TIMED = 5, 50
STEP_TIMEOUT_S = 240


def case(H, W, mask):
    """(map, Q, BGR image, lo, hi, zero_nonfinite)"""
    rng = np.random.default_rng(41)
    d = rng.integers(0, 40, (H, W)).astype(np.int16)
    d[rng.random((H, W)) < 0.1] = -16
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    Q = np.float32([[1, 0, 0, -640], [0, -1, 0, 360], [0, 0, 0, -1164], [0, 0, 1, 0]])
    if mask == "all":
        return d, Q, img, None, None, False
    if mask == "disparity_calculation":
        return d, Q, img, 10, 20, True
    d = d.astype(np.float32) * 8 / np.float32(16.0)
    if mask == "disparity_test":
        Q = np.float32([[1, 0, 0, -360], [0, -1, 0, 640], [0, 0, 0, -1164], [0, 0, -1 / -22, 0]])
        return d, Q, img, 2, None, True
    Q = np.float32([[1, 0, 0, -0.5 * W], [0, -1, 0, 0.5 * H], [0, 0, 0, -0.8 * W], [0, 0, 1, 0]])
    return d, Q, img, "min", None, False


def parent_path(d, Q, img, lo, hi, zero, fn):
    """The tail as the parent commit runs it; returns its wall time in seconds."""
    import stereo_match_amd as sma

    t0 = time.perf_counter()
    points = sma.reprojectImageTo3D(d, Q)
    colors = img[..., ::-1]
    mask = np.ones(d.shape, bool)
    if isinstance(lo, str):
        mask &= d > d.min()
    elif lo is not None:
        mask &= d > lo
    if hi is not None:
        mask &= d < hi
    out_points, out_colors = points[mask], colors[mask]
    if zero:
        out_points[np.isnan(out_points)] = 0
        out_points[np.isinf(out_points)] = 0
    sma.write_ply(fn, out_points, out_colors)
    return time.perf_counter() - t0


def one(H, W, mask, with_parent):
    """One GPU step: prints its JSON line."""
    import torch

    from stereo_match_amd import _lib, pointcloud

    d, Q, img, lo, hi, zero = case(H, W, mask)
    kind = 0 if d.dtype == np.int16 else 1
    prm = pointcloud._cloud_params(lo, hi, zero, False)
    dev = torch.device("cuda", 0)
    eng = _lib.engine(0)
    st = torch.cuda.Stream(device=dev)
    npx = H * W

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
        td, ti = torch.from_numpy(d).to(dev), torch.from_numpy(img).to(dev)
        verts = torch.empty((npx, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((npx, 3), dtype=torch.uint8, device=dev)
        meta = torch.zeros(2, dtype=torch.int64, device=dev)  # rows, bytes
        maps = (td.data_ptr(), kind, ti.data_ptr(), 0, 3 * W, 1, H, W, Q, prm)
        # sizes first
        eng.cloud_ply_batch_device(*maps, 0, 0, meta.data_ptr(), meta.data_ptr() + 8)
        n, nbytes = (int(x) for x in meta.cpu())
        body = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        host = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
        extract = timed(lambda: eng.cloud_extract_batch_device(*maps, npx, verts.data_ptr(), colors.data_ptr(),
                                                               meta.data_ptr()))
        fmt = timed(lambda: eng.ply_format_device(verts.data_ptr(), colors.data_ptr(), n, nbytes, body.data_ptr(),
                                                  meta.data_ptr() + 8))
        # the write pass with every row straight to global memory (SM_TUNE_PLY_STAGE -1) against the
        # default, a block's rows staged in LDS: same bytes
        staged = body.clone()
        eng.set_tuning(eng.TUNE_PLY_STAGE, -1)
        body.zero_()
        fmt_direct = timed(lambda: eng.ply_format_device(verts.data_ptr(), colors.data_ptr(), n, nbytes, body.data_ptr(),
                                                      meta.data_ptr() + 8))
        direct_equal = bool(torch.equal(staged, body))
        eng.set_tuning(eng.TUNE_PLY_STAGE, 0)
        fused = timed(lambda: eng.cloud_ply_batch_device(*maps, nbytes, body.data_ptr(), meta.data_ptr(),
                                                         meta.data_ptr() + 8))
        d2h = timed(lambda: host.copy_(body, non_blocking=True))
        walls = []
        for _ in range(10):
            st.synchronize()
            t0 = time.perf_counter()
            eng.cloud_ply_batch_device(*maps, nbytes, body.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8)
            host.copy_(body, non_blocking=True)
            st.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        st.synchronize()
    eng.set_stream(None)
    res = dict(what="ply", H=H, W=W, mask=mask, map=str(d.dtype), rows=n, bytes=nbytes,
               extract_us=extract[0], extract_us_min=extract[1], format_us=fmt[0], format_us_min=fmt[1],
               format_direct_stores_us=fmt_direct[0], format_direct_stores_us_min=fmt_direct[1],
               direct_stores_equal=direct_equal,
               fused_us=fused[0], fused_us_min=fused[1], d2h_us=d2h[0], d2h_us_min=d2h[1],
               new_wall_ms=round(float(np.median(walls)), 3))
    if with_parent:
        tmp = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
        fn = os.path.join(tmp, f"ply_bench_{os.getpid()}.ply")
        try:
            sec = parent_path(d, Q, img, lo, hi, zero, fn)
            with open(fn, "rb") as f:
                ref = f.read()
        finally:
            if os.path.exists(fn):
                os.remove(fn)
        head = ref.index(b"end_header\n") + len(b"end_header\n")
        res.update(parent_ms=round(sec * 1e3, 1), parent_body_equal=bool(ref[head:] == host[:nbytes].numpy().tobytes()),
                   parent_over_new_device=round(sec * 1e6 / (fused[0] + d2h[0]), 1),
                   parent_over_new_wall=round(sec * 1e3 / float(np.median(walls)), 1))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--one", nargs=3, metavar=("H", "W", "MASK"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(int(args.one[0]), int(args.one[1]), args.one[2], not args.no_parent)
        return
    lines = []
    for H, W in SHAPES:
        for mask in MASKS:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", str(H), str(W), mask]
            if args.no_parent:
                cmd.append("--no-parent")
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
            if r.returncode != 0:
                sys.exit(f"ply_bench: the step {H}x{W} {mask} ended with status {r.returncode}; stopping")
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

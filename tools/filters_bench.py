"""Device time of image_measure, the float64 Gaussian and pyrDown: HIP events
around the device entry points on one stream, 1280x720 frames, 5 warm-up launches + 50 timed
back to back (each between its own pair of events), the median reported.
    python tools/filters_bench.py [--out profiles/filters/filters_bench.jsonl] [--no-cpu]
  image_measure  sm_image_measure_u8_batch_device (two launches) at 1, 2 and 16 images; 1 is what
                 disparity_test.py:82-83 does, one call per image
  gauss          sm_gauss2d_f64_batch_device at sigma 5, one image
  pyr_down       sm_pyr_down_u8_batch_device, BGR, at 1 and 16 images
  cpu_*          the host path on this machine's CPU for one frame: scipy.ndimage (the
                 reference's own two filters) if it imports, else the numpy restatement
                 tests/filters_np.py, named as such; pyrDown always the restatement (there is
                 no cv2 to time: this is not OpenCV's figure).  Never the code under test.
Per line: the compulsory bytes and the float64 operations computed from the shape, and the
rates they give over the measured time.  Every GPU step is a child process of its own under a
time limit; the first one that fails ends the run.  One JSON object per line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 720, 1280
STEPS = [("image_measure", 1), ("image_measure", 2), ("image_measure", 16), ("gauss", 1), ("pyr_down", 1),
         ("pyr_down", 16)]
WARMUP, TIMED = 5, 50
STEP_TIMEOUT_S = 120


def gauss_flops(r):
    """float64 operations per pixel of one 2-D filter: per axis 1 multiply + r (2 adds + 1 multiply)."""
    return 2 * (1 + 3 * r)


def one(what, nimg):
    """One GPU step: prints its JSON line."""
    import torch

    import filters_np
    from stereo_match_amd import _lib, filters

    dev = torch.device("cuda", 0)
    eng = _lib.engine(0)
    st = torch.cuda.Stream(device=dev)
    w5, w3 = (filters.gaussian_kernel1d(s)[0][filters.gaussian_kernel1d(s)[1]:] for s in (5, 3))
    npx = H * W
    with torch.cuda.stream(st):
        eng.set_stream(st.cuda_stream)
        if what == "gauss":
            src = torch.from_numpy(np.stack([filters_np.image_f64(H, W, 100 + i) for i in range(nimg)])).to(dev)
            dst = torch.empty_like(src)

            def launch():
                eng.gauss2d_batch_device(src.data_ptr(), nimg, npx, H, W, W, w5, w5, dst.data_ptr(), npx, W)
            nbytes, flops = 16 * npx, gauss_flops(20) * npx
        else:
            src = torch.from_numpy(np.stack([filters_np.image_u8(H, W, 100 + i) for i in range(nimg)])).to(dev)
            if what == "image_measure":
                dst = torch.empty((nimg, H, W), dtype=torch.float64, device=dev)

                def launch():
                    eng.image_measure_batch_device(src.data_ptr(), nimg, npx * 3, H, W, W * 3, w5, w3, 30.0,
                                                   dst.data_ptr())
                # 3 B in, a written and read again, 8 B out (halo and unsharp re-reads are not compulsory)
                nbytes, flops = (3 + 8 + 8 + 8) * npx, (gauss_flops(20) + gauss_flops(12) + 3) * npx
            else:
                dH, dW = (H + 1) // 2, (W + 1) // 2
                dst = torch.empty((nimg, dH, dW, 3), dtype=torch.uint8, device=dev)

                def launch():
                    eng.pyr_down_batch_device(src.data_ptr(), nimg, npx * 3, H, W, W * 3, 3, dst.data_ptr(),
                                              dH * dW * 3, dW * 3)
                nbytes, flops = 3 * npx + 3 * dH * dW, 0
        ts = []
        for it in range(WARMUP + TIMED):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ts.append(a.elapsed_time(b) * 1e3)
        st.synchronize()
    eng.set_stream(None)
    us, lo = float(np.median(ts)), float(np.min(ts))
    line = dict(what=what, H=H, W=W, nimg=nimg, us=round(us, 1), us_min=round(lo, 1), us_per_image=round(us / nimg, 1),
                compulsory_MB_per_image=round(nbytes / 1e6, 2), GB_per_s=round(nimg * nbytes / us / 1e3, 1))
    if flops:
        line.update(f64_Mflop_per_image=round(flops / 1e6, 1), f64_Gflop_per_s=round(nimg * flops / us / 1e3, 1))
    print(json.dumps(line), flush=True)


def cpu_lines():
    import filters_np

    bgr = filters_np.image_u8(H, W, 100)
    gray = filters_np.bgr2gray(bgr).astype(float)
    try:
        from scipy import ndimage

        def measure():
            a = ndimage.gaussian_filter(gray, sigma=5)
            return a + 30 * (a - ndimage.gaussian_filter(a, 3))
        name = "cpu_scipy_two_gaussian_filters"
    except ImportError:
        def measure():
            a = filters_np.gaussian_filter(gray, 5)
            return a + 30 * (a - filters_np.gaussian_filter(a, 3))
        name = "cpu_numpy_restatement_two_gaussian_filters"
    for what, fn in ((name, measure), ("cpu_numpy_restatement_pyr_down_bgr", lambda: filters_np.pyr_down(bgr))):
        fn()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        yield json.dumps(dict(what=what, H=H, W=W, nimg=1, ms=round(float(np.median(ts)), 1),
                              ms_min=round(min(ts), 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--one", nargs=2, metavar=("WHAT", "NIMG"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(args.one[0], int(args.one[1]))
        return
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for what, nimg in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what, str(nimg)],
                           stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
        if r.returncode != 0:
            sys.exit(f"filters_bench: the step {what} x{nimg} ended with status {r.returncode}; stopping")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                emit(ln)
    if not args.no_cpu:
        for ln in cpu_lines():
            emit(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

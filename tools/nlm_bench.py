"""Device time of fastNlMeansDenoising: HIP events around
sm_nlm_denoise_u8_batch_device on one stream for (h, templateWindowSize, searchWindowSize) =
(10, 7, 21), 5 warm-up launches + 50 timed, the median reported.
    python tools/nlm_bench.py [--out profiles/nlm/nlm_bench.jsonl] [--no-cpu]
Per frame size (1280x720, the reference's, and 1242x375) and 1, 2 and 16 images per launch
(1 is what disparity_test.py:94-95 does: one call per image):
  nlm        the launch time, per image, and the derived pixel x offsets per second
  cpu        the vectorised numpy restatement tests/nlm_np.py on this host's CPU for one frame
             (there is no cv2 to time: this is not OpenCV's figure)
Every GPU step is a child process of its own under a time limit; the first one that fails
ends the run.  One JSON object per line."""
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

SHAPES = [(720, 1280), (375, 1242)]
NIMG = (1, 2, 16)
PRM = (10.0, 7, 21)
WARMUP, TIMED = 5, 50
STEP_TIMEOUT_S = 120


def one(H, W, nimg):
    """One GPU step: prints its JSON line."""
    import torch

    import nlm_np
    from stereo_match_amd import _lib

    dev = torch.device("cuda", 0)
    eng = _lib.engine(0)
    st = torch.cuda.Stream(device=dev)
    host = np.stack([nlm_np.noisy_blobs(H, W, seed=100 + i) for i in range(nimg)])
    with torch.cuda.stream(st):
        eng.set_stream(st.cuda_stream)
        src = torch.from_numpy(host).to(dev)
        dst = torch.empty_like(src)
        ts = []
        for it in range(WARMUP + TIMED):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.nlm_denoise_batch_device(src.data_ptr(), nimg, H * W, H, W, W, *PRM, dst.data_ptr())
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ts.append(a.elapsed_time(b) * 1e3)
        st.synchronize()
    eng.set_stream(None)
    us, lo = float(np.median(ts)), float(np.min(ts))
    s = 2 * (PRM[2] // 2) + 1
    changed = float((dst[0].cpu().numpy() != host[0]).mean())
    print(json.dumps(dict(what="nlm", H=H, W=W, nimg=nimg, h=PRM[0], template=PRM[1], search=PRM[2],
                          us=round(us, 1), us_min=round(lo, 1), us_per_image=round(us / nimg, 1),
                          Gpixel_offsets_per_s=round(nimg * H * W * s * s / us / 1e3, 1),
                          pixels_changed=round(changed, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--one", nargs=3, type=int, metavar=("H", "W", "NIMG"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one(*args.one)
        return
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for H, W in SHAPES:
        for nimg in NIMG:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(H), str(W), str(nimg)],
                               stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
            if r.returncode != 0:
                sys.exit(f"nlm_bench: the step {H}x{W} x{nimg} ended with status {r.returncode}; stopping")
            for ln in r.stdout.splitlines():
                if ln.startswith("{"):
                    emit(ln)
        if not args.no_cpu:
            import nlm_np

            img = nlm_np.noisy_blobs(H, W, seed=100)
            t0 = time.perf_counter()
            nlm_np.denoise(img, int(PRM[0]), PRM[1], PRM[2])
            emit(json.dumps(dict(what="cpu_vectorised_numpy_restatement", H=H, W=W, nimg=1,
                                 ms=round((time.perf_counter() - t0) * 1e3, 1))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

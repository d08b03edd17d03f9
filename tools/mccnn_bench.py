#!/usr/bin/env python3
"""Device time of the MC-CNN matching cost: features per image and the join, at
1280x720 with 228 planes and 1242x375 with 192, single and in a batch of 8, against (a) the
f32-MFMA floor of the 64 -> 64 layers at 155 TFLOP/s, (b) the join's store floor at 5.3 TB/s,
(c) torch's own conv2d + join on the same GPU, and the host-to-device copy of the volume that
computing it on the device saves.  HIP events on one stream; every shape is warmed up first.

    python tools/mccnn_bench.py [--out profiles/mccnn/mccnn_bench.jsonl] [--reps 20] [--layers 4]

One JSON line per measurement (times in ms: the median and the range of the repeats)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F32_TFLOPS = 155.0  # measured rate of the f32-input matrix instruction
STORE_TBS = 5.3          # store bandwidth this project measured (tools/ubench/write_bw.hip)


def timed(fn, reps, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": reps}


def torch_features(t, ws, bs):
    import torch
    import torch.nn.functional as F

    x = t.to(torch.float32)
    x = ((x - x.mean(dim=(1, 2), keepdim=True)) / x.std(dim=(1, 2), keepdim=True))[:, None]
    for i, (w, b) in enumerate(zip(ws, bs)):
        x = F.conv2d(x, w, b, padding=1)
        if i < len(ws) - 1:
            x = F.relu_(x)
    return x / x.pow(2).sum(1, keepdim=True).sqrt()  # [N, 64, H, W]


def torch_join(fa, fb, D):
    import torch

    n, _, H, W = fa.shape
    vol = torch.full((n, D, H, W), float("nan"), dtype=torch.float32, device=fa.device)
    for d in range(min(D, W)):
        vol[:, d, :, d:] = -(fa[:, :, :, d:] * fb[:, :, :, :W - d]).sum(1)
    return vol


def main():
    import torch

    import stereo_match_amd as sm

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--sizes", default="1280x720x228,1242x375x192")
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mccnn_bench needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    m = sm.McCnnFast.random(args.layers, 0)
    ws = [torch.tensor(w, device=dev) for w in m.weights]
    bs = [torch.tensor(b, device=dev) for b in m.biases]
    rng = np.random.default_rng(0)
    rows = []

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(kw) + "\n")

    for size in args.sizes.split(","):
        W, H, D = (int(v) for v in size.split("x"))
        for n in (int(v) for v in args.batches.split(",")):
            a = torch.from_numpy(rng.integers(0, 256, (n, H, W), dtype=np.uint8)).to(dev)
            b = torch.roll(a, -7, 2).contiguous()
            base = {"W": W, "H": H, "D": D, "batch": n, "layers": args.layers}
            flop = 2.0 * 576 * 64 * H * W * (args.layers - 1) * n
            floor_feat = flop / (MFMA_F32_TFLOPS * 1e12) * 1e3
            vbytes = 4.0 * n * D * H * W
            floor_join = vbytes / (STORE_TBS * 1e12) * 1e3
            fa, fb = m.features(a), m.features(b)
            r = timed(lambda: m.features(a), args.reps)
            emit(what="features", **base, **r, ms_per_image=r["ms"] / n, mfma_floor_ms=floor_feat,
                 ratio_to_mfma_floor=r["ms"] / floor_feat, tflops=flop / r["ms"] / 1e9)
            r = timed(lambda: m.join(fa, fb, D), args.reps)
            emit(what="join", **base, **r, ms_per_pair=r["ms"] / n, store_floor_ms=floor_join,
                 ratio_to_store_floor=r["ms"] / floor_join, store_tbs=vbytes / r["ms"] / 1e9)
            r = timed(lambda: m.cost_volume(a, b, D), max(3, args.reps // 2))
            emit(what="cost_volume", **base, **r, ms_per_pair=r["ms"] / n)
            del fa, fb
            with torch.no_grad():
                ta, tb = torch_features(a, ws, bs), torch_features(b, ws, bs)
                rt = timed(lambda: torch_features(a, ws, bs), args.reps)
                emit(what="torch_features", **base, **rt, ms_per_image=rt["ms"] / n)
                rt = timed(lambda: torch_join(ta, tb, D), max(3, args.reps // 4))
                emit(what="torch_join", **base, **rt, ms_per_pair=rt["ms"] / n)
                del ta, tb
            if n == 1:  # what computing the volume on the device saves: its copy from pinned host memory
                host = torch.empty((1, D, H, W), dtype=torch.float32).pin_memory()
                dst = torch.empty((1, D, H, W), dtype=torch.float32, device=dev)
                r = timed(lambda: dst.copy_(host, non_blocking=True), max(3, args.reps // 2))
                emit(what="volume_h2d_pinned", **base, **r, gbs=vbytes / r["ms"] / 1e6)
                del host, dst
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the accurate MC-CNN matching cost: features per image, the join
of one view (both projections and the scorer) and the join of a single plane (an upper bound of
the projections' share), at 1280x720 with 228 planes and 1242x375 with 192, single and in a batch,
against (a) the f32-MFMA floors of the FLOP counts (2 K N per output) at 155 TFLOP/s and (b) torch
running the same network in the same run: conv2d, then linear plane by plane.  One more line times
the whole McCnnStereo.compute.  HIP events on one stream; every shape is warmed up first.

--precision f32|bf16|both (the default f32 is the run above).  In bf16 mode the join's
floor is the hidden layers' FLOP at the bf16 matrix rate (2.5 PFLOP/s dense, the specification) plus
the projections' and the output unit's at the f32 rate; with "both" the two joins are timed in the
same run, every bf16 line carries its speed-up over that run's f32 figure, and one line per size
gives max and mean |bf16 - f32| of the similarity over the whole volume.

    python tools/mcacc_bench.py [--out profiles/mcacc/mcacc_bench.jsonl] [--reps 10] [--precision both]

One JSON line per measurement (times in ms: the median and the range of the repeats)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F32_TFLOPS = 155.0  # measured rate of the f32-input matrix instruction
MFMA_BF16_TFLOPS = 2500.0  # dense bf16 rate of the specification


def timed(fn, reps, warmup=2):
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
    for w, b in zip(ws, bs):
        x = F.relu_(F.conv2d(x, w, b, padding=1))
    return x.permute(0, 2, 3, 1).contiguous()  # [N, H, W, 112]


def torch_join(fa, fb, D, fws, fbs):
    """The same split first layer, then linear plane by plane (a plane's activations fit; a volume's
    do not)."""
    import torch
    import torch.nn.functional as F

    n, H, W, _ = fa.shape
    pl = F.linear(fa, fws[0][:, :112], fbs[0])
    pr = F.linear(fb, fws[0][:, 112:])
    vol = torch.full((n, D, H, W), float("nan"), dtype=torch.float32, device=fa.device)
    for d in range(min(D, W)):
        h = F.relu_(pl[:, :, d:] + pr[:, :, :W - d])
        for w, b in zip(fws[1:-1], fbs[1:-1]):
            h = F.relu_(F.linear(h, w, b))
        vol[:, d, :, d:] = -torch.sigmoid(F.linear(h, fws[-1], fbs[-1])[..., 0])
    return vol


def main():
    import torch

    import stereo_match_amd as sm

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--fc-layers", type=int, default=3)
    ap.add_argument("--units", type=int, default=384)
    ap.add_argument("--sizes", default="1280x720x228,1242x375x192")
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-stereo", action="store_true")
    ap.add_argument("--precision", choices=("f32", "bf16", "both"), default="f32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcacc_bench needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    L, F, U = args.layers, args.fc_layers, args.units
    m = sm.McCnnAccurate.random(L, F, U, 0)
    precisions = ("f32", "bf16") if args.precision == "both" else (args.precision,)
    nets = {p: m.with_precision(p) for p in precisions}
    ws = [torch.tensor(w, device=dev) for w in m.weights]
    bs = [torch.tensor(b, device=dev) for b in m.biases]
    fws = [torch.tensor(w, device=dev) for w in m.fc_weights]
    fbs = [torch.tensor(b, device=dev) for b in m.fc_biases]
    rng = np.random.default_rng(0)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(kw) + "\n")

    first = True
    for size in args.sizes.split(","):
        W, H, D = (int(v) for v in size.split("x"))
        for n in (int(v) for v in args.batches.split(",")):
            a = torch.from_numpy(rng.integers(0, 256, (n, H, W), dtype=np.uint8)).to(dev)
            b = torch.roll(a, -7, 2).contiguous()
            base = {"W": W, "H": H, "D": D, "batch": n, "layers": L, "fc_layers": F, "units": U}
            px, cells = float(n * H * W), float(n * D * H * W)
            flop_feat = 2.0 * 9 * 112 * 112 * (L - 1) * px
            flop_proj = 2.0 * 2 * 112 * U * px
            flop_score = (2.0 * U * U * (F - 1) + 2.0 * U) * cells
            floor = lambda flop: flop / (MFMA_F32_TFLOPS * 1e12) * 1e3  # noqa: E731
            fa, fb = m.features(a), m.features(b)
            r = timed(lambda: m.features(a), args.reps)
            emit(what="features", **base, **r, ms_per_image=r["ms"] / n, mfma_floor_ms=floor(flop_feat),
                 ratio_to_mfma_floor=r["ms"] / floor(flop_feat), tflops=flop_feat / r["ms"] / 1e9)
            r = timed(lambda: m.join(fa, fb, 1), args.reps)
            emit(what="join_one_plane", **base, **r, ms_per_pair=r["ms"] / n, projection_mfma_floor_ms=floor(flop_proj))
            flop_hidden = 2.0 * U * U * (F - 1) * cells
            join_ms = {}
            for p, net in nets.items():
                r = timed(lambda: net.join(fa, fb, D), args.reps)
                join_ms[p] = r["ms"]
                if p == "f32":
                    fl = floor(flop_proj + flop_score)
                    emit(what="join", precision=p, **base, **r, ms_per_view=r["ms"] / n, mfma_floor_ms=fl,
                         ratio_to_mfma_floor=r["ms"] / fl, tflops=(flop_proj + flop_score) / r["ms"] / 1e9)
                else:
                    fl = flop_hidden / (MFMA_BF16_TFLOPS * 1e12) * 1e3 + floor(flop_proj + flop_score - flop_hidden)
                    extra = {"speedup_over_f32_same_run": join_ms["f32"] / r["ms"]} if "f32" in join_ms else {}
                    emit(what="join", precision=p, **base, **r, ms_per_view=r["ms"] / n, mfma_floor_ms=fl,
                         ratio_to_mfma_floor=r["ms"] / fl, tflops=(flop_proj + flop_score) / r["ms"] / 1e9, **extra)
            if len(nets) == 2 and n == 1:
                diff = (nets["bf16"].join(fa, fb, D) - nets["f32"].join(fa, fb, D)).abs()
                ok = ~torch.isnan(diff)
                emit(what="similarity_bf16_minus_f32", **base, max_abs=float(diff[ok].max()), mean_abs=float(diff[ok].mean()),
                     cells=int(ok.sum()))
                del diff, ok
            if not args.no_torch:
                with torch.no_grad():
                    rt = timed(lambda: torch_features(a, ws, bs), args.reps)
                    emit(what="torch_features", **base, **rt, ms_per_image=rt["ms"] / n)
                    ta, tb = torch_features(a, ws, bs), torch_features(b, ws, bs)
                    rt = timed(lambda: torch_join(ta, tb, D, fws, fbs), args.reps)
                    emit(what="torch_join", **base, **rt, ms_per_view=rt["ms"] / n, tflops=(flop_proj + flop_score) / rt["ms"] / 1e9)
                    del ta, tb
            del fa, fb
            if first and n == 1 and not args.no_stereo:
                for p, net in nets.items():
                    stereo = sm.McCnnStereo(net)
                    r = timed(lambda: stereo.compute(a[0], b[0], D), max(3, args.reps // 3), warmup=1)
                    emit(what="stereo_compute", precision=p, **base, **r)
            torch.cuda.empty_cache()
        first = False


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the cross-based cost aggregation at 1280x720 and 1242x375 with
228 planes, l1 = 5 and l1 = 14, inputs resident in HBM: the arms of one image, one iteration of the
volume kernel, McCnnStereo.compute without and with the step, next to a device-to-device copy of the
same volume timed in the same run (it reads once and writes once: the yardstick), and the CPU twin
on this machine.  HIP events on one stream, the median of --reps; every shape is warmed up first.

    python tools/mccbca_bench.py [--out profiles/mccbca/mccbca_bench.jsonl] [--reps 10] [--no-twin]
    python tools/mccbca_bench.py --trace    # a few calls of every entry point, for a kernel trace or counters

One JSON line per measurement (times in ms).  A call of mc_cross_aggregate normalises both images
(one wait for their sums), computes their arms and runs `iterations` launches of k_mcb_agg; one
iteration is therefore reported as (call with 3 iterations - call with 1) / 2."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main():
    import torch

    import stereo_match_amd as sm

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1280x720x228,1242x375x228")
    ap.add_argument("--l1", default="5,14")
    ap.add_argument("--no-twin", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mccbca_bench needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    net = sm.McCnnFast.random(4, 0)
    prm = sm.McCnnStereoParams()
    rng = np.random.default_rng(0)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(kw) + "\n")

    for size in args.sizes.split(","):
        W, H, D = (int(v) for v in size.split("x"))
        # blocks of 9 x 12 with a little noise, shifted by 7 columns: arms end at the cap, at block edges and at the border
        tex = rng.integers(0, 256, (H // 9 + 1, W // 12 + 3), dtype=np.uint8).repeat(9, 0).repeat(12, 1).astype(np.int64)
        tex = np.clip(tex + rng.integers(-2, 3, tex.shape), 0, 255).astype(np.uint8)
        left_np, right_np = np.ascontiguousarray(tex[:H, 12:12 + W]), np.ascontiguousarray(tex[:H, 19:19 + W])
        left, right = torch.from_numpy(left_np).to(dev), torch.from_numpy(right_np).to(dev)
        vol = net.cost_volume(left, right, D, 0)
        if args.trace:
            for l1 in (int(v) for v in args.l1.split(",")):
                cp = sm.McCnnCrossParams(l1=l1)
                for _ in range(3):
                    sm.mc_cross_arms(left, cp)
                    sm.mc_cross_aggregate(vol, left, right, 0, cp, 2)
            torch.cuda.synchronize()
            continue
        base = {"W": W, "H": H, "D": D}
        dst = torch.empty_like(vol)
        copy = timed(lambda: dst.copy_(vol), args.reps)
        vbytes = 4.0 * D * H * W
        emit(what="copy", **base, **copy, tb_per_s=2 * vbytes / copy["ms"] * 1e-9,
             note="device-to-device copy of the volume: one read, one write")
        del dst
        for l1 in (int(v) for v in args.l1.split(",")):
            cp = sm.McCnnCrossParams(l1=l1)
            cfg = dict(base, l1=l1, tau1=cp.tau1)
            r = timed(lambda: sm.mc_cross_arms(left, cp), args.reps)
            emit(what="arms_call", **cfg, **r, note="one image: its sums (one wait), the table, k_mcs_norm, k_mcb_arms")
            one = timed(lambda: sm.mc_cross_aggregate(vol, left, right, 0, cp, 1), args.reps)
            three = timed(lambda: sm.mc_cross_aggregate(vol, left, right, 0, cp, 3), args.reps)
            emit(what="aggregate_call", **cfg, **one, iterations=1,
                 note="both images normalised (one wait), their arms, one launch of k_mcb_agg, the output's allocation")
            it = (three["ms"] - one["ms"]) / 2
            emit(what="iteration", **cfg, ms=it, copy_ms=copy["ms"], ratio_to_copy=it / copy["ms"],
                 note="(call with 3 iterations - call with 1) / 2, medians of %d" % args.reps)
            plain, crossed = sm.McCnnStereo(net, prm), sm.McCnnStereo(net, prm, cp)
            r = timed(lambda: plain.compute(left, right, D, 0), max(3, args.reps // 2))
            emit(what="compute", **cfg, cross=None, **r,
                 note="cross=None: the method as before this step existed; compare with profiles/mcsgm/mcsgm_bench.jsonl")
            r = timed(lambda: crossed.compute(left, right, D, 0), max(3, args.reps // 2))
            emit(what="compute", **cfg, cross=dict(l1=cp.l1, tau1=cp.tau1, i1=cp.i1, i2=cp.i2), **r)
            if not args.no_twin:
                got = sm.mc_cross_aggregate(vol, left, right, 0, cp, 1).cpu().numpy()
                v_np = vol.cpu().numpy()
                t0 = time.perf_counter()
                twin = sm.mc_cross_aggregate(v_np, left_np, right_np, 0, cp, 1, host=True)
                t1 = time.perf_counter()
                nan = np.isnan(twin)
                same = bool(np.array_equal(nan, np.isnan(got)) and np.array_equal(twin[~nan].view(np.uint32), got[~nan].view(np.uint32)))
                emit(what="twin_aggregate", **cfg, ms=(t1 - t0) * 1e3, threads=1, equals_device=same)
                del got, v_np, twin
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

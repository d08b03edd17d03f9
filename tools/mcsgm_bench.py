#!/usr/bin/env python3
"""Device time of MC-CNN's stereo method at 1280x720 and 1242x375 with 228 planes,
inputs resident in HBM: the aggregation, the disparity step, the whole McCnnStereo.compute, next to
(a) the traffic floor of the aggregation (the volume read once and written once at the 6.29 TB/s
copy rate), (b) computeFromCost on the same volume, (c) the CPU twin on this machine.  HIP events
on one stream; every shape is warmed up first.

    python tools/mcsgm_bench.py [--out profiles/mcsgm/mcsgm_bench.jsonl] [--reps 10] [--no-twin]
    python tools/mcsgm_bench.py --trace    # a few calls of every entry point, for a kernel trace or counters

One JSON line per measurement (times in ms: the median and the range of the repeats).  The time of
each kernel (the vertical pair r2 / r3, the horizontal pair r0 / r1 with the sum, every stage of the
disparity step) comes from a kernel trace of the --trace run."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29  # measured device copy rate of the MI355X


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
    ap.add_argument("--no-twin", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcsgm_bench needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    net = sm.McCnnFast.random(4, 0)
    prm = sm.McCnnStereoParams()
    stereo = sm.McCnnStereo(net, prm)
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
        base = {"W": W, "H": H, "D": D}
        # a textured pair with a shift, so that the intensity steps and the interpolation have work
        tex = rng.integers(0, 256, (H // 2 + 1, W // 3 + 9), dtype=np.uint8).repeat(2, 0).repeat(3, 1)
        left_np, right_np = np.ascontiguousarray(tex[:H, 12:12 + W]), np.ascontiguousarray(tex[:H, 19:19 + W])
        left, right = torch.from_numpy(left_np).to(dev), torch.from_numpy(right_np).to(dev)
        m_r = sm.mcstereo.right_min_disparity(D, 0)
        vol_l, vol_r = net.cost_volume(left, right, D, 0), net.cost_volume(right, left, D, m_r)
        agg_l = sm.mc_aggregate(vol_l, left, right, 0, prm)
        agg_r = sm.mc_aggregate(vol_r, right, left, m_r, prm)
        if args.trace:
            for _ in range(3):
                sm.mc_aggregate(vol_l, left, right, 0, prm)
                sm.mc_disparity(agg_l, agg_r, left, 0, prm)
            torch.cuda.synchronize()
            continue
        vbytes = 4.0 * D * H * W
        floor = 2 * vbytes / (COPY_TBS * 1e12) * 1e3
        r = timed(lambda: sm.mc_aggregate(vol_l, left, right, 0, prm), args.reps)
        emit(what="aggregate", **base, **r, traffic_floor_ms=floor, ratio_to_floor=r["ms"] / floor,
             note="one view; includes the images' sums (one wait) and the output's allocation")
        r = timed(lambda: sm.mc_disparity(agg_l, agg_r, left, 0, prm), args.reps)
        emit(what="disparity", **base, **r)
        r = timed(lambda: stereo.compute(left, right, D, 0), max(3, args.reps // 2))
        emit(what="compute", **base, **r, note="features, two volumes, two aggregations, the disparity step")
        matcher = sm.StereoSGBM_create(numDisparities=D, P1=200, P2=2000, disp12MaxDiff=1, uniquenessRatio=15)
        r = timed(lambda: matcher.computeFromCost(vol_l, 1.0, 2047.5), args.reps)
        emit(what="computeFromCost", **base, **r, note="the u16 SGBM engine on the same volume, one view")
        if not args.no_twin:
            v_np, a_np = vol_l.cpu().numpy(), agg_l.cpu().numpy()
            t0 = time.perf_counter()
            twin = sm.mc_aggregate(v_np, left_np, right_np, 0, prm, host=True)
            t1 = time.perf_counter()
            same = bool(np.array_equal(np.isnan(twin), np.isnan(a_np)) and np.array_equal(twin[~np.isnan(twin)], a_np[~np.isnan(a_np)]))
            emit(what="twin_aggregate", **base, ms=(t1 - t0) * 1e3, threads=1, equals_device=same)
            ar_np = agg_r.cpu().numpy()
            t0 = time.perf_counter()
            twin_d = sm.mc_disparity(twin, ar_np, left_np, 0, prm, host=True)
            t1 = time.perf_counter()
            dev_d = sm.mc_disparity(agg_l, agg_r, left, 0, prm).cpu().numpy()
            emit(what="twin_disparity", **base, ms=(t1 - t0) * 1e3, threads=1, equals_device=bool(np.array_equal(twin_d, dev_d)))
            del v_np, a_np, twin, ar_np
        del vol_l, vol_r, agg_l, agg_r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

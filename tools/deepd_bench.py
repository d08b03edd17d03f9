#!/usr/bin/env python3
"""Device time of the matcher at numDisparities 272..512 against the D = 256
per-direction engine (debug flag 4096), the engine the new range is built on.

    python tools/deepd_bench.py [--out profiles/deepd/deepd_bench.jsonl] [--reps 5] [--check]
    python tools/deepd_bench.py --baseline-only      # the D = 256 lines alone (runs on a parent checkout too)

Points: 2880 x 1988 at D = 256 (flag 4096: the baseline), 272, 384 and 512, census8 and sgbm8, 1
and 4 pairs per call; 1242 x 375 at D = 272.  Per point: HIP-event time of sm_compute_batch_device
per pair after warm-up (median and range of --reps calls), the time per pixel x disparity x path
relative to the D = 256 baseline of the same cost kind and batch, and the stage split of one more,
timed call (sm_set_timing; stage events delay the stream a little, so the split is not the total).
--check computes one full-size pair per cost kind at D = 512 on the CPU oracle (ref_c.compute, a
minute or two each) and records whether the device's map equals it: the evidence for the 64-bit
row addressing, since those volumes (2.4 GB of u8, 4.8 GB of u16 per direction) lie past 2^31 and
2^32 bytes.  One process on the GPU, nothing beside it.  One JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PERDIR = 4096


def frame_pair(H, W, D, seed):
    """Banded constant-shift pair (tests/deepd_cases.py) with shifts spread over [5, D - 3]."""
    from stereo_match_amd import synthetic

    rng = np.random.default_rng(seed)
    shifts = [5, D // 3, (2 * D) // 3, D - 3]
    base = np.clip(synthetic._smooth3(rng.integers(0, 256, (H, W + D)).astype(np.float64)), 0, 255).astype(np.uint8)
    left = np.ascontiguousarray(base[:, :W])
    right = np.empty_like(left)
    for b, s in enumerate(shifts):
        y0, y1 = b * H // 4, (b + 1) * H // 4
        right[y0:y1] = base[y0:y1, s:s + W]
    return left, right


def params(kind, D):
    from stereo_match_amd import synthetic

    p = synthetic.headline_params(D) if kind == "census8" else dict(synthetic.parity_params(D), mode=8)
    return p


def main():
    import torch

    from stereo_match_amd import _lib, synthetic

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--label", default="branch")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deepd_bench needs the GPU: a CPU run gives no time")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(kw) + "\n")

    eng = _lib.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    base_cell = {}  # (kind, n) -> ns per pixel x disparity x path of the D = 256 baseline

    def point(H, W, D, kind, n, flags=0):
        pairs = [frame_pair(H, W, D, 11 + i) for i in range(n)]
        tl = torch.tensor(np.stack([a for a, _ in pairs]), device="cuda")
        tr = torch.tensor(np.stack([b for _, b in pairs]), device="cuda")
        out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        sp = synthetic.to_sm_params(params(kind, D))
        eng.set_debug_flags(flags)

        def call():
            eng.compute_batch_device(tl.data_ptr(), tr.data_ptr(), n, H * W, H, W, W, sp, out.data_ptr())

        try:
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            eng.set_timing(True)
            eng.reset_timing()
            call()
            eng.synchronize()
            split = {k: round(v[0] * 1e3 / n, 1) for k, v in eng.timing().items() if v[1]}
            eng.set_timing(False)
        finally:
            eng.set_debug_flags(0)
        us = float(np.median(ms)) * 1e3 / n
        width1 = W - D
        cell = us * 1e3 / (H * width1 * D * 8)  # ns per pixel x disparity x path
        if D == 256:
            base_cell[(kind, n, W)] = cell
        rel = cell / base_cell[(kind, n, W)] if (kind, n, W) in base_cell else None
        emit(what="matcher", label=args.label, W=W, H=H, D=D, kind=kind, pairs=n, flags=flags, us_per_pair=round(us, 1),
             us_per_pair_min=round(min(ms) * 1e3 / n, 1), us_per_pair_max=round(max(ms) * 1e3 / n, 1), reps=args.reps,
             ns_per_cell_path=round(cell, 5), cell_cost_vs_d256_perdir=None if rel is None else round(rel, 3),
             stage_us_per_pair=split)
        res = out[0].cpu().numpy() if args.check else None
        del tl, tr, out
        torch.cuda.empty_cache()
        return pairs[0], res

    H, W = 1988, 2880
    for kind in ("census8", "sgbm8"):
        for n in (1, 4):
            point(H, W, 256, kind, n, PERDIR)
    if not args.baseline_only:
        for kind in ("census8", "sgbm8"):
            for D in (272, 384, 512):
                for n in (1, 4):
                    (a, b), got = point(H, W, D, kind, n)
                    if args.check and D == 512 and n == 1:
                        from oracle import ref_c

                        ref = ref_c.compute(a, b, params(kind, D))
                        valid = ref >= 0
                        emit(what="check", label=args.label, W=W, H=H, D=D, kind=kind, exact=bool(np.array_equal(got, ref)),
                             differing_px=int((got != ref).sum()), valid_fraction=round(float(valid.mean()), 4),
                             valid_on_planes_ge_256=round(float((ref[valid] >= 256 * 16).mean()), 4))
        for kind in ("census8", "sgbm8"):
            point(375, 1242, 256, kind, 1, PERDIR)
            point(375, 1242, 272, kind, 1)
    eng.close()


if __name__ == "__main__":
    main()

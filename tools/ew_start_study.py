#!/usr/bin/env python3
"""CPU study of the start state of the in-sweep E/W strip segments.

A strip's E (W) segment starts w columns before (after) its strip from a start state and runs
the SGM recurrence into the strip; the patch pass repairs it where its min-0 state entering the
strip differs from the true path's.  This script measures that share of (row, boundary)
segments for the zero start and for the cost-derived start

    G(d) = min(K * (A(d) - min_d A), P2),   A = sum of the n cost columns before the first
                                            warmup column in the line's direction,

over start states x warmups x both directions, for the census and the SGBM costs of the
bench's KITTI-sized random-dot pairs.  numpy only (oracle.sgm_np's recurrence step); writes
profiles/ewstart/study.json.

    python tools/ew_start_study.py [--seeds 1003] [--rows 150:199] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import sgm_np  # noqa: E402
from stereo_match_amd import synthetic  # noqa: E402

CW = 36       # own columns per strip of the wide KITTI instances
MARGIN = 8    # image rows kept around the studied rows (census window, box sum, prefilter)


def start_state(C, c0, cs, n, K, P2):
    """G for lines whose first warmup column is c0 and that advance by cs: [rows, D].
    Zero where a guess column falls outside [0, W1) (the kernel's rule) or n == 0."""
    rows, W1, D = C.shape
    cols = [c0 - cs * i for i in range(1, n + 1)]
    if n == 0 or min(cols) < 0 or max(cols) >= W1:
        return np.zeros((rows, D), np.int64)
    A = C[:, cols, :].sum(axis=1)
    return np.minimum(K * (A - A.min(-1, keepdims=True)), P2)


def true_states(C, cs, P1, P2):
    """min-0 state of the whole-row path after every column: [rows, W1, D]."""
    rows, W1, D = C.shape
    out = np.empty_like(C)
    Lp = np.zeros((rows, D), np.int64)
    mp = np.zeros(rows, np.int64)
    for x in (range(W1) if cs > 0 else range(W1 - 1, -1, -1)):
        Lp, mp = sgm_np._step(C[:, x], Lp, mp, P1, P2)
        out[:, x] = Lp - mp[:, None]
    return out


def mismatch(C, T, cs, w, n, K, P1, P2, cw=CW):
    """Share of (row, interior boundary) segments of direction cs whose state entering their
    strip differs from the true one T (true_states); also the number of segments."""
    rows, W1, D = C.shape
    bad = tot = 0
    for k in range((W1 + cw - 1) // cw):
        x0 = k * cw
        c0 = x0 - w if cs > 0 else x0 + cw - 1 + w   # first warmup column
        last = c0 + cs * (w - 1)                     # the column before the strip
        if c0 < 0 or c0 >= W1:
            continue  # enters from outside the domain: the zero state there is the true one
        Lp = start_state(C, c0, cs, n, K, P2)
        mp = np.zeros(rows, np.int64)
        for j in range(w):
            Lp, mp = sgm_np._step(C[:, c0 + cs * j], Lp, mp, P1, P2)
        bad += int(((Lp - mp[:, None]) != T[:, last]).any(-1).sum())
        tot += rows
    return (bad / tot if tot else 0.0), tot


def costs(seed, r0, r1, mode, blur=False):
    H, W, D = synthetic.CONFIGS["kitti"]
    left, right, _ = synthetic.random_dot_pair(H, W, D, seed)
    if blur:  # a low-contrast variant: 5 more box passes, contrast / 4
        def soft(a):
            a = a.astype(np.float64)
            for _ in range(5):
                a = synthetic._smooth3(a)
            return np.clip(96 + (a - 128) / 4, 0, 255).astype(np.uint8)
        left, right = soft(left), soft(right)
    p = synthetic.headline_params(D) if mode == "census" else synthetic.parity_params(D)
    prm = sgm_np.normalize_params(p)
    a, b = max(0, r0 - MARGIN), min(H, r1 + MARGIN)
    C = sgm_np.cost_volume(left[a:b], right[a:b], prm)[r0 - a:r0 - a + (r1 - r0)]
    return np.ascontiguousarray(C), prm["P1"], prm["P2"]


STARTS = [("zero", 0, 0), ("K16n1", 16, 1), ("K16n2", 16, 2), ("K8n2", 8, 2), ("K8n3", 8, 3), ("K8n4", 8, 4),
          ("K4n4", 4, 4), ("K16n4", 16, 4)]
WARMUPS = (6, 9, 12, 18)


def study(seed, r0, r1, mode, blur=False, starts=STARTS, warmups=WARMUPS):
    C, P1, P2 = costs(seed, r0, r1, mode, blur)
    out = {"seed": seed, "rows": [r0, r1], "cost": mode, "blur": blur, "P1": P1, "P2": P2, "cw": CW, "cells": {}}
    for dname, cs in (("E", 1), ("W", -1)):
        T = true_states(C, cs, P1, P2)
        for name, K, n in starts:
            for w in warmups:
                f, tot = mismatch(C, T, cs, w, n, K, P1, P2)
                out["cells"][f"{dname}/{name}/w{w}"] = round(f, 4)
                out["segments"] = tot
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="1003")
    ap.add_argument("--rows", default="150:199")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ewstart", "study.json"))
    ap.add_argument("--no-blur", action="store_true")
    args = ap.parse_args()
    r0, r1 = (int(v) for v in args.rows.split(":"))
    res = []
    for seed in (int(s) for s in args.seeds.split(",")):
        for mode in ("census", "sgbm"):
            for blur in ((False,) if args.no_blur or mode == "sgbm" else (False, True)):
                r = study(seed, r0, r1, mode, blur)
                res.append(r)
                print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ew_start_study.py", "G": "min(K * (A - min A), P2), A = sum of n columns",
                   "figure": "share of (row, boundary) segments whose min-0 entering state differs from the true path's",
                   "runs": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

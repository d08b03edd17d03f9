"""Inputs of test_highcost_oracle.py and test_gpu_highcost.py: image pairs and cost volumes that
drive the SGM path sums to the top of the packed u16 range (a 5-path partial
that saturates at 0xFFFF, a full sum that clamps at 32767), the parameter sets around the two
dispatch boundaries of `path_max` (13107 / 13108: row bands and the atomic E/W patch; 16383 /
16384: the fast path and sm_wide.hpp), and a meter that says how much of an input really gets
there.  No GPU here: everything is numpy and the oracles."""
import functools

import numpy as np

from oracle import sgm_np
from stereo_match_amd import synthetic

MAX_S = 32767  # the WTA's clamp of a full sum
MAX_U16 = 65535  # where the packed u16 partial saturates

# name: (blockSize, P1, P2, path_max); preFilterCap 63 (ftzero 63): side^2 * 189 + P2
SETS = {
    "ATOM_TOP": (7, 100, 3846, 13107),  # last value with row bands and the atomic E/W patch
    "SAT_BOTTOM": (7, 100, 3847, 13108),  # first value without
    "FAST_TOP": (7, 100, 7122, 16383),  # top of the fast path
    "WIDE_BOTTOM": (7, 100, 7123, 16384),  # first value on sm_wide.hpp
    "FLAT_TOP": (7, 7121, 7122, 16383),  # P2 = P1 + 1
    "BS9": (9, 8, 1074, 16383),  # most pixels all-saturated, hence invalid
    "BS3": (3, 10, 14500, 16201),  # small C, huge P2
}
FAST_SETS = [k for k in SETS if k != "WIDE_BOTTOM"]

# (uniquenessRatio, disp12MaxDiff): the WLS factory's left matcher, and an ordinary matcher
VARIANTS = {"open": (0, 1000000), "strict": (10, 1)}

# external cost volumes (VOL_CMAX 4095): (P1, P2); P2 = 12288 reaches L = 16383
VOLUME_SETS = {"P12288_100": (100, 12288), "P12288_flat": (12287, 12288), "P9000": (4000, 9000)}
VOLUME_LO = (2500, 3300)

INPUTS = ("saw", "mixed40", "mixed150")


def path_max(name):
    bs, _, P2, pm = SETS[name]
    assert bs * bs * (2 * 63 + 63) + P2 == pm
    return pm


def params(name, D, mode=5, minD=0, variant="open"):
    bs, P1, P2, _ = SETS[name]
    uniq, d12 = VARIANTS[variant]
    return dict(synthetic.parity_params(D), blockSize=bs, P1=P1, P2=P2, preFilterCap=63, mode=mode,
                minDisparity=minD, uniquenessRatio=uniq, disp12MaxDiff=d12)


def volume_params(name, D, mode=8, **kw):
    P1, P2 = VOLUME_SETS[name]
    return dict(synthetic.cost_volume_params(D), P1=P1, P2=P2, mode=mode, **kw)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def saw(H, W, seed=1):
    """Opposing sawtooth gradients (period 32 columns) plus a little noise: the prefiltered BT cost
    sits at its maximum nearly everywhere."""
    rng = np.random.default_rng(seed)
    ramp = 8 * (np.arange(W, dtype=np.int64) % 32)[None, :]
    left = ramp + rng.integers(0, 6, (H, W))
    right = 255 - ramp + rng.integers(0, 6, (H, W)) - 6
    return _ro(np.clip(left, 0, 255).astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def mixed(H, W, D, stripe, seed=1):
    """saw() with every second stripe of `stripe` columns taken from a random-dot pair: saturated
    and ordinary cells alternate along every E/W line and every diagonal."""
    left, right = (a.copy() for a in saw(H, W, seed))
    dl, dr, _ = synthetic.random_dot_pair(H, W, D, seed)
    dots = (np.arange(W) // stripe) % 2 == 1
    left[:, dots] = dl[:, dots]
    right[:, dots] = dr[:, dots]
    return _ro(left, right)


@functools.lru_cache(maxsize=None)
def saw_bands(H, W, seed=1, band=200):
    """saw() with the noise taken out of every second band of `band` columns (wider than any strip):
    there every column is constant down the rows and the saturated costs repeat with the ramp's
    period, nothing makes a path forget its state, and a repaired E/W walk does not meet the
    speculative one before its strip ends."""
    left, right = (a.copy() for a in saw(H, W, seed))
    ramp = 8 * (np.arange(W, dtype=np.int64) % 32)
    clean = (np.arange(W) // band) % 2 == 0
    left[:, clean] = np.clip(ramp, 0, 255).astype(np.uint8)[clean]
    right[:, clean] = np.clip(255 - ramp - 3, 0, 255).astype(np.uint8)[clean]
    return _ro(left, right)


def pair(name, H, W, D, seed=1):
    if name == "saw":
        return saw(H, W, seed)
    if name == "saw_bands":
        return saw_bands(H, W, seed)
    return mixed(H, W, D, int(name[len("mixed"):]), seed)


@functools.lru_cache(maxsize=None)
def high_volume(D, H, W, lo, seed=1):
    """float32 [D, H, W] of integers in [lo, 4095]; per column one cheaper plane d = 8 + 4 sin(x / 9),
    lowered by a random 0..1999, so that some pixels keep a winner.  For offset 0, scale 1."""
    rng = np.random.default_rng(seed)
    vol = rng.integers(lo, 4096, (D, H, W)).astype(np.float32)
    xs = np.arange(W)
    d = np.clip(np.rint(8 + 4 * np.sin(xs / 9.0)).astype(np.int64), 0, D - 1)
    vol[d, :, xs] -= rng.integers(0, 2000, (W, H)).astype(np.float32)
    return _ro(vol)[0]


DIRS_5 = [(1, 0), (-1, 0), (1, 1), (0, 1), (-1, 1)]  # E, W, SE, S, SW: the down sweep's partial
DIRS_UP = [(1, -1), (0, -1), (-1, -1)]  # NE, N, NW
# engine direction order of debug_fetch(1) (tests/test_gpu_parity.py test_path_volumes_match_oracle)
ENGINE_DIRS = DIRS_5 + DIRS_UP


def coverage(C, P1, P2, mode, disp=None, minD=0):
    """How far the cost volume C [H, width1, D] (the numpy oracle's) drives the u16 arithmetic:
      max_L     the largest path value of any direction;
      sat5      share of cells whose five-path sum (E, W, SE, S, SW) is >= 65535;
      sat_full  share of cells whose full sum (5 or 8 paths) is >= 65535;
      mid       share of cells whose full sum lies in (32767, 65535): clamped by the WTA, not saturated;
      all_sat   share of pixels whose every S is >= 32767 (no winner);
      valid     share of the in-domain pixels that `disp` leaves valid (the oracle's full [H, W] map
                of the same input; its domain is columns [minX1, minX1 + width1)); None without."""
    H, width1, D = C.shape
    s5 = np.zeros_like(C)
    max_L = 0
    for d in DIRS_5:
        L = sgm_np.aggregate_path(C, d, P1, P2)
        max_L = max(max_L, int(L.max()))
        s5 += L
    full = s5.copy()
    if mode == 8:
        for d in DIRS_UP:
            L = sgm_np.aggregate_path(C, d, P1, P2)
            max_L = max(max_L, int(L.max()))
            full += L
    out = dict(max_L=max_L, sat5=float(np.mean(s5 >= MAX_U16)), sat_full=float(np.mean(full >= MAX_U16)),
               mid=float(np.mean((full > MAX_S) & (full < MAX_U16))),
               all_sat=float(np.mean(full.min(-1) >= MAX_S)), valid=None)
    if disp is not None:
        out["valid"] = valid_share(disp, width1, D, minD)
    return out


def image_coverage(left, right, p):
    """coverage() of an image pair under the oracle-style params p, with the C oracle's map."""
    from oracle import ref_c

    prm = sgm_np.normalize_params(p)
    C = sgm_np.cost_volume(left, right, prm)
    return coverage(C, prm["P1"], prm["P2"], prm["mode"], ref_c.compute(left, right, p), prm["minD"])


def volume_coverage(vol, p):
    from oracle import ref_c

    prm = sgm_np.normalize_params(dict(p, cost=2))
    C = sgm_np.quantize_volume(vol, prm, 0.0, 1.0)
    return coverage(C, prm["P1"], prm["P2"], prm["mode"], ref_c.compute_volume(vol, p, 0.0, 1.0), prm["minD"])


# every `mixed` input the GPU tests use, (stripe, H, W, D, seed): test_highcost_oracle.py holds each
# to the coverage floors under FAST_TOP, so a GPU test that takes another one has to add it here
SHAPES = [(23, 3 * D + 257, D) for D in (16, 64, 128)]
FLOOR_INPUTS = ([(stripe, H, W, D, 1) for stripe in (40, 150) for H, W, D in SHAPES + [(23, 600, 256)]] +
                [(40, 40, 200, 32, 1), (40, 50, 320, 64, 1)] +
                [(150, H, W, D, seed) for W, D in ((449, 64), (641, 128)) for H in (23, 50) for seed in (2, 3, 4)] +
                [(150, 50, 449, 64, 1), (150, 50, 641, 128, 1)] + [(150, 23, 353, 32, seed) for seed in (1, 2, 3, 4)])

# the floors (conditions on the inputs, not measurements; the shares measured on the CPU are in
# DESIGN.md §3)
FLOOR_SAT5 = 0.02  # cells whose five-path sum is >= 65535
FLOOR_MID = 0.25  # cells whose full sum lies in (32767, 65535)
FLOOR_MAX_L = 15000
FLOOR_VALID = {"strict": 0.25, "open": 0.75}
FLOOR_ALL_SAT_8 = 0.03  # 8 paths: pixels whose every S is >= 32767
FLOOR_VOLUME_SAT = 0.10  # P2 = 12288 volumes: cells whose sum is >= 65535 (and largest L == 16383)


def valid_share(disp, width1, D, minD=0):
    minX1 = max(minD + D, 0)
    return float(np.mean(disp[:, minX1:minX1 + width1] >= minD * 16))


def assert_floors(stripe, H, W, D, seed, mode):
    """The floors of one `mixed` input at FAST_TOP; returns the coverage (its `valid` is the strict
    variant's share) and the open variant's valid share."""
    from oracle import ref_c

    left, right = mixed(H, W, D, stripe, seed)
    cs = image_coverage(left, right, params("FAST_TOP", D, mode, 0, "strict"))
    vo = valid_share(ref_c.compute(left, right, params("FAST_TOP", D, mode, 0, "open")), W - D, D)
    assert cs["sat5"] >= FLOOR_SAT5, cs
    assert cs["mid"] >= FLOOR_MID, cs
    assert cs["max_L"] >= FLOOR_MAX_L, cs
    assert cs["valid"] >= FLOOR_VALID["strict"], cs
    assert vo >= FLOOR_VALID["open"], vo
    if mode == 8:
        assert cs["all_sat"] >= FLOOR_ALL_SAT_8, cs
    return cs, vo

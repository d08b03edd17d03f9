"""Inputs and oracle results of the numDisparities 272..512 tests (no device).

synthetic.random_dot_pair puts almost no winner above plane 256 at the frame sizes a quick test
can afford, so the pairs here are banded constant-shift pairs: the rows fall into len(shifts)
bands, and band b of the right image is the left image's base shifted by shifts[b], i.e. a
constant disparity per band, two of the four at or above plane 250 and 258.  The oracle results
are computed once per case (ref_c: oracle/sgm_ref.c) and left unchanged."""
import functools

import numpy as np

from oracle import ref_c, sgm_np, wls_np
from stereo_match_amd import synthetic

H_IMG, H_VOL = 24, 16
# (numDisparities, minDisparity): both ends of the range, values that are and are not multiples
# of 64 (sm_deep.hpp: 17..32 disparities per lane, odd and even), a negative and a positive minD
RANGES = [(272, 0), (320, 0), (496, 0), (512, 0), (288, -7), (384, 3)]
KINDS = ["census8", "census5", "sgbm5", "sgbm8"]
IMAGE_CASES = [(D, minD, kind) for D, minD in RANGES for kind in KINDS]
# (planes, shifts): 257 pads to 272, 300 to 304, 512 is the largest
VOLUME_CASES = [(257, (5, 250, 256, 256)), (300, (5, 250, 258, 297)), (512, (5, 250, 258, 509))]
# coverage the oracle's own maps must reach, so that no GPU comparison passes vacuously (both
# below the minima measured over the cases: 18.1 % and 40.7 %)
MIN_VALID, MIN_DEEP = 0.15, 0.35


def params(kind: str, D: int, minD: int = 0, **kw) -> dict:
    base = synthetic.headline_params(D) if kind.startswith("census") else synthetic.parity_params(D)
    return dict(base, mode=int(kind[-1]), minDisparity=minD, **kw)


def key(p: dict):
    return tuple(sorted(p.items()))


def shifts_for(D: int, minD: int):
    return (max(minD + 5, 5), minD + 250, minD + 258, minD + D - 3)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def banded_pair(H: int, W: int, shifts: tuple, seed: int):
    """left = base[:, :W]; row y of right = base[y, s:s + W], s = shifts[y * len(shifts) // H]."""
    rng = np.random.default_rng(seed)
    smax = max(shifts)
    base = np.clip(synthetic._smooth3(rng.integers(0, 256, (H, W + smax)).astype(np.float64)), 0, 255).astype(np.uint8)
    left = np.ascontiguousarray(base[:, :W])
    right = np.empty_like(left)
    for y in range(H):
        s = shifts[y * len(shifts) // H]
        right[y] = base[y, s:s + W]
    return _frozen(left, right)


def image_pair(D: int, minD: int, seed: int = 5, H: int = H_IMG):
    return banded_pair(H, D + 150, shifts_for(D, minD), seed)


@functools.lru_cache(maxsize=None)
def expected_wta(D: int, minD: int, kind: str, seed: int = 5, extra=()):
    """(disparity, integer WTA index) of ref_c.compute_wta."""
    a, b = image_pair(D, minD, seed)
    return _frozen(*ref_c.compute_wta(a, b, params(kind, D, minD, **dict(extra))))


@functools.lru_cache(maxsize=None)
def expected(D: int, minD: int, kind: str, seed: int = 5, extra=()):
    a, b = image_pair(D, minD, seed)
    return _frozen(ref_c.compute(a, b, params(kind, D, minD, **dict(extra))))


def volume_params(Dv: int) -> dict:
    return synthetic.cost_volume_params(Dv)


VOL_OFFSET, VOL_SCALE = 0.0, 4095.0


@functools.lru_cache(maxsize=None)
def volume(Dv: int, shifts: tuple):
    a, b = banded_pair(H_VOL, Dv + 150, shifts, 6)
    return _frozen(synthetic.absdiff_volume(a, b, Dv))


@functools.lru_cache(maxsize=None)
def expected_volume(Dv: int, shifts: tuple):
    return _frozen(ref_c.compute_volume(volume(Dv, shifts), volume_params(Dv), VOL_OFFSET, VOL_SCALE))


def coverage(disp: np.ndarray, minD: int):
    """(valid fraction of the frame, fraction of the valid pixels on planes >= 256)."""
    valid = disp >= minD * 16
    nv = int(valid.sum())
    deep = int((disp[valid] >= (minD + 256) * 16).sum())
    return nv / disp.size, (deep / nv if nv else 0.0)


@functools.lru_cache(maxsize=None)
def lr_maps(D: int, minD: int, kind: str, seeds: tuple):
    """(displ, dispr) as compute_disparity makes them (tests/strided.py lr_maps)."""
    s = params(kind, D, minD)
    lp = dict(s, uniquenessRatio=0, disp12MaxDiff=1000000, speckleWindowSize=0)
    rp = sgm_np.right_matcher_params(s)
    src = [image_pair(D, minD, sd) for sd in seeds]
    dl = ref_c.compute_many(src, lp)
    dr = ref_c.compute_many([(b, a) for a, b in src], rp)
    return tuple(_frozen(o) for o in dl), tuple(_frozen(o) for o in dr)


@functools.lru_cache(maxsize=None)
def expected_wls(D: int, minD: int, kind: str, seeds: tuple, wkey):
    dl, dr = lr_maps(D, minD, kind, seeds)
    return tuple(_frozen(wls_np.wls_filter(dl[i], image_pair(D, minD, sd)[0], dr[i], dict(wkey)))
                 for i, sd in enumerate(seeds))

"""Case tables of test_bm_cases_oracle.py and test_gpu_bm_configs.py (no device here: numpy and
oracle/bm_np.py only).

k_bm_sad (csrc/sm_bm.hpp) runs in one of four configurations, picked by run_bm (csrc/sm_api.hip)
from (numDisparities, blockSize): the strip width SWs in {64, 32, 16, 8}, which fixes the lanes
per pixel of the WTA (256 / SWs) and how many thread groups share a sliding sum.  STRIP_CASES
reaches each of them, both sides of the boundaries between them, and the pairs run_bm refuses.
The other tables reach rofs > 0, the sub-pixel end mirrors, SADs that fill the 23 bits of the WTA
key, and batches past the launch group.  Oracle results are computed once per case and frozen."""
import collections
import functools

import numpy as np

from oracle import bm_np
from stereo_match_amd import synthetic

SEED = 5
MIN_MARGIN = 40  # W >= D + blockSize + MIN_MARGIN where a row's size is ours to choose


def strip_width(D: int, blockSize: int) -> int:
    """The strip width run_bm (csrc/sm_api.hip) picks: the largest of 64 / 32 / 16 / 8 whose
    dynamic LDS (vsum [NC][D], sad [SWs][D], vtex [NC], tsum [SWs] as int; two staged rows of both
    views as bytes; 16 spare) fits in 64 KiB, NC = SWs + blockSize - 1.  0: SM_E_UNSUPPORTED."""
    for c in (64, 32, 16, 8):
        NC = c + 2 * (blockSize // 2)
        if (NC * D + c * D + NC + c) * 4 + 2 * (2 * NC + D) + 16 <= 65536:
            return c
    return 0


# uniq_b: the uniquenessRatio of parameter set B, chosen per row so that the oracle keeps and
# filters at least MIN_MIXED of the ROI each (test_bm_cases_oracle.py checks it).
# narrow: the (16, 255) row at W = 285, whose ROI of 16 columns is one partial strip and nothing
# else; its W = 345 sibling has a whole strip and a partial last one.
StripCase = collections.namedtuple("StripCase", "H W D bs minD sws uniq_b narrow", defaults=(False,))


def _smallest(D, bs, rows=2):
    """Smallest (H, W) with H > bs and W >= D + bs + MIN_MARGIN: an ROI of 42 columns, wider than
    a strip of 32 / 16 / 8 and a multiple of none, and of `rows` rows.  Two rows are enough for a
    small block; under a block of 63 and more the map is so smooth that it takes TALL rows of the
    slanted plane to reach MIN_DISTINCT values (which also makes a second band of 64 rows)."""
    return bs + rows - 1, D + bs + MIN_MARGIN


TALL = 80


def _row(D, bs, sws, uniq_b, H=None, W=None, minD=0, narrow=False, rows=2):
    h, w = _smallest(D, bs, rows)
    return StripCase(H or h, W or w, D, bs, minD, sws, uniq_b, narrow)


STRIP_CASES = [
    # SWs = 64
    _row(112, 15, 64, 2, 30, 200),  # the last blockSize of D = 112 on 64
    _row(16, 255, 64, 2, 262, 285, narrow=True),
    _row(16, 255, 64, 3, 262, 345),
    _row(96, 9, 64, 2, 40, 190),
    # SWs = 32
    _row(112, 17, 32, 2, 30, 200),  # the other side of (112, 15)
    _row(128, 5, 32, 2, 30, 200),
    _row(128, 21, 32, 2, 40, 220),
    _row(160, 15, 32, 2, 30, 250),
    _row(160, 15, 32, 2, 30, 250, minD=-5),
    _row(144, 7, 32, 2, 30, 230),
    _row(224, 9, 32, 2),  # the last blockSize of D = 224 on 32
    # SWs = 16
    _row(256, 5, 16, 2, 24, 330),
    _row(256, 5, 16, 2, 72, 330),  # ROI of 68 rows: two bands of 64
    _row(240, 11, 16, 2, 30, 280),
    _row(224, 11, 16, 2, 30, 300),  # the other side of (224, 9)
    _row(128, 63, 16, 2, rows=TALL),
    _row(256, 31, 16, 2, 60, 330),  # the last blockSize of D = 256 on 16
    # SWs = 8
    _row(256, 47, 8, 2, 60, 340),  # the last blockSize of D = 256 that runs
    _row(256, 33, 8, 2, 60, 330),  # the other side of (256, 31)
    _row(160, 71, 8, 2, rows=TALL),
    _row(128, 95, 8, 2, rows=TALL),
    _row(160, 85, 8, 2, rows=TALL),  # the running neighbours of the refused rows
    _row(128, 109, 8, 2, 209, 345),
    # refused
    _row(256, 49, 0, 0, 62, 345),
    _row(128, 111, 0, 0),
    _row(160, 87, 0, 0),
]
RUNNING = [c for c in STRIP_CASES if c.sws]
REFUSED = [c for c in STRIP_CASES if not c.sws]
SETS = ("A", "B", "C")
MIN_MIXED = 0.05  # set B: share of the ROI kept, and filtered, at least
MIN_KEPT_C = 0.5
MIN_DISTINCT, MIN_DISTINCT_WIDE = 40, 3  # set A; the latter where blockSize >= 129


def case_id(c) -> str:
    return f"H{c.H}W{c.W}D{c.D}bs{c.bs}m{c.minD}"


def running_neighbour(c: StripCase) -> StripCase:
    """The running row with c's numDisparities and the next smaller blockSize."""
    return max((r for r in RUNNING if r.D == c.D and r.bs < c.bs), key=lambda r: r.bs)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def base_params(c, **kw) -> dict:
    return dict(numDisparities=c.D, blockSize=c.bs, minDisparity=c.minD, **kw)


def strip_inputs(c: StripCase, which: str):
    """(left, right, params) of parameter set A, B or C of a row."""
    left, right = pair(c.H, c.W, c.D)
    a = base_params(c, textureThreshold=0, uniquenessRatio=0, disp12MaxDiff=-1)
    if which == "A":
        return left, right, a
    if which == "B":
        return left, right, base_params(c, textureThreshold=0, uniquenessRatio=c.uniq_b, disp12MaxDiff=1)
    assert which == "C"
    return right, left, bm_np.right_matcher_params(a)


@functools.lru_cache(maxsize=None)
def pair(H, W, D, seed=SEED):
    left, right, _ = synthetic.random_dot_pair(H, W, D, seed=seed)
    return _frozen(left, right)


def key(p: dict):
    return tuple(sorted(p.items()))


@functools.lru_cache(maxsize=None)
def _bm(left_bytes, right_bytes, shape, pkey, cost):
    left = np.frombuffer(left_bytes, np.uint8).reshape(shape)
    right = np.frombuffer(right_bytes, np.uint8).reshape(shape)
    out = bm_np.stereo_bm(left, right, dict(pkey), return_cost=cost)
    return _frozen(*out) if cost else _frozen(out)


def oracle(left, right, p: dict, return_cost=False):
    """bm_np.stereo_bm, computed once per (images, parameters) and read-only."""
    return _bm(left.tobytes(), right.tobytes(), left.shape, key(p), return_cost)


def expected_strip(c: StripCase, which: str):
    left, right, p = strip_inputs(c, which)
    return oracle(left, right, p)


def roi_of(disp, p: dict):
    """The valid-disparity ROI of a map (a view), and FILTERED."""
    q = bm_np.normalize_bm(p)
    x, y, w, h = bm_np.valid_roi(disp.shape[0], disp.shape[1], q)
    return disp[y:y + h, x:x + w], (q["minDisparity"] - 1) * 16


# ---- rofs > 0 (minDisparity < -(D - 1)) and frames with no region at all ------------------------
RangeCase = collections.namedtuple("RangeCase", "H W D bs minD extra")
_RANGE_P = dict(textureThreshold=0, uniquenessRatio=2, disp12MaxDiff=1)
RANGE_CASES = [
    RangeCase(20, 90, 16, 5, -19, _RANGE_P),
    RangeCase(26, 120, 32, 7, -40, _RANGE_P),
    RangeCase(24, 330, 256, 5, -260, _RANGE_P),
    RangeCase(24, 330, 256, 5, -260, dict(textureThreshold=0, uniquenessRatio=0, disp12MaxDiff=-1)),
    # too narrow for any region (W - blockSize + 1 < numDisparities): FILTERED everywhere
    RangeCase(20, 40, 64, 9, 0, dict(speckleWindowSize=10, speckleRange=16)),
    RangeCase(20, 40, 64, 9, -70, dict(speckleWindowSize=10, speckleRange=16, disp12MaxDiff=1)),
]


def range_inputs(c: RangeCase):
    left, right = pair(c.H, c.W, c.D)
    return left, right, dict(numDisparities=c.D, blockSize=c.bs, minDisparity=c.minD, **c.extra)


# ---- the sub-pixel end mirrors: constant-shift pairs whose winner is index 0 or ndisp - 1 --------
ShiftCase = collections.namedtuple("ShiftCase", "H W D bs minD shift mind sws")
SHIFT_CASES = [ShiftCase(H, 330, 256, bs, minD, minD + (255 if mind == 0 else 0), mind, sws)
               for H, bs, sws in ((24, 5, 16), (60, 33, 8)) for minD in (0, 3) for mind in (0, 255)]
MIN_SHIFT_HIT = 0.9


def shift_inputs(c: ShiftCase):
    left, right = synthetic.shifted_pair(c.H, c.W, c.shift, seed=SEED)
    return left, right, dict(numDisparities=c.D, blockSize=c.bs, minDisparity=c.minD)


# ---- SADs above 2^22: the WTA key keeps 23 bits of SAD above 9 bits of index ---------------------
HIGH_SAD = dict(H=262, W=300, D=16, bs=255)
HIGH_SAD_UNIQ = (0, 100)  # minsad * 100 < 2^31; ratios above 262 would overflow int, as in OpenCV


@functools.lru_cache(maxsize=None)
def high_sad_pair():
    """Opposed sawtooth rows, (8x) mod 256 against 255 - (8x) mod 256: after the X-Sobel prefilter
    with preFilterCap 63 nearly every pixel differs by the full 126."""
    H, W = HIGH_SAD["H"], HIGH_SAD["W"]
    rng = np.random.default_rng(SEED)
    saw = (8 * np.arange(W)) % 256
    left = saw[None, :] + rng.integers(0, 3, (H, W))
    right = 255 - saw[None, :] + rng.integers(0, 3, (H, W))
    return _frozen(np.minimum(left, 255).astype(np.uint8), np.minimum(right, 255).astype(np.uint8))


def high_sad_inputs(uniq: int):
    left, right = high_sad_pair()
    return left, right, dict(numDisparities=HIGH_SAD["D"], blockSize=HIGH_SAD["bs"], preFilterCap=63,
                             textureThreshold=0, uniquenessRatio=uniq)


# ---- more pairs than one launch group (kMaxGroup = 16 in csrc/sm_api.hip) ------------------------
BATCH = dict(n=17, H=20, W=90, D=16, bs=5)
BATCH_PARAMS = dict(numDisparities=16, blockSize=5, disp12MaxDiff=1, speckleWindowSize=10, speckleRange=16)


def batch_pairs():
    return [pair(BATCH["H"], BATCH["W"], BATCH["D"], seed=100 + i) for i in range(BATCH["n"])]


# ---- validateDisparity on wide rows: W * 13 bytes of dynamic LDS per row -------------------------
VALIDATE_LDS_PER_COLUMN = 13
WIDE_OK = dict(H=12, W=5100, D=16, bs=5)  # 66,300 B: above 64 KiB
WIDE_REFUSED = dict(H=12, W=12700, D=16, bs=5)  # 165,100 B: above the CU's 163,840 B
WIDEST_VALIDATE = 163840 // VALIDATE_LDS_PER_COLUMN  # 12,603


def wide_inputs(shape: dict, d12: int):
    left, right = pair(shape["H"], shape["W"], shape["D"])
    return left, right, dict(numDisparities=shape["D"], blockSize=shape["bs"], textureThreshold=0,
                             uniquenessRatio=0, disp12MaxDiff=d12)

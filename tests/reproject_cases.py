"""Seeded inputs of test_reproject_oracle.py, test_gpu_reproject.py and the NaN cases of
test_gpu_pointcloud.py (no device here: numpy only).

k_disp_min (csrc/sm_reproject.hpp) runs at most 1024 blocks of 256 threads per map, so a map of
more than STEP = 256 * 1024 pixels is walked in a second grid-stride step; k_keys_to_float turns
64 maps' keys per block.  The maps below put their minimum, and their NaNs, where each of these
can go wrong: the first and the last pixel, a lane that is not its wave's lane 0, and the strided
tail of a map larger than STEP.  Every returned array is read-only and cached."""
import functools
import itertools

import numpy as np

EPS = np.float32(np.finfo(np.float32).eps)
BIG_Z = np.float32(10000.0)
STEP = 256 * 1024  # pixels k_disp_min sees in one grid-stride step

# ---- Q matrices
# disparity_calculation.py:293-298, under the two names the older test files use for it
Q_CALC = np.float32([[1, 0, 0, -640], [0, -1, 0, 360], [0, 0, 0, -1164], [0, 0, 1, 0]])
Q_REF = Q_CALC.copy()
# X overflows float32 alone; principal point x = 1, where d = 0 makes 0 * inf (test_gpu_pointcloud.py)
Q_IN = np.float32([[1e38, 0, 0, -1e38], [0, -1, 0, 7], [0, 0, 0, -50], [0, 0, 1, 0]])
# dense, float64, no entry float32-representable; the last row is kept away from 0 so that
# qw + Q32 * d is well conditioned on the random part of dense_map
Q_DENSE = np.random.default_rng(1234).standard_normal((4, 4))
Q_DENSE[3] = np.abs(Q_DENSE[3]) * [0.01, 0.01, 1, 1] + [0, 0, 0.5, 3]
assert not (Q_DENSE == Q_DENSE.astype(np.float32)).any()
# w = -x/2 + y/4 - 4 + d, every term exact in float64: d = 4 + x/2 - y/4 (zero_w_map) makes w
# exactly 0.  Then X = (x - 3) / 0, Y = (2 - y) / 0 (NaN in column 3 / row 2, else +-inf), Z = -50 / 0.
Q_ZERO = np.float64([[1, 0, 0, -3], [0, -1, 0, 2], [0, 0, 0, -50], [-0.5, 0.25, 1, -4]])
for _Q in (Q_CALC, Q_REF, Q_IN, Q_DENSE, Q_ZERO):
    _Q.setflags(write=False)


def nan32_bits(sign: int, payload: int = 0x400000) -> int:
    """Bit pattern of a float32 NaN: sign < 0 sets the sign bit; payload in [1, 0x7FFFFF] (the
    default 0x400000 is numpy's quiet NaN, anything below it a signalling one)."""
    assert 0 < payload <= 0x7FFFFF
    return (0x80000000 if sign < 0 else 0) | 0x7F800000 | payload


NAN_PAYLOADS = (0x400000, 0x400123, 0x000001, 0x7FFFFF)
QUIET_ONLY = (0x400000,)  # np.nan and its negative, nothing else


def put_nans(d: np.ndarray, flat_positions, sign: int, payloads=NAN_PAYLOADS) -> None:
    """NaNs of one sign and of cycling payloads, written as bits (no FP move touches them)."""
    bits = d.reshape(-1).view(np.uint32)
    for p, payload in zip(flat_positions, itertools.cycle(payloads)):
        bits[p] = nan32_bits(sign, payload)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- the shape grid
SHAPES = [(1, 1), (1, 255), (3, 256), (2, 257), (5, 513), (37, 53), (513, 512)]
assert SHAPES[-1][0] * SHAPES[-1][1] > STEP


def min_position(H: int, W: int) -> int:
    """Flat index of a grid map's unique minimum: the third pixel from the end (not a wave's lane
    0; behind STEP in the large map, so only k_disp_min's second step sees it)."""
    return max(H * W - 3, 0)


assert min_position(*SHAPES[-1]) >= STEP and min_position(*SHAPES[-1]) % 64 not in (0, 63)


@functools.lru_cache(maxsize=None)
def grid_map(H: int, W: int, kind: str, Qname: str = "calc"):
    """int16: uniform in [-16, 1500], -32768 (the unique minimum) at min_position, 32767 at the
    second pixel.  float32: uniform in [0, 100) with the unique minimum -7.25 at min_position.
    With Qname "dense" every 16th pixel of a float32 map is a cancellation pixel, d =
    float32(-qw / Q32): there qw + Q32 * d is ~2^-25 of its terms, and one rounding more or less
    in the float64 chain (FP contraction) reaches the float32 result."""
    rng = np.random.default_rng(1000 + 7 * H + W)
    n, mp = H * W, min_position(H, W)
    if kind == "s16":
        d = rng.integers(-16, 1501, (H, W)).astype(np.int16)
        if n > 1:
            d.flat[1] = 32767
        d.flat[mp] = -32768
        return _frozen(d)
    d = (rng.random((H, W)) * 100).astype(np.float32)
    if Qname == "dense":
        y, x = np.divmod(np.arange(n), W)
        qw = Q_DENSE[3, 1] * y + Q_DENSE[3, 3] + Q_DENSE[3, 0] * x
        sel = np.arange(n) % 16 == 5
        d.flat[sel] = (-qw[sel] / Q_DENSE[3, 2]).astype(np.float32)
    d.flat[mp] = -7.25 if Qname != "dense" else np.float32(d.min() - np.float32(7.25))
    return _frozen(d)


def Q_of(Qname: str):
    return {"calc": Q_CALC, "dense": Q_DENSE}[Qname]


# ---- special values (float32, handleMissingValues)
SPECIAL_SHAPE = (5, 70)  # 350 pixels: two blocks, six waves
FIRST, LAST, MID = 0, 5 * 70 - 1, 64 + 37  # MID: lane 37 of the second wave
SPECIAL_CASES = ("specials", "neg_inf", "all_nan", "pos_inf_only")


@functools.lru_cache(maxsize=None)
def special_map(case: str, nan_sign: int):
    """float32 SPECIAL_SHAPE maps, the NaNs of sign nan_sign (payloads cycling):

    specials      uniform [1, 50) with +0, -0, +-denormals and +inf; NaNs at FIRST, MID, LAST and
                  two more.  The minimum is the negative denormal -2^-149: it, the zeros and the
                  positive denormals (7 pixels) lie within FLT_EPSILON of it.
    neg_inf       the same with one -inf: the minimum, and `-inf - -inf` marks nothing.
    all_nan       no non-NaN pixel: no minimum, nothing marked.
    pos_inf_only  +inf and NaNs only: the minimum is +inf and `inf - inf` marks nothing."""
    H, W = SPECIAL_SHAPE
    rng = np.random.default_rng(77)
    d = (1 + 49 * rng.random((H, W))).astype(np.float32)
    f = d.reshape(-1)
    tiny = np.float32(2.0 ** -149)
    if case in ("specials", "neg_inf"):
        f[3], f[66], f[130] = 0.0, -0.0, 0.0
        f[7], f[200], f[261], f[300] = tiny, -tiny, np.float32(1e-39), np.float32(2.0 ** -127)
        f[11], f[257] = np.inf, np.inf
        if case == "neg_inf":
            f[150] = -np.inf
        put_nans(d, (FIRST, MID, LAST, 255, 256), nan_sign)
    elif case == "all_nan":
        put_nans(d, range(H * W), nan_sign)
    else:
        f[:] = np.inf
        put_nans(d, (FIRST, MID, LAST), nan_sign)
    return _frozen(d)


# pixels the oracle marks 10000 (written down, checked against the oracle on the CPU)
SPECIAL_MARKED = {"specials": (3, 7, 66, 130, 200, 261, 300), "neg_inf": (), "all_nan": (), "pos_inf_only": ()}

# ---- the FLT_EPSILON ladder around the minimum md, in float32:
#   md, nextafter(md, +inf), md + eps, nextafter(md + eps, +inf), md + 2 eps
# float32's spacing is 2^-149 at 0, eps / 2 just above -1 and 2 eps at 3.75 (where md + eps is a
# tie that rounds back to md, and its successor is md + 2 eps).
LADDER_MD = (0.0, -1.0, 3.75)
LADDER_AT = (9, 64 + 21, 100, 2, 128)  # the rungs' flat positions in a (3, 70) map
LADDER_FLAGS = {0.0: (True, True, True, False, False),    # 0, 2^-149, eps | eps's successor, 2 eps
                -1.0: (True, True, True, False, False),   # -1, + eps / 2, + eps | + 3 eps / 2, + 2 eps
                3.75: (True, False, True, False, False)}  # 3.75 twice | 3.75 + 2 eps three times


def ladder_values(md: float) -> np.ndarray:
    m = np.float32(md)
    inf = np.float32(np.inf)
    return np.array([m, np.nextafter(m, inf), m + EPS, np.nextafter(np.float32(m + EPS), inf), m + np.float32(2) * EPS],
                    np.float32)


@functools.lru_cache(maxsize=None)
def ladder_map(md: float, nan_sign: int):
    """(3, 70) float32: uniform in [md + 1, md + 50), the five rungs at LADDER_AT, NaNs at the
    first and the last pixel."""
    rng = np.random.default_rng(88)
    d = (np.float32(md) + 1 + 49 * rng.random((3, 70))).astype(np.float32)
    d.reshape(-1)[list(LADDER_AT)] = ladder_values(md)
    put_nans(d, (0, d.size - 1), nan_sign)
    return _frozen(d)


# ---- NaN and minimum at every pair of the hard positions
def position_cases():
    """(H, W, nan_at, min_at): each hard position once as the NaN's and once as the minimum's."""
    H, W = SPECIAL_SHAPE
    small = [(H, W, a, b) for a, b in ((FIRST, LAST), (LAST, MID), (MID, FIRST))]
    HB, WB = SHAPES[-1]
    tail = STEP + 300 + 37  # only the second grid-stride step; lane 17
    return small + [(HB, WB, tail, 5), (HB, WB, 5, tail)]


@functools.lru_cache(maxsize=None)
def position_map(H: int, W: int, nan_at: int, min_at: int, nan_sign: int):
    """float32, uniform in [1, 50), the minimum -2.5 at min_at, its float32 successor (2 eps above
    it: outside the window) beside it, one NaN at nan_at."""
    rng = np.random.default_rng(99)
    d = (1 + 49 * rng.random((H, W))).astype(np.float32)
    f = d.reshape(-1)
    f[min_at] = -2.5
    nb = min_at + 1 if min_at + 1 not in (nan_at, H * W) else min_at - 1
    f[nb] = np.nextafter(np.float32(-2.5), np.float32(0))
    put_nans(d, (nan_at,), nan_sign)
    return _frozen(d)


# ---- division by zero
@functools.lru_cache(maxsize=None)
def zero_w_map(kind: str):
    """((12, 20) map, the mask of its zero-w pixels).  d = 4 + x / 2 - y / 4 makes Q_ZERO's w
    exactly 0 and is an integer (so that an int16 map can hold it) where (2 x - y) % 4 == 0: x
    even in rows 0, 4, 8 and x odd in rows 2, 6, 10 -- among them column 3 (X = 0 * inf) and row 2
    (Y = 0 * inf).  Elsewhere uniform integers in [20, 60], where w >= 6.5."""
    H, W = 12, 20
    rng = np.random.default_rng(55)
    d = rng.integers(20, 61, (H, W)).astype(np.float64)
    y, x = np.mgrid[:H, :W]
    zero = (2 * x - y) % 4 == 0
    d[zero] = (4 + 0.5 * x - 0.25 * y)[zero]
    assert (d == np.round(d)).all() and zero[2, 3] and zero[0, 0]
    return _frozen(d.astype(np.int16 if kind == "s16" else np.float32)), _frozen(zero)

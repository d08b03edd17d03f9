"""CPU: oracle/reproject_np.py itself, on the inputs of tests/reproject_cases.py (no device).

* its two NaN rules (the oracle's docstring), which may depend on neither the
  sign nor the payload of a NaN, and the FLT_EPSILON window around the minimum;
* its float64 chain against exact rational arithmetic;
* that FP contraction of that chain would be seen in the float32 result of a map the GPU test runs."""
import fractions
import math

import numpy as np
import pytest

import reproject_cases as C
from oracle import reproject_np

F = fractions.Fraction


def marked(out):
    return tuple(np.flatnonzero(out[..., 2].reshape(-1) == C.BIG_Z).tolist())


def same_bits(a, b):
    """Equal bit for bit, NaN payloads and signs aside (NaN position for NaN position)."""
    an, bn = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn])


# ---- rule 1
def test_map_minimum_rules():
    nan_p = np.uint32([C.nan32_bits(+1)]).view(np.float32)[0]
    nan_n = np.uint32([C.nan32_bits(-1, 0x123)]).view(np.float32)[0]
    assert np.signbit(nan_n) and not np.signbit(nan_p) and np.isnan(nan_n) and np.isnan(nan_p)
    for nan in (nan_p, nan_n):
        assert reproject_np.map_minimum(np.float32([[nan, 3, -2, nan]])) == -2.0
        assert reproject_np.map_minimum(np.float32([[5, nan], [nan, 7]])) == 5.0
        assert math.isnan(reproject_np.map_minimum(np.float32([[nan, nan]])))
        assert reproject_np.map_minimum(np.float32([[nan, -np.inf, 1]])) == -np.inf
        assert reproject_np.map_minimum(np.float32([[nan, np.inf]])) == np.inf
    assert reproject_np.map_minimum(np.float32([[0.0, -0.0, 1]])) == 0.0
    assert reproject_np.map_minimum(np.int16([[4, -32768, 32767]])) == -32768.0


@pytest.mark.parametrize("case", C.SPECIAL_CASES)
def test_special_maps_follow_rule_1(case):
    pos, neg = C.special_map(case, +1), C.special_map(case, -1)
    nan = np.isnan(pos)
    assert np.array_equal(nan, np.isnan(neg)) and nan.any()
    assert not np.signbit(pos[nan]).any() and np.signbit(neg[nan]).all()
    assert len(set(pos[nan].view(np.uint32).tolist())) == min(len(C.NAN_PAYLOADS), int(nan.sum()))
    outs = [reproject_np.reproject_image_to_3d(d, Q, True) for d in (pos, neg) for Q in (C.Q_CALC, C.Q_DENSE)]
    assert same_bits(outs[0], outs[2]) and same_bits(outs[1], outs[3])
    for o in outs:
        assert marked(o) == C.SPECIAL_MARKED[case]
    if case == "specials":
        # the marked pixels are the negative denormal, both zeros and the positive denormals
        assert sorted(pos.reshape(-1)[list(C.SPECIAL_MARKED[case])].tolist()) == sorted(
            [0.0, -0.0, 0.0, 2.0 ** -149, -2.0 ** -149, float(np.float32(1e-39)), 2.0 ** -127])
        assert reproject_np.map_minimum(pos) == -2.0 ** -149
    # without handle_missing nothing is marked and a NaN pixel is a NaN point
    plain = reproject_np.reproject_image_to_3d(pos, C.Q_CALC, False)
    assert marked(plain) == () and np.isnan(plain[nan]).all()


@pytest.mark.parametrize("md", C.LADDER_MD)
def test_ladder_flags(md):
    v = C.ladder_values(md)
    eps = float(C.EPS)
    assert float(v[0]) == md and float(v[4]) == md + 2 * eps
    assert [abs(float(x) - md) <= eps for x in v] == list(C.LADDER_FLAGS[md])
    want = tuple(sorted(p for p, f in zip(C.LADDER_AT, C.LADDER_FLAGS[md]) if f))
    outs = [reproject_np.reproject_image_to_3d(C.ladder_map(md, s), C.Q_CALC, True) for s in (+1, -1)]
    assert marked(outs[0]) == want == marked(outs[1]) and same_bits(*outs)


@pytest.mark.parametrize("H,W,nan_at,min_at", C.position_cases())
def test_position_maps(H, W, nan_at, min_at):
    outs = [reproject_np.reproject_image_to_3d(C.position_map(H, W, nan_at, min_at, s), C.Q_CALC, True) for s in (+1, -1)]
    assert marked(outs[0]) == (min_at,) == marked(outs[1]) and same_bits(*outs)
    assert np.isnan(outs[0].reshape(-1, 3)[nan_at]).all()


def test_grid_maps_have_one_marked_pixel():
    for H, W in C.SHAPES:
        for kind, Qn in (("s16", "calc"), ("f32", "calc"), ("f32", "dense")):
            d = C.grid_map(H, W, kind, Qn)
            assert marked(reproject_np.reproject_image_to_3d(d, C.Q_of(Qn), True)) == (C.min_position(H, W),)
            if kind == "s16" and H * W > 2:
                assert d.min() == -32768 and d.max() == 32767


def test_zero_w_and_overflow_cases():
    for kind in ("s16", "f32"):
        d, zero = C.zero_w_map(kind)
        out = reproject_np.reproject_image_to_3d(d, C.Q_ZERO)
        assert not np.isfinite(out[zero]).any() and np.isfinite(out[~zero]).all()
        assert np.isnan(out).any() and np.isposinf(out).any() and np.isneginf(out).any()
        assert np.isnan(out[zero][:, 0]).sum() == zero[:, 3].sum() and np.isnan(out[zero][:, 1]).sum() == zero[2].sum()


# ---- the float64 chain against exact arithmetic
def _ulps(a: np.float32, b: np.float32) -> int:
    def key(v):
        i = int(np.float32(v).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def test_oracle_against_exact_rationals():
    """Every sampled pixel of the dense-Q map whose denominator keeps 2^-20 of its terms: the
    float64 chain's handful of roundings (2^-53 each), amplified by at most 2^20, stays far below
    float32's 2^-24, so the oracle equals the exactly rounded quotient or its neighbour."""
    H, W = 37, 53
    d, Q = C.grid_map(H, W, "f32", "dense"), C.Q_DENSE
    got = reproject_np.reproject_image_to_3d(d, Q)
    idx = np.random.default_rng(3).choice(H * W, 400, replace=False)
    Qf = [[F(float(v)) for v in row] for row in Q]
    ok = 0
    for p in idx.tolist():
        y, x = divmod(p, W)
        dv = F(float(d[y, x]))
        q = [Qf[r][1] * y + Qf[r][3] + Qf[r][0] * x for r in range(4)]
        qw, qd = q[3], Qf[3][2] * dv
        w = qw + qd
        if abs(w) < F(1, 2 ** 20) * (abs(qw) + abs(qd)):
            continue
        ok += 1
        for c in range(3):
            exact = np.float32(float((q[c] + Qf[c][2] * dv) / w))
            assert _ulps(got[y, x, c], exact) <= 1, (p, c, got[y, x, c], exact)
    assert ok >= 0.9 * len(idx), ok


# ---- the contraction witness
def _fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (math.fma where Python has it)."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(F(a) * F(b) + F(c))


def fused_reproject(d, Q):
    """reproject_image_to_3d with every `a * b + c` of the chain fused, as a compiler with FP
    contraction on may write it."""
    H, W = d.shape
    Q = [[float(v) for v in row] for row in np.asarray(Q, np.float64)]
    out = np.empty((H, W, 3), np.float64)
    for y in range(H):
        for x in range(W):
            dv = float(d[y, x])
            q = [_fma(Q[r][0], x, _fma(Q[r][1], y, Q[r][3])) for r in range(4)]
            iW = 1.0 / _fma(Q[3][2], dv, q[3])
            out[y, x] = [_fma(Q[c][2], dv, q[c]) * iW for c in range(3)]
    return out.astype(np.float32)


def test_contraction_would_be_seen_in_float32():
    """The 37 x 53 dense-Q float32 map of test_gpu_reproject.py's shape grid.  On a random pixel a
    fused chain differs from the oracle by ~2^-53 of the result and float32 does not see it; on
    the map's cancellation pixels (grid_map) the denominator is ~2^-25 of its terms, the one
    rounding that fusing saves is ~2^-28 of the denominator, and float32 sees it on some of them.
    The witness exists at float32: nothing here is a threshold."""
    H, W = 37, 53
    d = C.grid_map(H, W, "f32", "dense")
    plain = reproject_np.reproject_image_to_3d(d, C.Q_DENSE)
    fused = fused_reproject(d, C.Q_DENSE)
    assert np.isfinite(plain).all() and np.isfinite(fused).all()
    differ = (plain.view(np.uint32) != fused.view(np.uint32)).any(-1)
    print(f"fused != unfused after the float32 cast on {int(differ.sum())} of {H * W} pixels")
    assert differ.any()
    # and only where the cancellation was built in
    assert (np.flatnonzero(differ) % 16 == 5).all()

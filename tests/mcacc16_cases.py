"""Shared inputs of the tests of McCnnAccurate's precision="bf16" (DESIGN.md §4.21): a numpy
restatement of the bfloat16 rounding, dense integer scorers with their exact numpy values, random
float nets with the two CPU twins' volumes and the distance E_q between them.  Everything is
computed once per process and never modified.  Images, shapes and models are mcacc_cases'."""
import functools

import numpy as np

import stereo_match_amd as sm
from mcacc_cases import SHAPES, UNITS, UNITS_INTERLEAVED, image, model, same_bits, twin_features  # noqa: F401  (re-exported)

C = 112

# (rows, columns) of the integer feature maps; the first two are mccnn_cases.SHAPES' tiny and ragged;
# tall has more rows than a grid has workgroup rows (65535)
GEOMETRY = {"tiny": (13, 45), "ragged": (37, 70), "narrow": (9, 19), "odd": (11, 37), "wide": (64, 256),
            "tall": (65538, 2)}


def bf16_round(x):
    """float32 -> the float32 value of its bfloat16 rounding (nearest, ties to even), in numpy
    integer operations; finite inputs that do not overflow."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def dense_integer_fc(F, U, seed=0):
    """A dense integer scorer: fw0 in {-1, 0, 1}, hidden weights in {-2 .. 2}, biases in {-2 .. 2};
    the output unit has a weight of +-1 at every eighth unit (its sum has to stay below 2^24 after
    up to three dense layers have grown the activations)."""
    rng = np.random.default_rng(700 + 10 * F + U + seed)
    fws = [rng.integers(-1, 2, (U, 2 * C)).astype(np.float32)]
    fbs = [rng.integers(-2, 3, U).astype(np.float32)]
    for _ in range(1, F):
        fws.append(rng.integers(-2, 3, (U, U)).astype(np.float32))
        fbs.append(rng.integers(-2, 3, U).astype(np.float32))
    wl = np.zeros((1, U), np.float32)
    wl[0, ::8] = rng.choice(np.array([-1.0, 1.0], np.float32), len(wl[0, ::8]))
    fws.append(wl)
    fbs.append(np.array([3], np.float32))
    return fws, fbs


@functools.lru_cache(maxsize=None)
def dense_model(F, U, precision="bf16"):
    """The dense integer scorer behind one random convolution (which the join tests do not run)."""
    base = model(1, 1, 32)
    fws, fbs = dense_integer_fc(F, U)
    return sm.McCnnAccurate(base.weights, base.biases, fws, fbs, precision=precision)


@functools.lru_cache(maxsize=None)
def int_features(geo, seed):
    """Integers 0 .. 3 as a feature map [H, W, 112] (read-only)."""
    H, W = GEOMETRY[geo]
    f = np.random.default_rng(900 + seed).integers(0, 4, (H, W, C)).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def int_volume16(F, U, geo, D, m0, a_is_left=True):
    """-z of the dense integer scorer with precision="bf16", from the network's definition with an
    explicit bfloat16 rounding of every hidden operand, NaN outside: float32 [D, H, W], and a dict
    of what the evaluation saw.  Exact integer arithmetic: int64 throughout, the matrix products
    carried in float64 (every partial sum is an integer below 2^53, asserted with the 2^24 bound)
    because numpy multiplies float64 matrices much faster than int64 ones.  Asserts |b| + sum |terms|
    < 2^24 for every unit of every layer, the output unit included."""
    fws, fbs = dense_integer_fc(F, U)
    fa, fb = int_features(geo, 0), int_features(geo, 1)
    H, W, _ = fa.shape
    vol = np.full((D, H, W), np.nan, np.float32)
    info = {"peak": 0, "changed": [0.0] * (F + 1), "ties": 0}

    def layer(h, w, b):
        mag = np.abs(h).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(b)
        assert mag.max() < 2**24, f"a sum of magnitudes reaches {mag.max()}"
        info["peak"] = max(info["peak"], int(mag.max()))
        return (h.astype(np.float64) @ w.astype(np.float64).T).astype(np.int64) + b.astype(np.int64)

    for d in range(D):
        s = m0 + d
        lo, hi = max(0, s), min(W, W + s)
        if lo >= hi:
            continue
        xa, xb = fa[:, lo:hi].astype(np.int64), fb[:, lo - s:hi - s].astype(np.int64)
        h = np.concatenate((xa, xb) if a_is_left else (xb, xa), axis=2).reshape(-1, 2 * C)
        h = np.maximum(layer(h, fws[0], fbs[0]), 0)
        for i in range(1, F):
            hf = h.astype(np.float32)
            assert np.array_equal(hf.astype(np.int64), h)  # below 2^24: float32 holds it
            hq = bf16_round(hf)
            info["changed"][i] = max(info["changed"][i], float((hq != hf).mean()))
            info["ties"] += int(((hf.view(np.uint32) & 0xFFFF) == 0x8000).sum())
            h = np.maximum(layer(hq.astype(np.int64), fws[i], fbs[i]), 0)
        z = layer(h, fws[F], fbs[F])
        vol[d, :, lo:hi] = -z[:, 0].astype(np.float32).reshape(H, hi - lo)
    vol.setflags(write=False)
    return vol, info


def float_net(F, U, precision="bf16", seed=0):
    """He-scaled random float scorer behind two random convolutions (mcacc_cases.model's, so the
    twin's feature maps are shared)."""
    m = model(2, F, U)
    return m.with_precision(precision)


@functools.lru_cache(maxsize=None)
def twin_raw(name, D, m0, F, U, precision, a_is_left=True):
    """The raw volume of a CPU twin on images 0 and 1 of a shape (read-only)."""
    fa, fb = twin_features(name, 2, 0), twin_features(name, 2, 1)
    v = float_net(F, U, precision).join(fa, fb, D, m0, a_is_left=a_is_left, raw=True, host=True)
    v.setflags(write=False)
    return v


def e_q(name, D, m0, F, U, a_is_left=True):
    """max |twin_bf16 - twin_f32| of the raw volume: what the rounding of the hidden operands moves.
    From the two CPU twins alone."""
    a, b = twin_raw(name, D, m0, F, U, "bf16", a_is_left), twin_raw(name, D, m0, F, U, "f32", a_is_left)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def exact_head_net(F, U, seed=0):
    """A net whose hidden layers are random floats while everything around them is exact in any
    arithmetic: fw0 and fb0 integers (with integer features the projections are integers), the
    output unit's weights in {-1, 0, 1} (h * w is exact, so fmaf(h, w, z) is the float32 add)."""
    rng = np.random.default_rng(300 + seed)
    base = model(1, 1, 32)
    fws = [rng.integers(-1, 2, (U, 2 * C)).astype(np.float32)]
    fbs = [rng.integers(-2, 3, U).astype(np.float32)]
    for _ in range(1, F):
        fws.append((rng.standard_normal((U, U)) * np.sqrt(2.0 / U)).astype(np.float32))
        fbs.append((rng.standard_normal(U) * 0.05).astype(np.float32))
    fws.append(rng.integers(-1, 2, (1, U)).astype(np.float32))
    fbs.append((rng.standard_normal(1) * 0.05).astype(np.float32))
    return sm.McCnnAccurate(base.weights, base.biases, fws, fbs, precision="bf16")


def chain_volume16(m, fa, fb, D, m0, a_is_left=True):
    """The bf16 twin's own chain restated in numpy for an exact_head_net on integer features: h1 in
    exact integers; per hidden layer the float32 products of the rounded operands (exact) added one
    at a time in ascending k to the float32 bias; the output unit's ascending float32 adds."""
    fws, fbs = m.fc_weights, m.fc_biases
    F = m.fc_layers
    H, W, _ = fa.shape
    vol = np.full((D, H, W), np.nan, np.float32)
    for d in range(D):
        s = m0 + d
        lo, hi = max(0, s), min(W, W + s)
        if lo >= hi:
            continue
        xa, xb = fa[:, lo:hi], fb[:, lo - s:hi - s]
        cat = np.concatenate((xa, xb) if a_is_left else (xb, xa), axis=2).reshape(-1, 2 * C)
        h = np.maximum(cat.astype(np.int64) @ fws[0].astype(np.int64).T + fbs[0].astype(np.int64), 0).astype(np.float32)
        for i in range(1, F):
            hq, wq = bf16_round(h), bf16_round(fws[i])
            acc = np.broadcast_to(fbs[i], (len(h), len(fbs[i]))).astype(np.float32)
            for k in range(hq.shape[1]):
                acc = acc + hq[:, k:k + 1] * wq[None, :, k]
            assert acc.dtype == np.float32
            h = np.where(acc > 0, acc, np.float32(0))
        z = np.full(len(h), fbs[F][0], np.float32)
        for k in range(h.shape[1]):
            z = z + h[:, k] * fws[F][0, k]
        vol[d, :, lo:hi] = -z.reshape(H, hi - lo)
    return vol

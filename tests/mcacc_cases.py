"""Shared inputs of the accurate MC-CNN tests: models, integer nets with their int64 numpy values and
the CPU twin's results, each computed once per process and never modified.  Images and shapes are
mccnn_cases'."""
import functools

import numpy as np

import stereo_match_amd as sm
from mccnn_cases import SHAPES, image, same_bits  # noqa: F401  (re-exported)

C = 112

# every hidden width the scorer takes, and the same twelve from the ends inwards (384, 32, 352, 64,
# ...): neither ascending nor descending, so one engine repacks its weights from larger to smaller
# U and back
UNITS = tuple(range(32, 385, 32))
UNITS_INTERLEAVED = tuple(u for pair in zip(UNITS[::-1], UNITS) for u in pair)[:len(UNITS)]


@functools.lru_cache(maxsize=None)
def model(conv_layers=2, fc_layers=2, units=96, seed=0):
    return sm.McCnnAccurate.random(conv_layers, fc_layers, units, seed)


def integer_conv(layers):
    """mccnn_cases.integer_model's pattern on 112 maps: layer i, output map co: weight 1 + (co + i) % 3
    at input map (5 co + 3 i + 1) % Cin, tap (co + 2 i) % 9, and -1 at input map (co + 7) % Cin, tap
    (3 co + 1) % 9; bias (co % 5) - 2."""
    ws, bs = [], []
    for i in range(layers):
        cin = 1 if i == 0 else C
        w = np.zeros((C, cin, 9), np.float32)
        for co in range(C):
            w[co, (5 * co + 3 * i + 1) % cin, (co + 2 * i) % 9] += 1 + (co + i) % 3
            w[co, (co + 7) % cin, (3 * co + 1) % 9] += -1
        ws.append(w.reshape(C, cin, 3, 3))
        bs.append(((np.arange(C) % 5) - 2).astype(np.float32))
    return ws, bs


def integer_fc(F, U):
    """An asymmetric integer scorer: a few nonzeros per row, at other columns in the left half of fw0
    than in its right half, so swapped halves, a transposed matrix or the wrong role give other
    integers."""
    fw0 = np.zeros((U, 2 * C), np.float32)
    for u in range(U):
        fw0[u, (5 * u + 1) % C] += 1 + u % 3
        fw0[u, (u + 7) % C] += -1
        fw0[u, C + (3 * u + 2) % C] += 2 - 3 * (u % 2)
        fw0[u, C + (11 * u + 5) % C] += 1
    fws, fbs = [fw0], [((np.arange(U) % 5) - 2).astype(np.float32)]
    for i in range(1, F):
        w = np.zeros((U, U), np.float32)
        for u in range(U):
            w[u, (7 * u + 3 * i + 1) % U] += 1 + (u + i) % 2
            w[u, (u + 5) % U] += -1
            w[u, (3 * u + 2) % U] += 1
        fws.append(w)
        fbs.append(((np.arange(U) % 3) - 1).astype(np.float32))
    fws.append(((np.arange(U) % 7) - 3).astype(np.float32)[None])
    fbs.append(np.array([2], np.float32))
    return fws, fbs


@functools.lru_cache(maxsize=None)
def integer_model(conv_layers=2, F=2, U=32):
    ws, bs = integer_conv(conv_layers)
    fws, fbs = integer_fc(F, U)
    return sm.McCnnAccurate(ws, bs, fws, fbs)


@functools.lru_cache(maxsize=None)
def integer_features(name, seed):
    """Small non-negative integers as a feature map [H, W, 112] (read-only)."""
    H, W = SHAPES[name]
    f = np.random.default_rng(50 + seed).integers(0, 4, (H, W, C)).astype(np.float32)
    f.setflags(write=False)
    return f


def int_volume(m, fa, fb, D, m0, a_is_left=True):
    """-z of the scorer of ``m`` on integer-valued features in int64 numpy, written from the network's
    definition (concatenate left and right, nn.Linear layers), NaN outside: float32 [D, H, W]; also
    the largest magnitude any sum reached."""
    fws = [w.astype(np.int64) for w in m.fc_weights]
    fbs = [b.astype(np.int64) for b in m.fc_biases]
    ia, ib = fa.astype(np.int64), fb.astype(np.int64)
    H, W, _ = fa.shape
    vol = np.full((D, H, W), np.nan, np.float32)
    peak = 0
    for d in range(D):
        s = m0 + d
        lo, hi = max(0, s), min(W, W + s)
        if lo >= hi:
            continue
        xa, xb = ia[:, lo:hi], ib[:, lo - s:hi - s]
        h = np.concatenate((xa, xb) if a_is_left else (xb, xa), axis=2)
        for i, (w, b) in enumerate(zip(fws, fbs)):
            h = h @ w.T + b
            peak = max(peak, int(np.abs(h).max()))
            if i < len(fws) - 1:
                h = np.maximum(h, 0)
        vol[d, :, lo:hi] = -h[..., 0].astype(np.float32)
    return vol, peak


@functools.lru_cache(maxsize=None)
def twin_features(name, conv_layers=2, seed=0, batch=0, integer=False):
    m = integer_model(conv_layers) if integer else model(conv_layers)
    f = m.features(image(name, seed, batch), host=True)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def twin_volume(name, D, m0, fc_layers=2, units=96, a_is_left=True, raw=False, conv_layers=2, batch=0):
    """The twin's volume of images 0 and 1 of a shape; every net of one conv_layers has the same
    convolutions (model's seed), so the feature maps are shared."""
    m = model(conv_layers, fc_layers, units)
    fa, fb = twin_features(name, conv_layers, 0, batch), twin_features(name, conv_layers, 1, batch)
    v = m.join(fa, fb, D, m0, a_is_left=a_is_left, raw=raw, host=True)
    v.setflags(write=False)
    return v

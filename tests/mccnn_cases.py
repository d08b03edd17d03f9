"""Shared inputs of the MC-CNN tests: images, models and the CPU twin's results, each computed once
per process and never modified."""
import functools

import numpy as np

import stereo_match_amd as sm

SHAPES = {"tiny": (13, 45), "ragged": (37, 70), "tiles": (70, 131)}


@functools.lru_cache(maxsize=None)
def image(name, seed=0, batch=0):
    """uint8 noise with some smooth structure (read-only); batch > 0 gives [batch, H, W]."""
    H, W = SHAPES[name]
    rng = np.random.default_rng(1000 + seed)
    n = max(batch, 1)
    yy, xx = np.mgrid[0:H, 0:W]
    img = rng.integers(0, 256, (n, H, W)).astype(np.float64) * 0.7 + 40 * np.sin(xx / 5.0 + seed) + 30 * np.cos(yy / 3.0)
    img = np.clip(img, 0, 255).astype(np.uint8)
    out = img if batch else img[0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(layers=4, seed=0):
    return sm.McCnnFast.random(layers, seed)


@functools.lru_cache(maxsize=None)
def integer_model(layers=2):
    """An asymmetric hand-made net: one nonzero weight per (co, ci, tap) pattern, small integers, so
    a transposed operand or a swapped tap gives other integers.  Layer i, output map co: weight
    1 + (co + i) % 3 at input map (5 co + 3 i + 1) % Cin, tap (co + 2 i) % 9, and -1 at input map
    (co + 7) % Cin, tap (3 co + 1) % 9 (layer 0 has one input map); bias (co % 5) - 2."""
    ws, bs = [], []
    for i in range(layers):
        cin = 1 if i == 0 else 64
        w = np.zeros((64, cin, 9), np.float32)
        for co in range(64):
            w[co, (5 * co + 3 * i + 1) % cin, (co + 2 * i) % 9] += 1 + (co + i) % 3
            w[co, (co + 7) % cin, (3 * co + 1) % 9] += -1
        ws.append(w.reshape(64, cin, 3, 3))
        bs.append(((np.arange(64) % 5) - 2).astype(np.float32))
    return sm.McCnnFast(ws, bs)


@functools.lru_cache(maxsize=None)
def twin_features(name, layers=4, seed=0, batch=0, integer=False):
    m = integer_model(layers) if integer else model(layers)
    f = m.features(image(name, seed, batch), host=True)
    f.setflags(write=False)
    return f


def same_bits(a, b):
    """Equal NaN masks and equal values elsewhere (np.array_equal on the float bits would also tell
    NaN payloads apart, which no caller can observe)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])

"""Independent numpy restatement of fastNlMeansDenoising on uint8 gray images (DESIGN.md
§4.8: OpenCV's FastNlMeansDenoisingInvoker, NORM_L2, one channel, int accumulators), written
from its text and sharing no code with the package:

* :func:`weight_table` — the fixed-point weight table (the only floating-point part);
* :func:`denoise` — vectorised: per search offset a squared-difference image and its box sum
  through 2-D cumulative sums in int64;
* :func:`denoise_direct` — a per-pixel scalar loop, for tiny images.

Both return ``(out uint8 [H, W], wsum int64 [H, W])``.  A plain module, not a conftest.
"""
import math

import numpy as np

INT32_MAX = 2147483647


def windows(tws, sws):
    """(th, t, sh, s, b): half sizes, the odd sizes actually used, and the border."""
    th, sh = int(tws) // 2, int(sws) // 2
    return th, 2 * th + 1, sh, 2 * sh + 1, th + sh


def weight_table(h, tws, sws):
    """(tab int64 [n], fpm, shift)."""
    _, t, _, s, _ = windows(tws, sws)
    fpm = min(INT32_MAX // (s * s * 255), INT32_MAX)
    shift = 0
    while (1 << shift) < t * t:
        shift += 1
    mult = float(1 << shift) / (t * t)
    n = int(65025 / mult + 1)
    with np.errstate(over="ignore"):
        hh = float(np.float32(h) * np.float32(h))  # h is a C float
    tab = np.zeros(n, np.int64)
    floor_w = 0.001 * fpm
    for a in range(n):
        x = -(a * mult)
        if hh == 0.0:
            w = float("nan") if x == 0.0 else 0.0  # -0 / 0 is NaN, -x / 0 is -inf and exp(-inf) = 0
        else:
            w = math.exp(x / hh)
        if w != w:
            w = 1.0
        v = int(round(fpm * w))  # Python's round: half to even
        if v < floor_w:
            v = 0
        tab[a] = v
    return tab, fpm, shift


def extend(src, b):
    """BORDER_REFLECT_101 by b on every side; reflected again as often as needed, a length-1
    axis repeats its sample (np.pad's "reflect" does both)."""
    return np.pad(np.asarray(src, np.uint8), b, mode="reflect")


def denoise(src, h, tws, sws):
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    th, t, sh, s, b = windows(tws, sws)
    tab, fpm, shift = weight_table(h, tws, sws)
    E = extend(src, b).astype(np.int64)
    est = np.zeros((H, W), np.int64)
    wsum = np.zeros((H, W), np.int64)
    # squared differences are needed on the image grown by th; that region of E starts at sh
    Hh, Wh = H + 2 * th, W + 2 * th
    base = E[sh:sh + Hh, sh:sh + Wh]
    for dy in range(-sh, sh + 1):
        for dx in range(-sh, sh + 1):
            sq = (base - E[sh + dy:sh + dy + Hh, sh + dx:sh + dx + Wh]) ** 2
            c = np.zeros((Hh + 1, Wh + 1), np.int64)
            c[1:, 1:] = sq.cumsum(0).cumsum(1)
            dist = c[t:, t:] - c[:-t, t:] - c[t:, :-t] + c[:-t, :-t]
            wgt = tab[dist >> shift]
            est += wgt * E[b + dy:b + dy + H, b + dx:b + dx + W]
            wsum += wgt
    assert int(est.max()) <= INT32_MAX and int(wsum.min()) >= fpm
    out = (est + wsum // 2) // wsum
    assert int(out.max()) <= 255
    return out.astype(np.uint8), wsum


def denoise_direct(src, h, tws, sws):
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    th, t, sh, s, b = windows(tws, sws)
    tab, fpm, shift = weight_table(h, tws, sws)
    E = [[int(v) for v in row] for row in extend(src, b)]
    out = np.zeros((H, W), np.uint8)
    wsum = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            py, px = y + b, x + b
            est = ws = 0
            for dy in range(-sh, sh + 1):
                for dx in range(-sh, sh + 1):
                    dist = 0
                    for qy in range(-th, th + 1):
                        ra, rb = E[py + qy], E[py + dy + qy]
                        for qx in range(-th, th + 1):
                            d = ra[px + qx] - rb[px + dx + qx]
                            dist += d * d
                    wgt = int(tab[dist >> shift])
                    est += wgt * E[py + dy][px + dx]
                    ws += wgt
            out[y, x] = ((est & 0xFFFFFFFF) + ws // 2) // ws
            wsum[y, x] = ws
    return out, wsum


def noisy_blobs(H, W, seed, sigma=8.0):
    """A smooth ramp plus two blobs plus Gaussian noise, clipped to uint8: patches repeat up to
    the noise, so many offsets get a non-zero weight (pure random bytes denoise to themselves)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 60.0 + 90.0 * xx / max(W - 1, 1) + 40.0 * yy / max(H - 1, 1)
    img += 50.0 * np.exp(-((xx - 0.3 * W) ** 2 + (yy - 0.4 * H) ** 2) / (2.0 * (0.15 * max(H, W) + 1.0) ** 2))
    img -= 40.0 * np.exp(-((xx - 0.75 * W) ** 2 + (yy - 0.7 * H) ** 2) / (2.0 * (0.1 * max(H, W) + 1.0) ** 2))
    img += rng.normal(0.0, sigma, (H, W))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)

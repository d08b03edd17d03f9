"""Independent numpy restatement of the rectification front end's per-pixel arithmetic
(DESIGN.md §4.7), written from its text and sharing no code with the package:

* :func:`rectify_map` — initUndistortRectifyMap(K, dist, R, P, (W, H), CV_32FC1) given
  ``iR = inv(P[:3,:3] @ R)``;
* :func:`remap` — cv2.remap(src, mapx, mapy, INTER_LINEAR) on uint8, constant-0 border,
  5-bit fixed-point bilinear;
* :func:`bgr2gray` — cvtColor(COLOR_BGR2GRAY) on uint8.

Plain float64 / float32 / int32 numpy with explicit operation order (numpy never contracts
a multiply and an add).  A plain module, not a conftest.
"""
import numpy as np


def rectify_map(K, dist, iR, H, W):
    """float32 (mapx, mapy), each [H, W]."""
    iR = np.asarray(iR, np.float64).reshape(3, 3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3 = (np.float64(v) for v in np.asarray(dist, np.float64).reshape(5))
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    j = np.arange(W, dtype=np.float64)[None, :]
    i = np.arange(H, dtype=np.float64)[:, None]
    X = iR[0, 0] * j + (iR[0, 1] * i + iR[0, 2])
    Y = iR[1, 0] * j + (iR[1, 1] * i + iR[1, 2])
    Wd = iR[2, 0] * j + (iR[2, 1] * i + iR[2, 2])
    with np.errstate(all="ignore"):
        w = 1.0 / Wd
        x = X * w
        y = Y * w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
        mapx = (fx * xd + cx).astype(np.float32)
        mapy = (fy * yd + cy).astype(np.float32)
    return mapx, mapy


def _fixed(m):
    """float32 map -> (valid, integer part, 5-bit fraction) as int64 / bool arrays."""
    m = np.asarray(m, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(m) < np.float32(16777216.0)
    s = np.rint(np.where(ok, m, np.float32(0)) * np.float32(32.0))  # float32 product, half to even
    s = s.astype(np.int64)
    return ok, s >> 5, s & 31


def remap(src, mapx, mapy):
    """uint8 [h, w] or [h, w, c] through float32 maps [H, W] -> uint8 [H, W] or [H, W, c]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    s3 = src[:, :, None] if src.ndim == 2 else src
    h, w, cn = s3.shape
    okx, ix, fx = _fixed(mapx)
    oky, iy, fy = _fixed(mapy)
    ok = okx & oky

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = s3[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int32)
        return np.where(inside[..., None], v, 0)

    a00 = ((32 - fx) * (32 - fy)).astype(np.int32)[..., None]
    a01 = (fx * (32 - fy)).astype(np.int32)[..., None]
    a10 = ((32 - fx) * fy).astype(np.int32)[..., None]
    a11 = (fx * fy).astype(np.int32)[..., None]
    acc = a00 * tap(iy, ix) + a01 * tap(iy, ix + 1) + a10 * tap(iy + 1, ix) + a11 * tap(iy + 1, ix + 1)
    out = (acc + 512) >> 10
    out = np.where(ok[..., None], out, 0).astype(np.uint8)
    return out[:, :, 0] if src.ndim == 2 else out


def bgr2gray(img):
    """uint8 [..., 3] BGR -> uint8 [...]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    b = img[..., 0].astype(np.int32)
    g = img[..., 1].astype(np.int32)
    r = img[..., 2].astype(np.int32)
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)

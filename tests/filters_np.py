"""Independent numpy restatements of the three filter arithmetics of DESIGN.md §4.11, written
from their statement, not from the kernels: the float64 Gaussian that equals
scipy.ndimage.gaussian_filter(mode='reflect') bit for bit, the reference's image_measure, and
cv2.pyrDown on uint8 (default size and border; parity with OpenCV unpinned).

numpy rounds every elementwise product and sum to float64 and fuses nothing, which is the
contract: t = a[i]*w[0]; for j = r..1: t = t + (a[refl(i-j)] + a[refl(i+j)])*w[j]."""
import numpy as np


def kernel1d(sigma, truncate=4.0):
    """(w[0 .. 2r], r) with scipy's expressions."""
    sigma = float(sigma)
    r = int(truncate * sigma + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / sigma ** 2 * x ** 2)
    return phi / phi.sum(), r


def refl(k, n):
    """scipy's 'reflect' (half-sample symmetric): k mod 2n, then 2n-1-k where >= n."""
    k = np.mod(np.asarray(k), 2 * n)
    return np.where(k >= n, 2 * n - 1 - k, k)


def gauss1d(a, sigma, axis, truncate=4.0):
    a = np.asarray(a, np.float64)
    w, r = kernel1d(sigma, truncate)
    h = w[r:]  # centre first
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    i = np.arange(n)
    t = a * h[0]
    for j in range(r, 0, -1):
        t = t + (a[refl(i - j, n)] + a[refl(i + j, n)]) * h[j]
    return np.moveaxis(t, 0, axis)


def gaussian_filter(a, sigma, truncate=4.0):
    """Axis 0 over the whole image, then axis 1 on that result.  sigma: scalar or (s0, s1)."""
    s = np.atleast_1d(np.asarray(sigma, np.float64))
    s0, s1 = float(s[0]), float(s[-1])
    return gauss1d(gauss1d(a, s0, 0, truncate), s1, 1, truncate)


def bgr2gray(img):
    b, g, r = (img[..., c].astype(np.int64) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def image_measure(img):
    g = bgr2gray(img).astype(np.float64)
    a = gaussian_filter(g, 5)
    b = gaussian_filter(a, 3)
    d = a - b
    e = 30.0 * d
    return a + e


def r101(p, n):
    """cv::borderInterpolate(BORDER_REFLECT_101)."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def pyr_down(src):
    """uint8 [H, W] or [H, W, C] -> uint8 [(H+1)//2, (W+1)//2(, C)].  Another integer dtype
    (values the image type cannot hold, for known answers) gives the int64 result."""
    src = np.asarray(src)
    assert src.dtype.kind in "ui"
    H, W = src.shape[:2]
    dH, dW = (H + 1) // 2, (W + 1) // 2
    k = (1, 4, 6, 4, 1)
    s = src.astype(np.int64)
    acc = np.zeros((dH, dW) + src.shape[2:], np.int64)
    for i in range(5):
        ys = [r101(2 * y + i - 2, H) for y in range(dH)]
        for j in range(5):
            xs = [r101(2 * x + j - 2, W) for x in range(dW)]
            acc += k[i] * k[j] * s[np.ix_(ys, xs)]
    out = (acc + 128) >> 8
    return out.astype(np.uint8) if src.dtype == np.uint8 else out


def image_u8(H, W, seed, channels=3):
    """A seeded smooth-plus-noise uint8 image (full range, no flat areas)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    shape = (H, W, channels) if channels > 1 else (H, W)
    base = 128 + 100 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0)
    if channels > 1:
        base = base[..., None] + np.arange(channels) * 9
    return np.clip(base + rng.integers(-40, 41, shape), 0, 255).astype(np.uint8)


def image_f64(H, W, seed):
    """A seeded float64 image around +-1e3 with sign changes (a contracted FMA shows)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((H, W)) * 1e3

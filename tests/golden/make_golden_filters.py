"""Generate the committed filter fixtures with scipy itself:

    python tests/golden/make_golden_filters.py          (needs scipy)

writes into tests/golden/filters/ (a directory of its own: every ``tests/golden/*.npz`` is read
as a matcher fixture):

  gauss_41x53_<tag>.npz   for sigma 5, 3, 1.2 and (2, 0.7): ``src`` (a seeded float64 [41, 53]
                          image around +-1e3), ``sigma`` (per axis), ``w0`` / ``w1`` (the host
                          weights of axis 0 / 1, w[0 .. 2r]) and ``out`` =
                          scipy.ndimage.gaussian_filter(src, sigma)
  image_measure_37x67.npz ``bgr`` (a seeded uint8 [37, 67, 3] image), ``gray`` (the integer
                          formula of DESIGN.md §4.7 (c)) and ``out``: the reference's
                          image_measure expression evaluated with scipy on that gray image

The fixtures are frozen: where scipy is not installed the restatement tests/filters_np.py is
checked against them, and the kernels always are.
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import filters_np  # noqa: E402

SIGMAS = {"s5": (5, 5), "s3": (3, 3), "s1p2": (1.2, 1.2), "s2_0p7": (2, 0.7)}


def scipy_weights(sigma, truncate=4.0):
    """The weights scipy itself builds for this sigma."""
    from scipy.ndimage import _filters

    sd = float(sigma)
    return _filters._gaussian_kernel1d(sd, 0, int(truncate * sd + 0.5))[::-1]


def main():
    out_dir = os.path.join(HERE, "filters")
    os.makedirs(out_dir, exist_ok=True)
    src = filters_np.image_f64(41, 53, seed=3)
    for tag, sig in SIGMAS.items():
        path = os.path.join(out_dir, f"gauss_41x53_{tag}.npz")
        np.savez_compressed(path, src=src, sigma=np.array(sig, np.float64), w0=scipy_weights(sig[0]),
                            w1=scipy_weights(sig[1]), out=ndimage.gaussian_filter(src, sigma=sig))
        print(path, os.path.getsize(path), "bytes")
    bgr = filters_np.image_u8(37, 67, seed=4)
    gray = filters_np.bgr2gray(bgr)
    img = gray.astype(float)
    img = ndimage.gaussian_filter(img, sigma=5)
    blurred = ndimage.gaussian_filter(img, 3)
    out = img + 30 * (img - blurred)
    path = os.path.join(out_dir, "image_measure_37x67.npz")
    np.savez_compressed(path, bgr=bgr, gray=gray, out=out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

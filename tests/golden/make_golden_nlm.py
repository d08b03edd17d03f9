"""Generate the committed fastNlMeansDenoising fixture from the numpy restatement
(tests/nlm_np.py):

    python tests/golden/make_golden_nlm.py

writes tests/golden/nlm/nlm_h10_t7_s21_40x56.npz: ``src`` (a smooth scene plus Gaussian noise,
uint8 [40, 56]), ``out`` and ``wsum`` at (h, templateWindowSize, searchWindowSize) =
(10, 7, 21), and ``params``.  The fixture is frozen: the restatement and the kernel are both
checked against it, so the two cannot drift together unnoticed.  It lives in a directory of
its own because every ``tests/golden/*.npz`` is read as a matcher fixture.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import nlm_np  # noqa: E402

NAME = "nlm_h10_t7_s21_40x56.npz"


def main():
    src = nlm_np.noisy_blobs(40, 56, seed=7)
    out, wsum = nlm_np.denoise(src, 10, 7, 21)
    path = os.path.join(HERE, "nlm", NAME)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, src=src, out=out, wsum=wsum, params=np.array([10, 7, 21], np.int32))
    print(path, os.path.getsize(path), "bytes; wsum / fpm from",
          wsum.min() / 19096.0, "to", wsum.max() / 19096.0)


if __name__ == "__main__":
    main()

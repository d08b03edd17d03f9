"""Writes tests/golden/jpeg/pillow.npz: small JPEG files made by Pillow (libjpeg-turbo, the library
behind cv2.imread) from synthetic pictures, with Pillow's own decode of each beside it:

    <name>__file   the file's bytes
    <name>__rgb    Image.open(file): RGB [H, W, 3], or [H, W] for a gray file
    <name>__y      the same file opened with draft('L', size): libjpeg's JCS_GRAYSCALE output, the
                   Y plane, as cv2.imread(file, 0) gives

Run from the repository root: python tests/golden/jpeg/make_golden_jpeg.py (needs Pillow; the
tests that read the fixture do not)."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jpeg_np as J  # noqa: E402

# name: (H, W, channels, Pillow's save options)
CASES = {
    "gray_q75": (37, 29, 1, dict(quality=75)),
    "gray_q30_rows": (26, 40, 1, dict(quality=30, restart_marker_rows=1)),
    "c444_q95": (17, 33, 3, dict(quality=95, subsampling=0)),
    "c444_q75_opt": (16, 16, 3, dict(quality=75, subsampling=0, optimize=True)),
    "c422_q30": (31, 35, 3, dict(quality=30, subsampling=1)),
    "c422_q75_rows": (24, 40, 3, dict(quality=75, subsampling=1, restart_marker_rows=1)),
    "c420_q75": (45, 37, 3, dict(quality=75, subsampling=2)),
    "c420_q95_opt": (21, 19, 3, dict(quality=95, subsampling=2, optimize=True)),
    "c420_q75_blocks": (35, 41, 3, dict(quality=75, subsampling=2, restart_marker_blocks=3)),
    "c420_1x1": (1, 1, 3, dict(quality=75, subsampling=2)),
    "c420_9x5": (9, 5, 3, dict(quality=75, subsampling=2)),
    "c420_17x2": (17, 2, 3, dict(quality=75, subsampling=2)),
    "c422_7x3": (7, 3, 3, dict(quality=75, subsampling=1)),
    "c420_131x97_q75": (131, 97, 3, dict(quality=75, subsampling=2)),
}


def main():
    out = {}
    for i, (name, (H, W, ch, kw)) in enumerate(CASES.items()):
        img = J.test_image(100 + i, H, W, ch)
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        data = b.getvalue()
        out[name + "__file"] = np.frombuffer(data, np.uint8)
        out[name + "__rgb"] = np.asarray(Image.open(io.BytesIO(data)))
        im = Image.open(io.BytesIO(data))
        im.draft("L", im.size)
        out[name + "__y"] = np.asarray(im)
        assert out[name + "__y"].shape == (H, W), (name, out[name + "__y"].shape)
    np.savez_compressed(os.path.join(HERE, "pillow.npz"), **out)
    print("Pillow", Image.__version__, "libjpeg-turbo", features.version("jpg"), len(out) // 3, "files",
          os.path.getsize(os.path.join(HERE, "pillow.npz")), "bytes")


if __name__ == "__main__":
    main()

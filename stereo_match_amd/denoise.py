"""Non-local-means denoising: ``cv2.fastNlMeansDenoising`` as the reference's
test flow calls it in front of the matcher (``disparity_test.py:94-95``).

:func:`fastNlMeansDenoising` runs on the GPU (``sm_nlm_denoise_u8``) for uint8 single-channel
images, ``NORM_L2``.  The arithmetic is a version-scoped restatement of OpenCV's; parity with
OpenCV itself is unpinned.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _denoise_torch(src, dst, h, tws, sws):
    import torch

    if not src.is_cuda:
        raise ValueError("fastNlMeansDenoising: a torch source must be a CUDA tensor (or pass a numpy array)")
    if src.dtype != torch.uint8 or src.dim() not in (2, 3):
        raise ValueError(f"fastNlMeansDenoising: src must be a uint8 [H, W] or [N, H, W] tensor, not "
                         f"{src.dtype} {tuple(src.shape)}")
    src = src.contiguous()
    n = 1 if src.dim() == 2 else src.shape[0]
    H, W = src.shape[-2:]
    if dst is None:
        dst = torch.empty_like(src)
    elif not (_is_torch(dst) and dst.is_cuda and dst.device == src.device and dst.dtype == torch.uint8
              and dst.shape == src.shape and dst.is_contiguous()):
        raise ValueError("fastNlMeansDenoising: dst must be a contiguous uint8 CUDA tensor of the source's shape")
    eng = _lib.engine(src.device.index or 0)
    eng.set_stream(torch.cuda.current_stream(src.device).cuda_stream)
    eng.nlm_denoise_batch_device(src.data_ptr(), n, H * W, H, W, W, h, tws, sws, dst.data_ptr())
    return dst


def fastNlMeansDenoising(src, dst=None, h=3, templateWindowSize=7, searchWindowSize=21, device=0):
    """``cv2.fastNlMeansDenoising(src, dst, h, templateWindowSize, searchWindowSize)`` on uint8
    single-channel images.

    numpy ``uint8 [H, W]`` in -> numpy out (synchronous; ``dst`` is filled and returned when
    given).  A torch CUDA ``uint8 [H, W]`` or ``[N, H, W]`` tensor in -> CUDA tensor out on
    torch's current stream, the batch in one launch.

    ``templateWindowSize`` 1..9 and ``searchWindowSize`` 1..35 (an even size counts as the next
    odd one), any finite ``h >= 0``.  Colour input (``fastNlMeansDenoisingColored``), the
    ``Multi`` variants and ``NORM_L1`` are not implemented."""
    h = float(h)
    tws, sws = int(templateWindowSize), int(searchWindowSize)
    if _is_torch(src):
        return _denoise_torch(src, dst, h, tws, sws)
    a = np.asarray(src)
    if a.dtype != np.uint8:
        raise ValueError(f"fastNlMeansDenoising: src must be uint8, not {a.dtype}")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim != 2:
        raise ValueError(f"fastNlMeansDenoising: src must be a single-channel [H, W] image, not shape {a.shape} "
                         "(fastNlMeansDenoisingColored is not implemented)")
    return _lib.engine(device).nlm_denoise(a, h, tws, sws, dst)

"""The reference's host image filters on the GPU.

* :func:`gaussian_filter` — ``scipy.ndimage.gaussian_filter`` on float64 images,
  ``mode='reflect'``; with the weights of :func:`gaussian_kernel1d` (scipy's own numpy
  expressions) the result equals scipy's bit for bit.
* :func:`image_measure` — the reference's "image smoothing and denoising" function
  (``disparity_test.py:54-66``, called on both images at ``:82-83``).
* :func:`pyrDown` — ``cv2.pyrDown`` as ``try_try.py:56-57`` calls it, on uint8 gray or BGR
  images.  A restatement of OpenCV's documented behaviour; parity with OpenCV is unpinned.

All three run in ``libstereo_match_amd.so`` (``sm_filter.hpp``); there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib

BORDER_DEFAULT = 4  # cv2.BORDER_DEFAULT = cv2.BORDER_REFLECT_101
MAX_RADIUS = 64     # sm_filter.hpp GF_MAX_R
_MEASURE_SIGMAS = (5, 3)   # disparity_test.py:58-59
_MEASURE_ALPHA = 30.0      # disparity_test.py:60


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def gaussian_kernel1d(sigma, truncate=4.0):
    """``(w, r)``: the weights ``scipy.ndimage.gaussian_filter1d(sigma, truncate=truncate)``
    correlates with, ``w[0 .. 2 r]``, and their radius ``r = int(truncate * sigma + 0.5)``.
    numpy on the host, the expressions scipy uses, so the values are scipy's on any machine.
    The library takes the half kernel ``w[r:]`` (centre first)."""
    sd = float(sigma)
    if not sd > 0 or not np.isfinite(sd):
        raise ValueError(f"gaussian_kernel1d: sigma must be a finite number > 0, not {sigma!r}")
    r = int(float(truncate) * sd + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return phi / phi.sum(), r


def _half(sigma, truncate):
    """The half kernel of one axis, or None for an axis scipy leaves alone (sigma <= 1e-15)
    or filters with the single weight 1 (r = 0)."""
    if not float(sigma) > 1e-15:
        return None
    w, r = gaussian_kernel1d(sigma, truncate)
    return np.ascontiguousarray(w[r:]) if r > 0 else None


def _sigma_pair(sigma):
    s = np.atleast_1d(np.asarray(sigma, np.float64))
    if s.ndim != 1 or s.size not in (1, 2) or not np.all(np.isfinite(s)):
        raise ValueError(f"gaussian_filter: sigma must be a finite scalar or a pair, not {sigma!r}")
    return (float(s[0]), float(s[-1]))


def _check_axes(ndim, axes):
    if ndim == 2:
        if axes is not None and tuple(axes) not in ((0, 1), (-2, -1)):
            raise ValueError(f"gaussian_filter: axes={axes!r} of a 2-D input (both axes, in order, only)")
    elif ndim == 3:
        if axes is None or tuple(axes) not in ((1, 2), (-2, -1)):
            raise ValueError(f"gaussian_filter: a 3-D input is a batch [N, H, W] and needs axes=(1, 2), not "
                             f"axes={axes!r}")
    else:
        raise ValueError(f"gaussian_filter: input must be 2-D, or 3-D [N, H, W] with axes=(1, 2), not {ndim}-D")


def _gauss_torch(x, output, wy, wx):
    import torch

    if not x.is_cuda:
        raise ValueError("gaussian_filter: a torch input must be a CUDA tensor (or pass a numpy array)")
    if x.dtype != torch.float64:
        raise ValueError(f"gaussian_filter: input must be float64, not {x.dtype}")
    if x.numel() and x.stride(-1) != 1:
        x = x.contiguous()
    if output is None:
        output = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    elif not (_is_torch(output) and output.is_cuda and output.device == x.device and output.dtype == torch.float64
              and output.shape == x.shape and output.is_contiguous()):
        raise ValueError("gaussian_filter: output must be a contiguous float64 CUDA tensor of the input's shape")
    n = 1 if x.dim() == 2 else x.shape[0]
    H, W = x.shape[-2:]
    if x.numel() and (x.stride(-2) < W or (x.dim() == 3 and n > 1 and x.stride(0) < (H - 1) * x.stride(-2) + W)):
        x = x.contiguous()
    eng = _lib.engine(x.device.index or 0)
    eng.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
    eng.gauss2d_batch_device(x.data_ptr(), n, x.stride(0) if x.dim() == 3 else 0, H, W, x.stride(-2) if H * W else W,
                             wy, wx, output.data_ptr(), H * W, W)
    return output


def gaussian_filter(input, sigma, order=0, output=None, mode="reflect", cval=0.0, truncate=4.0, *, radius=None,
                    axes=None, device=0):
    """``scipy.ndimage.gaussian_filter(input, sigma, ...)`` for float64 images, ``order=0``,
    ``mode='reflect'``; bit for bit scipy's result.

    ``input``: a 2-D float64 array, or a 3-D ``[N, H, W]`` batch with ``axes=(1, 2)`` (or
    ``(-2, -1)``), one launch for the batch.  ``sigma``: a scalar or a pair (axis 0, axis 1).
    ``output``: a float64 array of the input's shape to fill, or ``float``/``numpy.float64``.
    numpy in -> numpy out (synchronous); a torch CUDA float64 tensor in -> CUDA tensor out on
    torch's current stream.  A radius ``int(truncate * sigma + 0.5)`` above 64 raises
    :class:`SmError` (``SM_E_UNSUPPORTED``).  Anything else scipy accepts (another dtype,
    ``order``, ``mode``, ``radius``, other ``axes``) is a ``ValueError`` naming it; ``cval`` has
    no meaning in ``'reflect'`` mode and is ignored, as scipy does."""
    if not (isinstance(order, (int, np.integer)) and order == 0):
        raise ValueError(f"gaussian_filter: order={order!r} is not implemented (order=0 only)")
    if mode != "reflect":
        raise ValueError(f"gaussian_filter: mode={mode!r} is not implemented (mode='reflect' only)")
    if radius is not None:
        raise ValueError(f"gaussian_filter: radius={radius!r} is not implemented (the radius follows from truncate)")
    sy, sx = _sigma_pair(sigma)
    if _is_torch(input):
        _check_axes(input.dim(), axes)
        return _gauss_torch(input, output, _half(sy, truncate), _half(sx, truncate))
    if not isinstance(input, np.ndarray):
        input = np.asarray(input)
    if input.dtype != np.float64:
        raise ValueError(f"gaussian_filter: input must be float64, not dtype {input.dtype}")
    _check_axes(input.ndim, axes)
    if output is not None and not isinstance(output, np.ndarray):
        if np.dtype(output) != np.float64:
            raise ValueError(f"gaussian_filter: output dtype {np.dtype(output)} is not implemented (float64 only)")
        output = None
    if output is not None and (output.dtype != np.float64 or output.shape != input.shape
                               or not output.flags.writeable):
        raise ValueError(f"gaussian_filter: output must be a writeable float64 array of shape {input.shape}")
    res = _lib.engine(device).gauss2d(input, _half(sy, truncate), _half(sx, truncate))
    if output is None:
        return res
    output[...] = res
    return output


def _measure_kernels():
    return tuple(_half(s, 4.0) for s in _MEASURE_SIGMAS)


def image_measure(img, test_mode=False, device=0):
    """The reference's ``image_measure(img, test_mode)`` (``disparity_test.py:54-66``)::

        img = cv2.cvtColor(img, cv2.COLOR_BGR2GRAY).astype(float)
        img = ndimage.gaussian_filter(img, sigma=5)
        blurred = ndimage.gaussian_filter(img, 3)
        return img + 30 * (img - blurred)

    uint8 BGR ``[H, W, 3]`` in -> float64 ``[H, W]`` out; numpy (synchronous) or a torch CUDA
    tensor, which may be a batch ``[N, H, W, 3]`` -> ``[N, H, W]`` on torch's current stream.
    The gray stage is :func:`cvtColor`'s, the two filters are :func:`gaussian_filter`'s.
    ``test_mode`` is accepted and ignored: the reference shows the result in a matplotlib window
    when it is set, and plotting is out of scope."""
    w1, w2 = _measure_kernels()
    if _is_torch(img):
        import torch

        if not img.is_cuda:
            raise ValueError("image_measure: a torch image must be a CUDA tensor (or pass a numpy array)")
        if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
            raise ValueError(f"image_measure: the image must be uint8 BGR [H, W, 3] or [N, H, W, 3], not "
                             f"{img.dtype} {tuple(img.shape)}")
        img = img.contiguous()
        n = 1 if img.dim() == 3 else img.shape[0]
        H, W = img.shape[-3:-1]
        out = torch.empty(img.shape[:-1], dtype=torch.float64, device=img.device)
        eng = _lib.engine(img.device.index or 0)
        eng.set_stream(torch.cuda.current_stream(img.device).cuda_stream)
        eng.image_measure_batch_device(img.data_ptr(), n, H * W * 3, H, W, W * 3, w1, w2, _MEASURE_ALPHA,
                                       out.data_ptr())
        return out
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"image_measure: the image must be uint8 BGR [H, W, 3], not {a.dtype} {a.shape}")
    return _lib.engine(device).image_measure(a, w1, w2, _MEASURE_ALPHA)


def _pyr_torch(src, dst):
    import torch

    if not src.is_cuda:
        raise ValueError("pyrDown: a torch source must be a CUDA tensor (or pass a numpy array)")
    if src.dtype != torch.uint8 or src.dim() not in (2, 3, 4) or (src.dim() == 4 and src.shape[-1] != 3):
        raise ValueError(f"pyrDown: src must be uint8 [H, W], [H, W, 3], [N, H, W] or [N, H, W, 3], not "
                         f"{src.dtype} {tuple(src.shape)}")
    src = src.contiguous()
    # a 3-D tensor whose last dimension is 3 is one BGR image, as in cv2
    cn = 3 if src.dim() == 4 or (src.dim() == 3 and src.shape[-1] == 3) else 1
    lead = src.dim() - (3 if cn == 3 else 2)
    n = src.shape[0] if lead else 1
    H, W = src.shape[lead:lead + 2]
    dH, dW = (H + 1) // 2, (W + 1) // 2
    shape = tuple(src.shape[:lead]) + ((dH, dW, 3) if cn == 3 else (dH, dW))
    if dst is None:
        dst = torch.empty(shape, dtype=torch.uint8, device=src.device)
    elif not (_is_torch(dst) and dst.is_cuda and dst.device == src.device and dst.dtype == torch.uint8
              and tuple(dst.shape) == shape and dst.is_contiguous()):
        raise ValueError(f"pyrDown: dst must be a contiguous uint8 CUDA tensor of shape {shape}")
    eng = _lib.engine(src.device.index or 0)
    eng.set_stream(torch.cuda.current_stream(src.device).cuda_stream)
    eng.pyr_down_batch_device(src.data_ptr(), n, H * W * cn, H, W, W * cn, cn, dst.data_ptr(), dH * dW * cn, dW * cn)
    return dst


def pyrDown(src, dst=None, dstsize=None, borderType=None, device=0):
    """``cv2.pyrDown(src)``: the 5 x 5 kernel (1, 4, 6, 4, 1)^2 / 256 with ``BORDER_REFLECT_101``
    and every second row and column kept, ``((H + 1) // 2, (W + 1) // 2)``, in exact integer
    arithmetic with OpenCV's rounding ``(sum + 128) >> 8``.

    uint8 ``[H, W]`` or ``[H, W, 3]``, numpy (synchronous; ``dst`` is filled and returned when
    given) or torch CUDA, where a batch ``[N, H, W]`` / ``[N, H, W, 3]`` shares one launch (a
    3-D tensor whose last dimension is 3 is one BGR image).  The result goes into
    ``StereoSGBM.compute`` as it stands.  Only the default ``dstsize`` and ``borderType``
    (``BORDER_DEFAULT``) are implemented: anything else is a ``ValueError``."""
    if borderType is not None and borderType != BORDER_DEFAULT:
        raise ValueError(f"pyrDown: borderType={borderType!r} is not implemented (BORDER_DEFAULT only)")
    shape = tuple(src.shape) if hasattr(src, "shape") else np.asarray(src).shape
    if dstsize is not None and tuple(dstsize) != ():
        batched = _is_torch(src) and (len(shape) == 4 or (len(shape) == 3 and shape[-1] != 3))
        H, W = shape[1:3] if batched else shape[:2]
        if len(shape) < 2 or tuple(int(v) for v in dstsize) != ((W + 1) // 2, (H + 1) // 2):
            raise ValueError(f"pyrDown: dstsize={dstsize!r} is not implemented (the default size only)")
    if _is_torch(src):
        return _pyr_torch(src, dst)
    a = np.asarray(src)
    if a.dtype != np.uint8:
        raise ValueError(f"pyrDown: src must be uint8, not {a.dtype}")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError(f"pyrDown: src must be a 1- or 3-channel [H, W] / [H, W, 3] image, not shape {a.shape}")
    out = _lib.engine(device).pyr_down(a)
    if dst is None:
        return out
    if (not isinstance(dst, np.ndarray) or dst.dtype != np.uint8 or dst.shape != out.shape
            or not dst.flags.writeable):
        raise ValueError(f"pyrDown: dst must be a writeable uint8 array of shape {out.shape}")
    dst[...] = out
    return dst

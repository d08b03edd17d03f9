"""Baseline JPEG input on the GPU: the plumbing behind :func:`imread`,
:func:`imdecode`, :func:`imdecode_batch` and :func:`imdecode_host` of :mod:`.png` for buffers that
begin ``FF D8 FF`` -- what ``build_npz.py:229``, ``io_functions.py:92`` and ``try_try.py:56-57``
hand to ``cv2.imread``.

The pixels are libjpeg-turbo's with its defaults (islow IDCT, fancy upsampling), bit for bit, for
baseline files with 1 or 3 (YCbCr) components at 4:4:4, 4:2:2 or 4:2:0, with or without restart
markers.  ``flags=1`` gives BGR (a gray file replicated), ``flags=0`` the Y plane itself (no
BGR-to-gray conversion happens), ``flags=-1`` gray for a gray file and BGR for a colour file;
``keep_channel_order`` gives RGB.  The EXIF orientation is **not** applied (OpenCV 3.1 and later
apply it unless ``IMREAD_IGNORE_ORIENTATION`` is set).  Progressive and the other unsupported
kinds raise ``SmError(SM_E_UNSUPPORTED)`` with the reason; a file that does not decode cleanly
raises ``SmError(SM_E_DATA)`` -- also where libjpeg would warn and return a picture.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def is_jpeg(f: np.ndarray) -> bool:
    """Whether the file bytes ``f`` (a uint8 array) begin with SOI and another marker."""
    return f.size >= 3 and f[0] == 0xFF and f[1] == 0xD8 and f[2] == 0xFF


def _params(info, flags, keep_channel_order):
    """(sm_jpegdec_params, output shape) for files of geometry ``info``."""
    H, W, ch, sub = info
    flags = int(flags)
    if flags not in (1, 0, -1):
        raise ValueError(f"flags must be 1 (BGR), 0 (gray) or -1 (unchanged), not {flags}")
    p = _lib.SmJpegDecParams()
    p.flags, p.keep_channel_order, p.file_channels, p.subsampling = flags, int(bool(keep_channel_order)), ch, sub
    three = flags == 1 or (flags == -1 and ch == 3)
    return p, ((H, W, 3) if three else (H, W))


def decode(f: np.ndarray, flags, device, keep_channel_order):
    """One file on the device into a numpy array."""
    prm, shape = _params(_lib.jpeg_info(f), flags, keep_channel_order)
    return _lib.engine(device).jpeg_decode(f, prm, np.empty(shape, np.uint8))


def decode_host(f: np.ndarray, flags, keep_channel_order):
    """One file by the CPU twin."""
    prm, shape = _params(_lib.jpeg_info(f), flags, keep_channel_order)
    return _lib.jpeg_decode_host(f, prm, np.empty(shape, np.uint8))


def decode_batch_device(files, flags, device, keep_channel_order=False, out=None):
    """The files (uint8 arrays, equal geometry) on the device: a CUDA tensor [N, ...]; ``out``: a
    uint8 CUDA tensor of that shape to decode into (its last dimensions contiguous)."""
    import torch

    if not files:
        raise ValueError("empty batch")
    info, descs = None, []
    for i, f in enumerate(files):
        try:
            descs.append(_lib.jpeg_parse(f))  # the one parse of the file: geometry and tables
        except _lib.SmError as e:
            raise _lib.SmError(e.code, f"image {i}: {e.args[0]}") from None
        g = _lib.jpeg_desc_info(descs[-1])
        if info is None:
            info = g
        elif g != info:
            raise _lib.SmError(_lib.SM_E_UNSUPPORTED,
                               f"image {i}: geometry {g} differs from image 0's {info} (H, W, channels, subsampling)")
    prm, shape = _params(info, flags, keep_channel_order)
    H, W = info[:2]
    dev = torch.device("cuda", int(device))
    eng = _lib.engine(dev.index)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    n, dsz = len(files), descs[0].size
    offs, at = [], (n * dsz + 15) & ~15
    for f in files:
        offs.append(at)
        at += (f.size + 15) & ~15
    blob = torch.empty(at, dtype=torch.uint8, pin_memory=True)  # the descriptors, then the files
    hb = blob.numpy()
    for i, (f, o) in enumerate(zip(files, offs)):
        hb[i * dsz:(i + 1) * dsz] = descs[i]
        hb[o:o + f.size] = f
    tab = torch.tensor([offs, [f.size for f in files]], dtype=torch.int64).pin_memory()
    d_blob = blob.to(dev, non_blocking=True)
    d_tab = tab.to(dev, non_blocking=True)
    if out is None:
        out = torch.empty((n,) + shape, dtype=torch.uint8, device=dev)
    elif (tuple(out.shape) != (n,) + shape or out.dtype != torch.uint8 or not out.is_cuda
          or out[0, 0].stride() != torch.empty(shape[1:]).stride()):
        raise ValueError(f"out must be a uint8 CUDA tensor {(n,) + shape} with contiguous rows")
    status = torch.empty(n, dtype=torch.int32, device=dev)
    prm.max_file_bytes = max(f.size for f in files)
    prm.d_desc = d_blob.data_ptr()
    eng.jpeg_decode_batch_device(d_blob.data_ptr(), d_tab[0].data_ptr(), d_tab[1].data_ptr(), n, H, W, prm,
                                 out.data_ptr(), out.stride(0), out.stride(1), status.data_ptr())
    st = status.cpu().tolist()  # synchronises: the pinned staging buffers are free again
    for i, code in enumerate(st):
        if code:
            lib = _lib.load()
            raise _lib.SmError(lib.sm_jpegdec_status_code(code),
                               f"jpeg decode: image {i}: {lib.sm_jpegdec_status_message(code).decode()}")
    return out

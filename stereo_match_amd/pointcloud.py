"""Point clouds on the GPU: the tail every script of the reference ends with,

    points = cv2.reprojectImageTo3D(disp, Q)
    colors = cv2.cvtColor(img, cv2.COLOR_BGR2RGB)
    mask = lo < disp < hi
    write_ply(fn, points[mask], colors[mask])

(``disparity_calculation.py:302-320``, ``disparity_test.py:230-265``, ``try_try.py:90-96``,
``mapTo3D_mc_cnn.py:124`` ff.) without the full ``[H, W, 3]`` image, the numpy compaction or
``np.savetxt``:

* :func:`extract_point_cloud` — mask, reprojection, compaction and the BGR -> RGB swap in one
  pass over the map (``sm_cloud_extract*``);
* :func:`format_ply` — the rows ``'%f %f %f %d %d %d '`` of ``io_functions.write_ply``, byte for
  byte Python's, from an integer-only formatter (``sm_ply_format_device`` / ``sm_ply_format_host``);
* :func:`write_point_cloud` — both back to back and the file (``sm_cloud_ply*``).

:func:`stereo_match_amd.write_ply` stays the general path (any dtype, through ``np.savetxt``).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from .reproject import PLY_HEADER


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _cloud_params(lo, hi, zero_nonfinite, handleMissingValues) -> _lib.SmCloudParams:
    p = _lib.SmCloudParams()
    p.lo_mode = _lib.SM_CLOUD_LO_NONE
    if isinstance(lo, str):
        if lo != "min":
            raise ValueError(f"lo must be a number, None or 'min', not {lo!r}")
        p.lo_mode = _lib.SM_CLOUD_LO_MIN
    elif lo is not None:
        p.lo = float(lo)
        p.lo_mode = _lib.SM_CLOUD_LO_VALUE
    if hi is not None:
        p.hi = float(hi)
        p.has_hi = 1
    if (p.lo_mode == _lib.SM_CLOUD_LO_VALUE and math.isnan(p.lo)) or (p.has_hi and math.isnan(p.hi)):
        raise ValueError("a NaN bound passes no pixel: leave the bound out (None) instead")
    p.zero_nonfinite = int(bool(zero_nonfinite))
    p.handle_missing = int(bool(handleMissingValues))
    return p


def _numpy_inputs(disparity, image_bgr):
    d = np.asarray(disparity)
    kind = {np.dtype(np.int16): 0, np.dtype(np.float32): 1}.get(d.dtype)
    if kind is None or d.ndim != 2:
        raise ValueError(f"disparity must be a 2-D int16 or float32 array, not {d.dtype} {d.shape}")
    img = np.asarray(image_bgr)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"image_bgr must be a uint8 [H, W, 3] array, not {img.dtype} {img.shape}")
    if img.shape[:2] != d.shape:
        raise ValueError(f"image_bgr {img.shape[:2]} and disparity {d.shape} differ in shape")
    if d.size == 0:
        raise ValueError("empty disparity map")
    d = np.ascontiguousarray(d)
    # a view with its own row stride is read in place; anything else is packed first
    if img.strides[2] != 1 or img.strides[1] != 3 or img.strides[0] < 3 * img.shape[1]:
        img = np.ascontiguousarray(img)
    return d, kind, img


def _torch_inputs(disparity, image_bgr):
    """(maps [n, H, W] contiguous, kind, image [n, H, W, 3] with contiguous pixels, batch?)"""
    import torch

    if not (_is_torch(image_bgr) and disparity.is_cuda and image_bgr.is_cuda and disparity.device == image_bgr.device):
        raise ValueError("a torch disparity needs a torch image_bgr on the same CUDA device (or pass numpy arrays)")
    kind = {torch.int16: 0, torch.float32: 1}.get(disparity.dtype)
    if kind is None or disparity.dim() not in (2, 3):
        raise ValueError(f"disparity must be an int16 or float32 [H, W] or [N, H, W] tensor, not "
                         f"{disparity.dtype} {tuple(disparity.shape)}")
    batch = disparity.dim() == 3
    if image_bgr.dtype != torch.uint8 or image_bgr.dim() != disparity.dim() + 1 or image_bgr.shape[-1] != 3:
        raise ValueError(f"image_bgr must be a uint8 [..., H, W, 3] tensor, not {image_bgr.dtype} "
                         f"{tuple(image_bgr.shape)}")
    if tuple(image_bgr.shape[:-1]) != tuple(disparity.shape):
        raise ValueError(f"image_bgr {tuple(image_bgr.shape[:-1])} and disparity {tuple(disparity.shape)} differ in shape")
    if disparity.numel() == 0:
        raise ValueError("empty disparity map")
    d = disparity.contiguous()
    img = image_bgr
    if not batch:
        d, img = d[None], img[None]
    H, W = d.shape[-2:]
    st = img.stride()
    if st[3] != 1 or st[2] != 3 or st[1] < 3 * W or (img.shape[0] > 1 and st[0] < (H - 1) * st[1] + 3 * W):
        img = img.contiguous()
    return d, kind, img, batch


def _engine_on_stream(t):
    import torch

    eng = _lib.engine(t.device.index or 0)
    eng.set_stream(torch.cuda.current_stream(t.device).cuda_stream)
    return eng


def extract_point_cloud(disparity, Q, image_bgr, lo=None, hi=None, *, zero_nonfinite=False,
                        handleMissingValues=False, device=0):
    """``reprojectImageTo3D(disparity, Q)[mask]`` and ``image_bgr[..., ::-1][mask]`` with
    ``mask = lo < disparity < hi``: ``(verts float32 [N, 3], colors uint8 [N, 3] RGB)``, in
    row-major order.  ``verts`` equals the full reprojection's pixels bit for bit.

    ``lo`` / ``hi``: strict bounds as Python scalars, compared as numpy >= 2 compares them (a
    float32 map with the bound rounded to float32, an int16 map exactly); ``None`` leaves a
    bound out; ``lo="min"`` is the map's own minimum (``try_try.py:92``; per map in a batch) as
    numpy's ``d > d.min()``: a map with a NaN pixel, of either sign, gives an empty cloud.
    ``handleMissingValues`` takes its minimum over the non-NaN pixels, as ``reprojectImageTo3D``.
    A NaN disparity passes no bound; a NaN bound is a ``ValueError``.
    ``zero_nonfinite`` replaces every NaN or infinite component by 0
    (``disparity_calculation.py:316-317``).

    numpy ``[H, W]`` map and ``[H, W, 3]`` image in -> numpy out (synchronous).  torch CUDA
    tensors in (``[H, W]`` or ``[N, H, W]``, image ``[..., 3]``) -> CUDA tensors of exactly ``N``
    rows on torch's current stream; a batch returns ``(verts, colors, counts)`` with the maps'
    rows one after the other and ``counts`` an int64 CPU tensor ``[N]``.  ``N`` is known only on
    the device: learning it costs ONE stream synchronisation in this call (after a first pass
    that only counts)."""
    prm = _cloud_params(lo, hi, zero_nonfinite, handleMissingValues)
    Qd = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(4, 4))
    if _is_torch(disparity):
        import torch

        d, kind, img, batch = _torch_inputs(disparity, image_bgr)
        n, H, W = d.shape
        eng = _engine_on_stream(d)
        counts_d = torch.empty(n, dtype=torch.int64, device=d.device)
        args = (d.data_ptr(), kind, img.data_ptr(), img.stride(0), img.stride(1), n, H, W, Qd, prm)
        eng.cloud_extract_batch_device(*args, 0, 0, 0, counts_d.data_ptr())
        counts = counts_d.cpu()  # the one synchronisation
        total = int(counts.sum())
        verts = torch.empty((total, 3), dtype=torch.float32, device=d.device)
        colors = torch.empty((total, 3), dtype=torch.uint8, device=d.device)
        if total:
            eng.cloud_extract_batch_device(*args, total, verts.data_ptr(), colors.data_ptr(), 0)
        return (verts, colors, counts) if batch else (verts, colors)
    d, kind, img = _numpy_inputs(disparity, image_bgr)
    return _lib.engine(device).cloud_extract(d, kind, img, Qd, prm)


def format_ply(verts, colors):
    """The PLY body of ``verts`` float32 ``[N, 3]`` and ``colors`` uint8 ``[N, 3]``: row i is
    ``'%f %f %f %d %d %d ' % (*verts[i], *colors[i])`` and a newline, byte for byte what
    ``write_ply`` (``np.savetxt``) writes, for every float32 bit pattern.

    CUDA tensors -> a uint8 CUDA tensor (device formatter, torch's current stream, one stream
    synchronisation to learn the size); numpy arrays -> ``bytes`` (the same row function on the
    CPU; no device needed).  Other dtypes are a ``ValueError``: ``write_ply`` is the general path."""
    if _is_torch(verts) or _is_torch(colors):
        import torch

        if not (_is_torch(verts) and _is_torch(colors) and verts.is_cuda and colors.is_cuda
                and verts.device == colors.device):
            raise ValueError("format_ply: verts and colors must both be CUDA tensors on one device (or numpy arrays)")
        if (verts.dtype != torch.float32 or colors.dtype != torch.uint8 or verts.dim() != 2 or verts.shape[1] != 3
                or tuple(colors.shape) != tuple(verts.shape)):
            raise ValueError(f"format_ply takes float32 verts [N, 3] and uint8 colors [N, 3], not {verts.dtype} "
                             f"{tuple(verts.shape)} / {colors.dtype} {tuple(colors.shape)}; write_ply is the general path")
        v, c = verts.contiguous(), colors.contiguous()
        n = v.shape[0]
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device=v.device)
        eng = _engine_on_stream(v)
        nb_d = torch.empty(1, dtype=torch.int64, device=v.device)
        eng.ply_format_device(v.data_ptr(), c.data_ptr(), n, 0, 0, nb_d.data_ptr())
        nb = int(nb_d.cpu()[0])  # the one synchronisation
        out = torch.empty(nb, dtype=torch.uint8, device=v.device)
        eng.ply_format_device(v.data_ptr(), c.data_ptr(), n, nb, out.data_ptr(), 0)
        return out
    v, c = np.asarray(verts), np.asarray(colors)
    if v.dtype != np.float32 or c.dtype != np.uint8 or v.ndim != 2 or v.shape[1] != 3 or c.shape != v.shape:
        raise ValueError(f"format_ply takes float32 verts [N, 3] and uint8 colors [N, 3], not {v.dtype} {v.shape} / "
                         f"{c.dtype} {c.shape}; write_ply is the general path")
    return _lib.ply_format_host(v, c).tobytes()


def write_point_cloud(fn, disparity, Q, image_bgr, lo=None, hi=None, *, zero_nonfinite=False,
                      handleMissingValues=False, device=0):
    """Write the ASCII PLY file of the masked point cloud and return ``N``: the file is byte for
    byte ``write_ply(fn, reprojectImageTo3D(disparity, Q)[mask], image_bgr[..., ::-1][mask])`` with
    ``mask = lo < disparity < hi`` (and the non-finite components zeroed first when
    ``zero_nonfinite``).  Arguments as :func:`extract_point_cloud`; one map (``[H, W]``), numpy
    arrays or torch CUDA tensors.  Only the text reaches host memory."""
    prm = _cloud_params(lo, hi, zero_nonfinite, handleMissingValues)
    Qd = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(4, 4))
    if _is_torch(disparity):
        import torch

        d, kind, img, batch = _torch_inputs(disparity, image_bgr)
        if batch:
            raise ValueError("write_point_cloud writes one map: pass an [H, W] disparity")
        _, H, W = d.shape
        eng = _engine_on_stream(d)
        meta = torch.empty(2, dtype=torch.int64, device=d.device)  # N, bytes
        args = (d.data_ptr(), kind, img.data_ptr(), img.stride(0), img.stride(1), 1, H, W, Qd, prm)
        eng.cloud_ply_batch_device(*args, 0, 0, meta.data_ptr(), meta.data_ptr() + 8)
        n, nb = (int(x) for x in meta.cpu())
        out = torch.empty(nb, dtype=torch.uint8, device=d.device)
        if nb:
            eng.cloud_ply_batch_device(*args, nb, out.data_ptr(), 0, 0)
        body = out.cpu().numpy()
    else:
        d, kind, img = _numpy_inputs(disparity, image_bgr)
        body, n = _lib.engine(device).cloud_ply(d, kind, img, Qd, prm)
    with open(fn, 'wb') as f:
        f.write((PLY_HEADER % dict(vert_num=n)).encode('utf-8'))
        f.write(memoryview(body))
    return n

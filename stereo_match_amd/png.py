"""PNG output on the GPU: what the reference's scripts hand to ``cv2.imwrite``
(``disparity_calculation.py:247-248,278-279,290-291``, ``rectified_img_cal.py:316-319``,
``disparity_test.py:114-115``, ``try_try.py:155,190``) and the KITTI disparity format, encoded
where the images already are:

* :func:`imencode_png`, :func:`imwrite` — uint8 gray, uint8 BGR and uint16 gray images, numpy
  arrays or torch CUDA tensors (``sm_png_encode*``); :func:`imencode_png_batch` for a CUDA batch;
* :func:`encode_disparity_png`, :func:`write_disparity_png` — an int16 x16 or float32 disparity
  map as the KITTI 16-bit PNG (disparity * 256, 0 invalid) or as a min-max uint8 picture
  (``show_disparity``'s ``normalize(NORM_MINMAX)``, ``plot_functions.py:99-100``), converted
  inside the filter kernel;
* :func:`imencode_png_host` — the same file from the same functions on the CPU.

PNG input, decoded on the device (``sm_png_decode*``):

* :func:`imread`, :func:`imdecode` — ``cv2.imread`` / ``cv2.imdecode`` for PNG files with flags
  ``1``, ``0`` and ``-1``, as a numpy array or (``as_tensor=True``) a CUDA tensor;
  :func:`imdecode_batch` for files of one geometry in one call;
* :func:`read_disparity_png`, :func:`decode_disparity_png` — a KITTI 16-bit map back to int16 x16
  or float32 disparities;
* :func:`imdecode_host` — the same pixels from the same functions on the CPU.

The files are standard PNGs (one IDAT chunk per 32 KiB of the filtered stream); the filter choice
and the coder are the package's own and documented in ``include/stereo_match_amd.h``.  The integer
rounding of the min-max picture is this package's contract: OpenCV's ``normalize`` is not pinned.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib, jpeg as _jpeg


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _unsupported(msg):
    raise _lib.SmError(_lib.SM_E_UNSUPPORTED, msg)


def _image_params(dtype_name: str, shape, filter, keep_channel_order) -> _lib.SmPngParams:
    p = _lib.SmPngParams()
    nd = len(shape)
    if dtype_name == "uint8" and (nd == 2 or (nd == 3 and shape[2] in (1, 3))):
        p.src_kind, p.channels = _lib.SM_PNG_SRC_U8, (3 if nd == 3 and shape[2] == 3 else 1)
    elif dtype_name == "uint16" and (nd == 2 or (nd == 3 and shape[2] == 1)):
        p.src_kind, p.channels = _lib.SM_PNG_SRC_U16, 1
    else:
        _unsupported(f"PNG output takes uint8 [H, W], uint8 [H, W, 3] and uint16 [H, W] images, not {dtype_name} "
                     f"{tuple(shape)}")
    p.keep_channel_order = int(bool(keep_channel_order))
    p.filter = -1 if filter is None else int(filter)
    return p


def _disp_params(dtype_name: str, shape, fmt, lo, hi, filter) -> _lib.SmPngParams:
    p = _lib.SmPngParams()
    if len(shape) != 2 or dtype_name not in ("int16", "float32"):
        raise ValueError(f"disparity must be a 2-D int16 (x16) or float32 map, not {dtype_name} {tuple(shape)}")
    p.src_kind = _lib.SM_PNG_SRC_DISP_I16 if dtype_name == "int16" else _lib.SM_PNG_SRC_DISP_F32
    p.channels = 1
    p.filter = -1 if filter is None else int(filter)
    if fmt == "kitti":
        p.disp_mode = _lib.SM_PNG_DISP_KITTI
        if lo is not None or hi is not None:
            raise ValueError("fmt='kitti' takes no bounds")
    elif fmt == "u8":
        p.disp_mode = _lib.SM_PNG_DISP_LINEAR_U8
        if (lo is None) != (hi is None):
            raise ValueError("give both lo and hi (in the map's own units), or neither for the map's min and max")
        if lo is not None:
            p.has_bounds, p.lo, p.hi = 1, int(lo), int(hi)
    else:
        raise ValueError(f"fmt must be 'kitti' or 'u8', not {fmt!r}")
    return p


def _torch_rows(t):
    """A tensor whose pixels are contiguous: (tensor, row stride in bytes)."""
    inner = 1
    ok = True
    for d in range(t.dim() - 1, 0, -1):
        ok = ok and t.stride(d) == inner
        inner *= t.shape[d]
    if not ok or t.stride(0) < inner:
        t = t.contiguous()
    return t, t.stride(0) * t.element_size()


def _encode_device(t, prm, nimg, H, W, img_stride, row_stride):
    """nimg files of a CUDA tensor on torch's current stream: a list of bytes, through pinned
    host memory."""
    import torch

    eng = _lib.engine(t.device.index or 0)
    eng.set_stream(torch.cuda.current_stream(t.device).cuda_stream)
    cap = _lib.load().sm_png_bound(H, W, *_lib.png_file_geometry(prm))
    if cap == 0:
        _unsupported(f"PNG output: an image of {W}x{H} is too large")
    cap = (cap + 15) & ~15
    out = torch.empty((nimg, cap), dtype=torch.uint8, device=t.device)
    nb = torch.empty(nimg, dtype=torch.int64, device=t.device)
    eng.png_encode_batch_device(t.data_ptr(), img_stride, row_stride, nimg, H, W, prm, cap, out.data_ptr(), nb.data_ptr())
    nb_h = torch.empty(nimg, dtype=torch.int64, pin_memory=True)
    nb_h.copy_(nb, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    sizes = [int(x) for x in nb_h]
    host = torch.empty((nimg, max(sizes)), dtype=torch.uint8, pin_memory=True)
    host.copy_(out[:, :max(sizes)], non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    h = host.numpy()
    return [h[i, :sizes[i]].tobytes() for i in range(nimg)]


def _numpy_image(img):
    a = np.asarray(img)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.size == 0:
        raise ValueError("empty image")
    inner = a.itemsize
    ok = True
    for d in range(a.ndim - 1, 0, -1):
        ok = ok and a.strides[d] == inner
        inner *= a.shape[d]
    if not ok or a.strides[0] < inner:
        a = np.ascontiguousarray(a)
    return a


def _encode(img, make_params, device, host):
    if _is_torch(img):
        if host:
            img = img.cpu().numpy()
        else:
            if not img.is_cuda:
                raise ValueError("a torch image must be a CUDA tensor (or pass a numpy array)")
            if img.numel() == 0:
                raise ValueError("empty image")
            if img.dim() == 3 and img.shape[2] == 1:
                img = img[:, :, 0]
            prm = make_params(str(img.dtype).replace("torch.", ""), tuple(img.shape))
            t, row_stride = _torch_rows(img)
            return _encode_device(t, prm, 1, t.shape[0], t.shape[1], 0, row_stride)[0]
    a = _numpy_image(img)
    prm = make_params(a.dtype.name, a.shape)
    if host:
        return _lib.png_encode_host(a, prm).tobytes()
    return _lib.engine(device).png_encode(a, prm).tobytes()


def imencode_png(img, *, filter=None, keep_channel_order=False, device=0) -> bytes:
    """The PNG file of ``img`` as ``bytes``: uint8 ``[H, W]`` (gray), uint8 ``[H, W, 3]`` (BGR in
    memory, RGB in the file, as ``cv2.imwrite``; ``keep_channel_order`` for an RGB source) or
    uint16 ``[H, W]``; a numpy array (uploaded, synchronous) or a torch CUDA tensor (encoded in
    place on torch's current stream, the bytes through pinned host memory).  ``filter``: ``None``
    picks a scanline filter per row, 0..4 fixes it.  Other dtypes or shapes raise
    ``SmError(SM_E_UNSUPPORTED)``."""
    return _encode(img, lambda dt, sh: _image_params(dt, sh, filter, keep_channel_order), device, False)


def imencode_png_host(img, *, filter=None, keep_channel_order=False) -> bytes:
    """:func:`imencode_png` on the CPU (``sm_png_encode_host``): the same bytes, no device."""
    return _encode(img, lambda dt, sh: _image_params(dt, sh, filter, keep_channel_order), 0, True)


def imencode_png_batch(imgs, *, filter=None, keep_channel_order=False):
    """The files of a uint8 CUDA batch ``[N, H, W]`` or ``[N, H, W, 3]`` (or uint16 ``[N, H, W]``)
    from one call: a list of ``bytes``, each equal to the image's own :func:`imencode_png`."""
    if not _is_torch(imgs) or not imgs.is_cuda or imgs.dim() not in (3, 4):
        raise ValueError("imencode_png_batch takes a CUDA tensor [N, H, W] or [N, H, W, 3]")
    if imgs.numel() == 0:
        raise ValueError("empty batch")
    prm = _image_params(str(imgs.dtype).replace("torch.", ""), tuple(imgs.shape[1:]), filter, keep_channel_order)
    t = imgs.contiguous()
    n, H, W = t.shape[:3]
    row = t.stride(1) * t.element_size()
    return _encode_device(t, prm, n, H, W, t.stride(0) * t.element_size(), row)


def imwrite(filename, img, *, device=0) -> bool:
    """``cv2.imwrite(filename, img)`` for ``.png`` files (BGR in memory, RGB in the file).  Another
    extension raises ``SmError(SM_E_UNSUPPORTED)``."""
    if os.path.splitext(str(filename))[1].lower() != ".png":
        _unsupported(f"imwrite writes .png files, not {filename!r}")
    data = imencode_png(img, device=device)
    with open(filename, "wb") as f:
        f.write(data)
    return True


def encode_disparity_png(disp, fmt="kitti", lo=None, hi=None, *, filter=None, device=0, host=False) -> bytes:
    """A disparity map (int16 x16, or float32 in pixels; numpy or torch CUDA) as a PNG file.

    ``fmt="kitti"``: 16-bit gray, value = disparity * 256, 0 = invalid (int16 ``d < 0 -> 0``, else
    ``min(65535, d << 4)``; float32 non-finite or ``<= 0 -> 0``, else ``min(65535, rint(d * 256))``).
    ``fmt="u8"`` (int16 maps): 8-bit gray ``clamp((d - lo) * 255 / (hi - lo), 0, 255)`` rounded half
    up in integers, ``lo`` / ``hi`` in the map's own units, or the map's minimum and maximum when
    left out (found on the device); ``hi == lo`` gives 0 everywhere.  ``host=True`` encodes on the
    CPU."""
    return _encode(disp, lambda dt, sh: _disp_params(dt, sh, fmt, lo, hi, filter), device, host)


def write_disparity_png(filename, disp, fmt="kitti", lo=None, hi=None, *, device=0) -> bool:
    """:func:`encode_disparity_png` into a file."""
    data = encode_disparity_png(disp, fmt, lo, hi, device=device)
    with open(filename, "wb") as f:
        f.write(data)
    return True


# ---- PNG input ---------------------------------------------------------------
def _file_bytes(buf) -> np.ndarray:
    if _is_torch(buf):
        buf = buf.cpu().numpy()
    b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, np.uint8).reshape(-1)
    return b


def _dec_params(info, flags, keep_channel_order=False, disp=None, invalid=None):
    """(sm_pngdec_params, output shape, numpy dtype) for a file of geometry ``info``."""
    H, W, ch, depth = info
    p = _lib.SmPngDecParams()
    p.file_channels, p.file_depth = ch, depth
    p.keep_channel_order = int(bool(keep_channel_order))
    if disp is not None:
        dt = np.dtype(disp)
        if dt == np.int16:
            p.out_kind, p.invalid_i16 = _lib.SM_PNGDEC_DISP_I16, int(-16 if invalid is None else invalid)
        elif dt == np.float32:
            p.out_kind, p.invalid_f32 = _lib.SM_PNGDEC_DISP_F32, float(-1.0 if invalid is None else invalid)
        else:
            raise ValueError(f"dtype must be int16 (x16) or float32, not {dt}")
        p.flags, p.disp_mode = -1, _lib.SM_PNG_DISP_KITTI
        return p, (H, W), dt
    flags = int(flags)
    if flags not in (1, 0, -1):
        raise ValueError(f"flags must be 1 (BGR), 0 (gray) or -1 (unchanged), not {flags}")
    p.flags = flags
    if flags == -1 and depth == 16:
        p.out_kind = _lib.SM_PNGDEC_U16
        return p, (H, W), np.dtype(np.uint16)
    p.out_kind = _lib.SM_PNGDEC_U8
    three = flags == 1 or (flags == -1 and ch >= 3)
    return p, ((H, W, 3) if three else (H, W)), np.dtype(np.uint8)


def _torch_dtype(dt):
    import torch

    return {"uint8": torch.uint8, "uint16": torch.uint16, "int16": torch.int16, "float32": torch.float32}[np.dtype(dt).name]


def _decode_batch_device(bufs, flags, device, keep_channel_order=False, disp=None, invalid=None):
    """The files ``bufs`` (equal geometry) on the device: a CUDA tensor [N, ...]."""
    import torch

    files = [_file_bytes(b) for b in bufs]
    if not files:
        raise ValueError("empty batch")
    info = None
    for i, f in enumerate(files):
        try:
            g = _lib.png_info(f)
        except _lib.SmError as e:
            raise _lib.SmError(e.code, f"image {i}: {e.args[0]}") from None
        if info is None:
            info = g
        elif g != info:
            _unsupported(f"image {i}: geometry {g} differs from image 0's {info} (H, W, channels, depth)")
    prm, shape, dt = _dec_params(info, flags, keep_channel_order, disp, invalid)
    H, W = info[:2]
    dev = torch.device("cuda", int(device))
    eng = _lib.engine(dev.index)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    offs, at = [], 0
    for f in files:
        offs.append(at)
        at += (f.size + 15) & ~15
    blob = torch.empty(max(at, 16), dtype=torch.uint8, pin_memory=True)
    hb = blob.numpy()
    for f, o in zip(files, offs):
        hb[o:o + f.size] = f
    tab = torch.tensor([offs, [f.size for f in files]], dtype=torch.int64).pin_memory()
    d_blob = blob.to(dev, non_blocking=True)
    d_tab = tab.to(dev, non_blocking=True)
    n = len(files)
    out = torch.empty((n,) + shape, dtype=_torch_dtype(dt), device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    prm.max_chunks = max(f.size for f in files) // 12 + 1
    prm.max_file_bytes = max(f.size for f in files)
    eng.png_decode_batch_device(d_blob.data_ptr(), d_tab[0].data_ptr(), d_tab[1].data_ptr(), n, H, W, prm,
                                out.data_ptr(), out.stride(0) * out.element_size(), out.stride(1) * out.element_size(),
                                status.data_ptr())
    st = status.cpu().tolist()  # synchronises: the pinned staging buffers are free again
    for i, code in enumerate(st):
        if code:
            lib = _lib.load()
            raise _lib.SmError(lib.sm_pngdec_status_code(code),
                               f"png decode: image {i}: {lib.sm_pngdec_status_message(code).decode()}")
    return out


def imdecode_batch(bufs, flags=1, *, device=0, keep_channel_order=False):
    """PNG files of one geometry (a sequence of bytes-like objects) decoded in one call: a CUDA
    tensor ``[N, H, W]`` or ``[N, H, W, 3]`` (``flags`` as in :func:`imdecode`).  A corrupt or
    unsupported file raises ``SmError`` naming its index.  A batch whose first buffer begins
    ``FF D8 FF`` is a batch of JPEG files (:mod:`.jpeg`)."""
    bufs = list(bufs)
    if bufs and _jpeg.is_jpeg(_file_bytes(bufs[0])):
        return _jpeg.decode_batch_device([_file_bytes(b) for b in bufs], flags, device, keep_channel_order)
    return _decode_batch_device(bufs, flags, device, keep_channel_order)


def imdecode(buf, flags=1, *, device=0, as_tensor=False, keep_channel_order=False):
    """``cv2.imdecode(buf, flags)`` for a PNG file in memory (bytes, bytearray, a uint8 array).

    ``flags=1``: BGR uint8 ``[H, W, 3]`` (a gray file replicated, 16-bit samples ``>> 8``, alpha
    dropped; ``keep_channel_order`` leaves the file's RGB).  ``flags=0``: gray uint8 ``[H, W]``; a
    colour file goes through this package's ``bgr2gray`` formula
    ``(1868*B + 9617*G + 4899*R + 8192) >> 14`` -- OpenCV converts inside its decoder and does not
    pin that rounding, so a colour file read with ``flags=0`` may differ from cv2 by one level.
    ``flags=-1``: the file's own channels and depth without alpha (uint16 ``[H, W]`` for a 16-bit
    file).  Returns a numpy array, or with ``as_tensor=True`` a CUDA tensor that stays on the device.
    A corrupt or unsupported file raises ``SmError``.

    A buffer that begins ``FF D8 FF`` is a baseline JPEG file and gives libjpeg-turbo's pixels
    (:mod:`.jpeg`): ``flags=0`` is then the file's Y plane, and the EXIF orientation is not applied."""
    f = _file_bytes(buf)
    if _jpeg.is_jpeg(f):
        if as_tensor:
            return _jpeg.decode_batch_device([f], flags, device, keep_channel_order)[0]
        return _jpeg.decode(f, flags, device, keep_channel_order)
    if as_tensor:
        return _decode_batch_device([buf], flags, device, keep_channel_order)[0]
    prm, shape, dt = _dec_params(_lib.png_info(f), flags, keep_channel_order)
    return _lib.engine(device).png_decode(f, prm, np.empty(shape, dt))


def imdecode_host(buf, flags=1, *, keep_channel_order=False):
    """:func:`imdecode` on the CPU (``sm_png_decode_host``, ``sm_jpeg_decode_host``): the same
    pixels, no device."""
    f = _file_bytes(buf)
    if _jpeg.is_jpeg(f):
        return _jpeg.decode_host(f, flags, keep_channel_order)
    prm, shape, dt = _dec_params(_lib.png_info(f), flags, keep_channel_order)
    return _lib.png_decode_host(f, prm, np.empty(shape, dt))


def imread(filename, flags=1, *, device=0, as_tensor=False):
    """``cv2.imread(filename, flags)`` for PNG and baseline JPEG files (see :func:`imdecode`; the
    content decides, not the extension).  A file that cannot be
    opened gives ``None``, as cv2 does; a corrupt or unsupported one raises ``SmError``."""
    try:
        with open(filename, "rb") as f:
            data = f.read()
    except OSError:
        return None
    return imdecode(data, flags, device=device, as_tensor=as_tensor)


def decode_disparity_png(buf, fmt="kitti", dtype=np.int16, invalid=None, *, device=0, as_tensor=False, host=False):
    """A KITTI disparity PNG (16-bit gray, value = disparity * 256, 0 = invalid) back to a map:
    ``dtype=np.int16`` gives the x16 fixed point ``v >> 4`` (exact for what
    :func:`encode_disparity_png` wrote from an int16 map), ``np.float32`` gives ``v / 256``; a 0
    sample becomes ``invalid`` (default -16, one pixel below zero as the matcher's invalid, and
    -1.0).  ``host=True`` decodes on the CPU."""
    if fmt != "kitti":
        raise ValueError(f"only fmt='kitti' maps are read back, not {fmt!r}")
    if as_tensor and not host:
        return _decode_batch_device([buf], -1, device, False, dtype, invalid)[0]
    f = _file_bytes(buf)
    prm, shape, dt = _dec_params(_lib.png_info(f), -1, False, dtype, invalid)
    out = np.empty(shape, dt)
    return _lib.png_decode_host(f, prm, out) if host else _lib.engine(device).png_decode(f, prm, out)


def read_disparity_png(filename, fmt="kitti", dtype=np.int16, invalid=None, *, device=0, as_tensor=False):
    """:func:`decode_disparity_png` of a file."""
    with open(filename, "rb") as f:
        data = f.read()
    return decode_disparity_png(data, fmt, dtype, invalid, device=device, as_tensor=as_tensor)

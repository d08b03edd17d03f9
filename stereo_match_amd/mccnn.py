"""The MC-CNN *fast* matching cost on the GPU: two gray images to the float32
cost volume :meth:`StereoSGBM.computeFromCost` takes -- what the reference makes with
``./main.lua kitti fast -a predict ... -disp_max 228`` (``mc_cnn/script.py:9``, Torch7 + CUDA) and
reopens as a memmap (``mapTo3D_mc_cnn.py:71``).

The network is the fast architecture of Žbontar & LeCun as the paper states it: ``L`` convolutions
3x3 with 64 feature maps and zero padding, ReLU after all but the last, the 64 features of a pixel
scaled to unit length, and the cost of a pixel pair minus their dot product.  mc-cnn's own code is
not available to this package, so parity with its output is **not** pinned; what is pinned is that
the device and the CPU twin (``host=True``) give the same bits, and that the twin agrees with
torch's ``conv2d`` to float32 accuracy.

No trained weights ship with this package.  :meth:`McCnnFast.random` gives He-scaled random ones
(tests, timing); a trained net comes from an ``.npz`` with the keys ``w0, b0, w1, b1, ...``:
``w0`` float32 ``[64, 1, 3, 3]``, ``w1..`` ``[64, 64, 3, 3]`` (output map, input map, row,
column: ``nn.SpatialConvolution.weight`` viewed as ``[nOutputPlane, nInputPlane, kH, kW]``) and
``b_i`` ``[64]``, which is what a user converts the ``.t7`` net's layers to.
"""
from __future__ import annotations

import numpy as np

from . import _lib

FEATURES = 64
MAX_LAYERS = 6
MAX_DISPARITIES = 256


def _is_torch_cuda(x) -> bool:
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


class McCnnFast:
    """``McCnnFast(weights, biases)``: ``L`` = 1..6 layers (``kitti fast`` has 4, ``mb fast`` 5).
    The arrays are copied and the copies (``.weights``, ``.biases``) are read-only."""

    def __init__(self, weights, biases, device: int = 0):
        weights, biases = list(weights), list(biases)
        L = len(weights)
        if not 1 <= L <= MAX_LAYERS or len(biases) != L:
            raise ValueError(f"{L} weight and {len(biases)} bias arrays: 1 .. {MAX_LAYERS} layers, one bias each")
        self.weights, self.biases = [], []
        for i, (w, b) in enumerate(zip(weights, biases)):
            w, b = np.asarray(w), np.asarray(b)
            if w.dtype != np.float32 or b.dtype != np.float32:
                raise ValueError(f"layer {i}: weights and biases must be float32, not {w.dtype} / {b.dtype}")
            want = (FEATURES, 1 if i == 0 else FEATURES, 3, 3)
            if w.shape != want or b.shape != (FEATURES,):
                raise ValueError(f"layer {i}: weights {w.shape} / biases {b.shape}, expected {want} / ({FEATURES},)")
            # private read-only copies: the device keeps what was uploaded for this object, so a
            # changed net is a new McCnnFast
            for dst, arr in ((self.weights, w), (self.biases, b)):
                arr = np.array(arr, dtype=np.float32, order="C")
                arr.setflags(write=False)
                dst.append(arr)
        self.layers = L
        self.device = int(device)

    @classmethod
    def from_npz(cls, path, device: int = 0):
        """The net stored under the keys ``w0, b0, w1, b1, ...`` (module docstring)."""
        with np.load(path) as z:
            L = 0
            while f"w{L}" in z.files:
                L += 1
            return cls([z[f"w{i}"] for i in range(L)], [z[f"b{i}"] for i in range(L)], device)

    @classmethod
    def random(cls, layers: int = 4, seed: int = 0, device: int = 0):
        """He-scaled random weights (std sqrt(2 / fan_in)), small random biases: untrained."""
        rng = np.random.default_rng(seed)
        ws, bs = [], []
        for i in range(int(layers)):
            cin = 1 if i == 0 else FEATURES
            ws.append((rng.standard_normal((FEATURES, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
            bs.append((rng.standard_normal(FEATURES) * 0.05).astype(np.float32))
        return cls(ws, bs, device)

    def save_npz(self, path):
        np.savez(path, **{f"w{i}": w for i, w in enumerate(self.weights)},
                 **{f"b{i}": b for i, b in enumerate(self.biases)})

    # ---- plumbing
    def _engine(self, device=None):
        eng = _lib.engine(self.device if device is None else device)
        if getattr(eng, "_mccnn_model", None) is not self:
            eng.mccnn_set_weights(self.weights, self.biases)
            eng._mccnn_model = self
        return eng

    @staticmethod
    def _np_images(img):
        a = np.asarray(img)
        if a.dtype != np.uint8:
            raise ValueError(f"images must be uint8 gray, not {a.dtype}")
        if a.ndim not in (2, 3) or a.size == 0:
            raise ValueError(f"images must be non-empty [H, W] or [N, H, W], not {a.shape}")
        return a, a.ndim == 2

    @staticmethod
    def _strided(a3):
        """(array to pass, image_stride, row_stride) of a uint8 [N, H, W] view with unit column stride."""
        if a3.strides[2] != 1 or a3.strides[1] < a3.shape[2] or (a3.shape[0] > 1 and a3.strides[0] < a3.strides[1] * (a3.shape[1] - 1) + a3.shape[2]):
            a3 = np.ascontiguousarray(a3)
        return a3, a3.strides[0], a3.strides[1]

    @staticmethod
    def _check_planes(D):
        D = int(D)
        if not 1 <= D <= MAX_DISPARITIES:
            raise ValueError(f"numDisparities {D}: 1 .. {MAX_DISPARITIES}")
        return D

    @staticmethod
    def _check_offset(m):
        m = int(m)
        if not -2**31 <= m < 2**31:
            raise ValueError(f"minDisparity {m} is no int32")
        return m

    @staticmethod
    def _torch_images(t):
        """(uint8 [N, H, W] view or packed copy the C-ABI can address, whether ``t`` was one image)."""
        import torch

        if t.dtype != torch.uint8 or t.dim() not in (2, 3) or t.numel() == 0:
            raise ValueError("images must be non-empty uint8 gray tensors [H, W] or [N, H, W]")
        single = t.dim() == 2
        t3 = t[None] if single else t
        if t3.stride(2) != 1 or t3.stride(1) < t3.shape[2] or (t3.shape[0] > 1 and t3.stride(0) < t3.stride(1) * (t3.shape[1] - 1) + t3.shape[2]):
            t3 = t3.contiguous()
        return t3, single

    def _torch_features(self, t):
        import torch

        t3, single = self._torch_images(t)
        n, H, W = t3.shape
        eng = self._engine(t.device.index or 0)
        eng.set_stream(torch.cuda.current_stream(t.device).cuda_stream)
        feat = torch.empty((n, H, W, FEATURES), dtype=torch.float32, device=t.device)
        eng.mccnn_features_device(t3.data_ptr(), n, t3.stride(0), H, W, t3.stride(1), feat.data_ptr())
        return feat, single, eng

    # ---- public
    def features(self, img, host: bool = False):
        """Unit-length features, float32 ``[H, W, 64]`` (``[N, H, W, 64]`` for a batch), channel
        last.  ``img``: uint8 gray, numpy (rows may be strided) or a torch CUDA tensor (the result
        is a CUDA tensor, enqueued on torch's current stream).  A constant image raises ValueError.
        ``host=True``: the CPU twin (numpy only)."""
        if _is_torch_cuda(img):
            if host:
                raise ValueError("host=True takes numpy images")
            feat, single, _ = self._torch_features(img)
            return feat[0] if single else feat
        a, single = self._np_images(img)
        a3 = a[None] if single else a
        n, H, W = a3.shape
        if host:
            a3, istride, rstride = self._strided(a3)
            feat = _lib.mccnn_features_host(self.weights, self.biases, a3, istride, rstride, n, H, W)
        else:
            feat = self._engine().mccnn_features(np.ascontiguousarray(a3))
        return feat[0] if single else feat

    def join(self, feat_a, feat_b, numDisparities, minDisparity: int = 0, host: bool = False):
        """The volume ``(N, D, H, W)`` of two feature maps ``[H, W, 64]`` or ``[N, H, W, 64]``: plane
        d at (y, x) is ``-dot(feat_a[y, x], feat_b[y, x - (minDisparity + d)])``, NaN where that
        column is outside the image."""
        D, m = self._check_planes(numDisparities), self._check_offset(minDisparity)
        if _is_torch_cuda(feat_a) or _is_torch_cuda(feat_b):
            import torch

            if host:
                raise ValueError("host=True takes numpy features")
            if (not (_is_torch_cuda(feat_a) and _is_torch_cuda(feat_b)) or feat_a.shape != feat_b.shape
                    or feat_a.dtype != torch.float32 or feat_b.dtype != torch.float32 or feat_a.device != feat_b.device
                    or feat_a.dim() not in (3, 4) or feat_a.shape[-1] != FEATURES):
                raise ValueError("features must be two float32 CUDA tensors [H, W, 64] or [N, H, W, 64] of one shape")
            fa, fb = feat_a.contiguous(), feat_b.contiguous()
            n, H, W = (1,) + tuple(fa.shape[:2]) if fa.dim() == 3 else tuple(fa.shape[:3])
            eng = _lib.engine(fa.device.index or 0)
            eng.set_stream(torch.cuda.current_stream(fa.device).cuda_stream)
            vol = torch.empty((n, D, H, W), dtype=torch.float32, device=fa.device)
            eng.mccnn_join_device(fa.data_ptr(), fb.data_ptr(), n, H, W, D, m, vol.data_ptr())
            return vol
        fa, fb = np.asarray(feat_a), np.asarray(feat_b)
        if (fa.shape != fb.shape or fa.dtype != np.float32 or fb.dtype != np.float32 or fa.ndim not in (3, 4)
                or fa.shape[-1] != FEATURES or fa.size == 0):
            raise ValueError("features must be two float32 arrays [H, W, 64] or [N, H, W, 64] of one shape")
        if fa.ndim == 3:
            fa, fb = fa[None], fb[None]
        fa, fb = np.ascontiguousarray(fa), np.ascontiguousarray(fb)
        if host:
            return _lib.mccnn_join_host(fa, fb, D, m)
        return _lib.engine(self.device).mccnn_join(fa, fb, D, m)

    def cost_volume(self, a, b, numDisparities, minDisparity: int = 0, host: bool = False):
        """float32 ``(1, D, H, W)`` (``(N, D, H, W)`` for batches), d-major: exactly what
        :meth:`StereoSGBM.computeFromCost` documents.  Plane d is the cost of ``a``'s x against
        ``b``'s x - (minDisparity + d); costs lie in [-1, 1] (``computeFromCost(vol, 1.0, 2047.5)``
        is the fixed quantisation window), NaN outside the image.  numpy in -> numpy out; torch
        CUDA tensors in -> a CUDA tensor on torch's current stream.  ``host=True``: the twin.  On
        the device this is the fused entry point (``sm_mccnn_volume[_device]``: both feature passes
        and the join in one call, the feature maps in the context's own buffers); it gives the bits
        of :meth:`features` + :meth:`join`."""
        D, m = self._check_planes(numDisparities), self._check_offset(minDisparity)
        if _is_torch_cuda(a) or _is_torch_cuda(b):
            import torch

            if host:
                raise ValueError("host=True takes numpy images")
            if not (_is_torch_cuda(a) and _is_torch_cuda(b)) or a.device != b.device:
                raise ValueError("both images must be numpy arrays or both CUDA tensors on one device")
            if a.shape != b.shape:
                raise ValueError("the two images must have the same shape")
            a3, b3 = self._torch_images(a)[0], self._torch_images(b)[0]
            if a3.stride() != b3.stride():  # the entry point takes one geometry for both
                a3, b3 = a3.contiguous(), b3.contiguous()
            n, H, W = a3.shape
            eng = self._engine(a.device.index or 0)
            eng.set_stream(torch.cuda.current_stream(a.device).cuda_stream)
            vol = torch.empty((n, D, H, W), dtype=torch.float32, device=a.device)
            eng.mccnn_volume_device(a3.data_ptr(), b3.data_ptr(), n, a3.stride(0), H, W, a3.stride(1), D, m,
                                    vol.data_ptr())
            return vol
        a, _ = self._np_images(a)
        b, _ = self._np_images(b)
        if a.shape != b.shape:
            raise ValueError("the two images must have the same shape")
        if host:
            return self.join(self.features(a, host=True), self.features(b, host=True), D, m, host=True)
        a3, b3 = (np.ascontiguousarray(v[None] if v.ndim == 2 else v) for v in (a, b))
        return self._engine().mccnn_volume(a3, b3, D, m)

    def cost_volumes(self, left, right, matcher, host: bool = False):
        """``(volume for matcher, volume for createRightMatcher(matcher))``: the features of both
        images are computed once.  The right matcher's volume is the same function with the images
        swapped and ``minDisparity = -(minDisparity + numDisparities) + 1``."""
        D, m = int(matcher.numDisparities), int(matcher.minDisparity)
        self._check_planes(D)
        if _is_torch_cuda(left) != _is_torch_cuda(right):
            raise ValueError("both images must be numpy arrays or both torch CUDA tensors")
        if not _is_torch_cuda(left):
            left, right = self._np_images(left)[0], self._np_images(right)[0]
        if tuple(left.shape) != tuple(right.shape):
            raise ValueError("the two images must have the same shape")
        fl, fr = self.features(left, host=host), self.features(right, host=host)
        return self.join(fl, fr, D, m, host=host), self.join(fr, fl, D, -(m + D) + 1, host=host)

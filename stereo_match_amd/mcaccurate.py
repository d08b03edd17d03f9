"""The MC-CNN *accurate* matching cost on the GPU: two gray images to the float32
cost volume :meth:`StereoSGBM.computeFromCost` and :class:`McCnnStereo` take -- what the reference
makes with ``./main.lua mb slow -a predict ... -disp_max 228`` (``mc_cnn/script.py:10``).

The network is the accurate architecture of Žbontar & LeCun (JMLR 2016, §3.2) as the paper states
it: ``L`` convolutions 3x3 with 112 feature maps, zero padding and a ReLU after every one, no
unit-length step; the two 112-vectors of a pixel pair concatenated (left image first) through ``F``
fully connected layers of ``U`` units with ReLU, one linear unit and a sigmoid; the cost is minus
that similarity, in [-1, 0].  mc-cnn's own code is not available to this package, so parity with
its output is **not** pinned (the concatenation order and the layer counts are as recalled); what
is pinned is that the device and the CPU twin (``host=True``) give the same bits, and that the twin
agrees with torch's ``conv2d`` / ``linear`` / ``sigmoid`` to float32 accuracy.

No trained weights ship with this package.  :meth:`McCnnAccurate.random` gives He-scaled random
ones; a trained net comes from an ``.npz`` with the keys ``w{i}, b{i}`` (``w0`` float32
``[112, 1, 3, 3]``, ``w1..`` ``[112, 112, 3, 3]``, ``b_i`` ``[112]``) and ``fw{i}, fb{i}``
(``nn.Linear``'s ``[out, in]``: ``fw0`` ``[U, 224]``, ``fw1..`` ``[U, U]``, the last ``[1, U]``;
``fb_i`` ``[U]``, the last ``[1]``).

``precision="bf16"`` runs the scorer's hidden layers 1 .. F-1 on the bfloat16
matrix instruction: the activations entering a layer and its weights are rounded to bfloat16
(nearest, ties to even), every unit's sum is accumulated in float32 from its float32 bias.  The
feature net, the first layer (the two projections and their add), the output unit, the sigmoid and
the NaN border stay float32.  The default ``"f32"`` is the arithmetic above, bit for bit.  In bf16
mode the device and the twin agree bit for bit where every sum is exact (integer nets) and to the
order of the float32 additions otherwise.  With no trained weights, the effect of bf16 on real
disparities is unknown.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .mccnn import MAX_DISPARITIES, McCnnFast, _is_torch_cuda

FEATURES = 112
MAX_LAYERS = 6
MAX_FC_LAYERS = 4
MAX_UNITS = 384
PRECISIONS = ("f32", "bf16")


def _frozen(arr):
    arr = np.array(arr, dtype=np.float32, order="C")
    arr.setflags(write=False)
    return arr


class McCnnAccurate:
    """``McCnnAccurate(conv_w, conv_b, fc_w, fc_b)``: ``L`` = 1..6 convolutions and ``F`` = 1..4
    hidden fully connected layers of ``U`` units (a multiple of 32, 32..384) followed by the output
    unit, so ``fc_w`` and ``fc_b`` hold ``F + 1`` arrays.  The arrays are copied and the copies
    (``.weights``, ``.biases``, ``.fc_weights``, ``.fc_biases``) are read-only."""

    def __init__(self, conv_w, conv_b, fc_w, fc_b, device: int = 0, precision: str = "f32"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision {precision!r}: one of {PRECISIONS}")
        conv_w, conv_b, fc_w, fc_b = list(conv_w), list(conv_b), list(fc_w), list(fc_b)
        L, F = len(conv_w), len(fc_w) - 1
        if not 1 <= L <= MAX_LAYERS or len(conv_b) != L:
            raise ValueError(f"{L} weight and {len(conv_b)} bias arrays: 1 .. {MAX_LAYERS} convolutions, one bias each")
        if not 1 <= F <= MAX_FC_LAYERS or len(fc_b) != F + 1:
            raise ValueError(f"{F + 1} scorer weight and {len(fc_b)} bias arrays: 1 .. {MAX_FC_LAYERS} hidden layers "
                             "and the output unit, one bias each")
        self.weights, self.biases, self.fc_weights, self.fc_biases = [], [], [], []
        for i, (w, b) in enumerate(zip(conv_w, conv_b)):
            w, b = np.asarray(w), np.asarray(b)
            if w.dtype != np.float32 or b.dtype != np.float32:
                raise ValueError(f"convolution {i}: weights and biases must be float32, not {w.dtype} / {b.dtype}")
            want = (FEATURES, 1 if i == 0 else FEATURES, 3, 3)
            if w.shape != want or b.shape != (FEATURES,):
                raise ValueError(f"convolution {i}: weights {w.shape} / biases {b.shape}, expected {want} / ({FEATURES},)")
            self.weights.append(_frozen(w))
            self.biases.append(_frozen(b))
        U = np.asarray(fc_w[0]).shape[0] if np.asarray(fc_w[0]).ndim == 2 else 0
        if not 32 <= U <= MAX_UNITS or U % 32:
            raise ValueError(f"{U} units: a multiple of 32, 32 .. {MAX_UNITS}")
        for i, (w, b) in enumerate(zip(fc_w, fc_b)):
            w, b = np.asarray(w), np.asarray(b)
            if w.dtype != np.float32 or b.dtype != np.float32:
                raise ValueError(f"scorer layer {i}: weights and biases must be float32, not {w.dtype} / {b.dtype}")
            out = 1 if i == F else U
            want = (out, 2 * FEATURES if i == 0 else U)
            if w.shape != want or b.shape != (out,):
                raise ValueError(f"scorer layer {i}: weights {w.shape} / biases {b.shape}, expected {want} / ({out},)")
            self.fc_weights.append(_frozen(w))
            self.fc_biases.append(_frozen(b))
        self.layers, self.fc_layers, self.units = L, F, int(U)
        self.device = int(device)
        self._root = self  # the net whose arrays these are: with_precision's copies share one upload
        self._precision = precision
        if precision == "bf16":
            self._check_bf16()

    @property
    def precision(self) -> str:
        """``"f32"`` or ``"bf16"``: the arithmetic of the scorer's hidden layers (read-only)."""
        return self._precision

    def _check_bf16(self):
        for i in range(1, self.fc_layers):
            if ((_lib.mcacc_bf16_host(self.fc_weights[i]) & 0x7F80) == 0x7F80).any():
                raise ValueError(f"scorer layer {i}: a weight is not finite or overflows in bfloat16 (precision='bf16')")

    def with_precision(self, precision: str):
        """A net of the same (shared, read-only) arrays whose scorer runs in ``precision``."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision {precision!r}: one of {PRECISIONS}")
        other = object.__new__(type(self))
        other.__dict__.update(self.__dict__)
        other._precision = precision
        if precision == "bf16":
            other._check_bf16()
        return other

    @classmethod
    def from_npz(cls, path, device: int = 0, precision: str = "f32"):
        """The net stored under the keys ``w{i}, b{i}, fw{i}, fb{i}`` (module docstring)."""
        with np.load(path) as z:
            L = F = 0
            while f"w{L}" in z.files:
                L += 1
            while f"fw{F}" in z.files:
                F += 1
            return cls([z[f"w{i}"] for i in range(L)], [z[f"b{i}"] for i in range(L)],
                       [z[f"fw{i}"] for i in range(F)], [z[f"fb{i}"] for i in range(F)], device, precision)

    @classmethod
    def random(cls, conv_layers: int = 4, fc_layers: int = 4, units: int = 384, seed: int = 0, device: int = 0,
               precision: str = "f32"):
        """He-scaled random weights (std sqrt(2 / fan_in)), small random biases: untrained."""
        rng = np.random.default_rng(seed)
        units = int(units)
        if not 32 <= units <= MAX_UNITS or units % 32:
            raise ValueError(f"{units} units: a multiple of 32, 32 .. {MAX_UNITS}")
        ws, bs, fws, fbs = [], [], [], []
        for i in range(int(conv_layers)):
            cin = 1 if i == 0 else FEATURES
            ws.append((rng.standard_normal((FEATURES, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
            bs.append((rng.standard_normal(FEATURES) * 0.05).astype(np.float32))
        for i in range(int(fc_layers) + 1):
            fan_in = 2 * FEATURES if i == 0 else units
            out = 1 if i == int(fc_layers) else units
            fws.append((rng.standard_normal((out, fan_in)) * np.sqrt(2.0 / fan_in)).astype(np.float32))
            fbs.append((rng.standard_normal(out) * 0.05).astype(np.float32))
        return cls(ws, bs, fws, fbs, device, precision)

    def save_npz(self, path):
        np.savez(path, **{f"w{i}": w for i, w in enumerate(self.weights)}, **{f"b{i}": b for i, b in enumerate(self.biases)},
                 **{f"fw{i}": w for i, w in enumerate(self.fc_weights)}, **{f"fb{i}": b for i, b in enumerate(self.fc_biases)})

    # ---- plumbing (the input conventions are McCnnFast's)
    _np_images = staticmethod(McCnnFast._np_images)
    _strided = staticmethod(McCnnFast._strided)
    _check_planes = staticmethod(McCnnFast._check_planes)
    _check_offset = staticmethod(McCnnFast._check_offset)
    _torch_images = staticmethod(McCnnFast._torch_images)

    def _engine(self, device=None):
        eng = _lib.engine(self.device if device is None else device)
        eng.mcacc_set_precision(self._precision)  # a state of the context: every call sets its own
        if getattr(eng, "_mcacc_model", None) is not self._root:
            eng.mcacc_set_weights(self.weights, self.biases, self.fc_weights, self.fc_biases)
            eng._mcacc_model = self._root
        return eng

    # ---- public
    def features(self, img, host: bool = False):
        """The feature maps, float32 ``[H, W, 112]`` (``[N, H, W, 112]`` for a batch), channel last.
        ``img``: uint8 gray, numpy (rows may be strided) or a torch CUDA tensor (the result is a
        CUDA tensor, enqueued on torch's current stream).  A constant image raises ValueError.
        ``host=True``: the CPU twin (numpy only)."""
        if _is_torch_cuda(img):
            import torch

            if host:
                raise ValueError("host=True takes numpy images")
            t3, single = self._torch_images(img)
            n, H, W = t3.shape
            eng = self._engine(img.device.index or 0)
            eng.set_stream(torch.cuda.current_stream(img.device).cuda_stream)
            feat = torch.empty((n, H, W, FEATURES), dtype=torch.float32, device=img.device)
            eng.mcacc_features_device(t3.data_ptr(), n, t3.stride(0), H, W, t3.stride(1), feat.data_ptr())
            return feat[0] if single else feat
        a, single = self._np_images(img)
        a3 = a[None] if single else a
        n, H, W = a3.shape
        if host:
            a3, istride, rstride = self._strided(a3)
            feat = _lib.mcacc_features_host(self.weights, self.biases, a3, istride, rstride, n, H, W)
        else:
            feat = self._engine().mcacc_features(np.ascontiguousarray(a3))
        return feat[0] if single else feat

    def join(self, feat_a, feat_b, numDisparities, minDisparity: int = 0, a_is_left: bool = True, raw: bool = False,
             host: bool = False):
        """The volume ``(N, D, H, W)`` of two feature maps ``[H, W, 112]`` or ``[N, H, W, 112]``: plane
        d at (y, x) is minus the scorer's similarity of ``feat_a[y, x]`` and
        ``feat_b[y, x - (minDisparity + d)]``, NaN where that column is outside the image.
        ``a_is_left`` says which of the two is the left image's (it multiplies columns 0..111 of
        ``fw0``); ``raw=True`` returns minus the logit, without the sigmoid."""
        D, m = self._check_planes(numDisparities), self._check_offset(minDisparity)
        if _is_torch_cuda(feat_a) or _is_torch_cuda(feat_b):
            import torch

            if host:
                raise ValueError("host=True takes numpy features")
            if (not (_is_torch_cuda(feat_a) and _is_torch_cuda(feat_b)) or feat_a.shape != feat_b.shape
                    or feat_a.dtype != torch.float32 or feat_b.dtype != torch.float32 or feat_a.device != feat_b.device
                    or feat_a.dim() not in (3, 4) or feat_a.shape[-1] != FEATURES or feat_a.numel() == 0):
                raise ValueError("features must be two float32 CUDA tensors [H, W, 112] or [N, H, W, 112] of one shape")
            fa, fb = feat_a.contiguous(), feat_b.contiguous()
            n, H, W = (1,) + tuple(fa.shape[:2]) if fa.dim() == 3 else tuple(fa.shape[:3])
            eng = self._engine(fa.device.index or 0)
            eng.set_stream(torch.cuda.current_stream(fa.device).cuda_stream)
            vol = torch.empty((n, D, H, W), dtype=torch.float32, device=fa.device)
            eng.mcacc_join_device(fa.data_ptr(), fb.data_ptr(), n, H, W, D, m, a_is_left, raw, vol.data_ptr())
            return vol
        fa, fb = np.asarray(feat_a), np.asarray(feat_b)
        if (fa.shape != fb.shape or fa.dtype != np.float32 or fb.dtype != np.float32 or fa.ndim not in (3, 4)
                or fa.shape[-1] != FEATURES or fa.size == 0):
            raise ValueError("features must be two float32 arrays [H, W, 112] or [N, H, W, 112] of one shape")
        if fa.ndim == 3:
            fa, fb = fa[None], fb[None]
        fa, fb = np.ascontiguousarray(fa), np.ascontiguousarray(fb)
        if host:
            return _lib.mcacc_join_host(self.fc_weights, self.fc_biases, fa, fb, D, m, a_is_left, raw, self._precision)
        return self._engine().mcacc_join(fa, fb, D, m, a_is_left, raw)

    def cost_volume(self, a, b, numDisparities, minDisparity: int = 0, a_is_left: bool = True, raw: bool = False,
                    host: bool = False):
        """float32 ``(1, D, H, W)`` (``(N, D, H, W)`` for batches), d-major: exactly what
        :meth:`StereoSGBM.computeFromCost` documents.  Plane d is the cost of ``a``'s x against
        ``b``'s x - (minDisparity + d); costs lie in [-1, 0] (``computeFromCost(vol, 1.0, 4095.0)``
        is the fixed quantisation window), NaN outside the image.  numpy in -> numpy out; torch
        CUDA tensors in -> a CUDA tensor on torch's current stream.  ``host=True``: the twin.  On
        the device this is the fused entry point (``sm_mcacc_volume[_device]``); it gives the bits
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
            eng.mcacc_volume_device(a3.data_ptr(), b3.data_ptr(), n, a3.stride(0), H, W, a3.stride(1), D, m, a_is_left, raw,
                                    vol.data_ptr())
            return vol
        a, _ = self._np_images(a)
        b, _ = self._np_images(b)
        if a.shape != b.shape:
            raise ValueError("the two images must have the same shape")
        if host:
            return self.join(self.features(a, host=True), self.features(b, host=True), D, m, a_is_left, raw, host=True)
        a3, b3 = (np.ascontiguousarray(v[None] if v.ndim == 2 else v) for v in (a, b))
        return self._engine().mcacc_volume(a3, b3, D, m, a_is_left, raw)

    def cost_volumes(self, left, right, matcher, host: bool = False):
        """``(volume for matcher, volume for createRightMatcher(matcher))``: the features of both
        images are computed once.  The right matcher's volume is the right image against the left
        one with ``a_is_left=False`` and ``minDisparity = -(minDisparity + numDisparities) + 1``:
        it pairs the same columns through the same two projections as the left one."""
        D, m = int(matcher.numDisparities), int(matcher.minDisparity)
        self._check_planes(D)
        if _is_torch_cuda(left) != _is_torch_cuda(right):
            raise ValueError("both images must be numpy arrays or both torch CUDA tensors")
        if not _is_torch_cuda(left):
            left, right = self._np_images(left)[0], self._np_images(right)[0]
        if tuple(left.shape) != tuple(right.shape):
            raise ValueError("the two images must have the same shape")
        fl, fr = self.features(left, host=host), self.features(right, host=host)
        return (self.join(fl, fr, D, m, True, host=host), self.join(fr, fl, D, -(m + D) + 1, False, host=host))


__all__ = ["McCnnAccurate", "PRECISIONS", "FEATURES", "MAX_LAYERS", "MAX_FC_LAYERS", "MAX_UNITS", "MAX_DISPARITIES"]

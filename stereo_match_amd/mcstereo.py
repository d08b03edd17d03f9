"""MC-CNN's stereo method after the matching cost: cross-based cost
aggregation (optional), semi-global matching on the float32 volume of :class:`McCnnFast` or
:class:`McCnnAccurate` with
penalties that follow the intensity steps of both images, left-right interpolation, the sub-pixel
step, a 5x5 median and a bilateral filter -- what turns the network's output into the ``left.png``
/ ``right.png`` that ``mapTo3D_mc_cnn.py:70-77`` reads.

This is §4 of Žbontar & LeCun (JMLR 2016) restated; mc-cnn's own code is not available to this
package, so parity with its output is **not** pinned (its cross-based aggregation may average the
two axes one after the other where this one sums over the region, as the paper's equation does),
and the default values are the paper's KITTI fast ones (:class:`McCnnStereoParams`) and KITTI
accurate ones (:class:`McCnnCrossParams`) as recalled (unverified).  What is pinned: the device and
the CPU twin (``host=True``) give the same values, and the twin equals an independent numpy
restatement.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib
from .mcaccurate import McCnnAccurate
from .mccnn import MAX_DISPARITIES, McCnnFast, _is_torch_cuda

MAX_OFFSET = 1 << 23
FLOAT32_MAX = float(np.finfo(np.float32).max)
STAGES = _lib.MCSGM_STAGES  # wta_left, wta_right, status, filled (int32), subpixel, median (float32)


@dataclasses.dataclass(frozen=True)
class McCnnStereoParams:
    """The method's numbers; every one is rounded to float32 on its way to the kernels.  ``pi1`` and
    ``pi2`` may be 0 (no smoothing), everything else must be positive and finite."""
    pi1: float = 4.0
    pi2: float = 55.72
    sgm_q1: float = 3.0
    sgm_q2: float = 2.5
    sgm_v: float = 1.5
    sgm_d: float = 0.02
    sgm_i: int = 1
    blur_sigma: float = 7.74
    blur_t: float = 5.0

    def __post_init__(self):
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if f.name == "sgm_i":
                if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= 16:
                    raise ValueError(f"sgm_i {v!r}: an integer 1 .. 16")
                continue
            v = float(v)
            lowest_ok = v >= 0.0 if f.name in ("pi1", "pi2") else v > 0.0
            if not math.isfinite(v) or not lowest_ok or v > FLOAT32_MAX:
                raise ValueError(f"{f.name} {v!r} must be finite and positive")
        if math.ceil(3.0 * float(np.float32(self.blur_sigma))) > 48:
            raise ValueError(f"blur_sigma {self.blur_sigma}: the window radius ceil(3 sigma) is at most 48")

    def c_struct(self) -> "_lib.SmMcsgmParams":
        return _lib.SmMcsgmParams(self.pi1, self.pi2, self.sgm_q1, self.sgm_q2, self.sgm_v, self.sgm_d, int(self.sgm_i),
                                  self.blur_sigma, self.blur_t)


@dataclasses.dataclass(frozen=True)
class McCnnCrossParams:
    """Cross-based cost aggregation: an arm grows while it stays inside the image,
    is shorter than ``l1`` and the pixel differs from the arm's origin by less than ``tau1`` (on the
    normalised image; rounded to float32); ``i1`` iterations run before the semi-global matching
    and ``i2`` after it.  The defaults are the paper's KITTI accurate values as recalled
    (unverified)."""
    l1: int = 5
    tau1: float = 0.13
    i1: int = 2
    i2: int = 0

    def __post_init__(self):
        for name, lo, hi in (("l1", 1, 32), ("i1", 0, 16), ("i2", 0, 16)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer, float)) or int(v) != v or not lo <= int(v) <= hi:
                raise ValueError(f"{name} {v!r}: an integer {lo} .. {hi}")
        t = float(self.tau1)
        if not math.isfinite(t) or not t > 0.0 or t > FLOAT32_MAX or float(np.float32(t)) == 0.0:
            raise ValueError(f"tau1 {self.tau1!r} must be finite and positive")

    def c_struct(self) -> "_lib.SmMccbcaParams":
        return _lib.SmMccbcaParams(int(self.l1), self.tau1, int(self.i1), int(self.i2))


def right_min_disparity(numDisparities: int, minDisparity: int) -> int:
    """``minDisparity`` of the right view's volume: ``-(minDisparity + numDisparities) + 1``."""
    return -(int(minDisparity) + int(numDisparities)) + 1


def _params(params):
    if params is None:
        return McCnnStereoParams()
    if not isinstance(params, McCnnStereoParams):
        raise ValueError("params must be a McCnnStereoParams")
    return params


def _cross_params(params):
    if params is None:
        return McCnnCrossParams()
    if not isinstance(params, McCnnCrossParams):
        raise ValueError("params must be a McCnnCrossParams")
    return params


def _iterations(n):
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= 16:
        raise ValueError(f"iterations {n!r}: an integer 1 .. 16")
    return int(n)


def _offset(m):
    m = int(m)
    if not -2**31 <= m < 2**31:
        raise ValueError(f"minDisparity {m} is no int32")
    return m


def _np_volume(vol, what):
    v = np.asarray(vol)
    if v.dtype != np.float32 or v.ndim not in (3, 4) or v.size == 0:
        raise ValueError(f"{what} must be a non-empty float32 array [D, H, W] or [N, D, H, W]")
    v4 = np.ascontiguousarray(v[None] if v.ndim == 3 else v)
    if not 1 <= v4.shape[1] <= MAX_DISPARITIES:
        raise ValueError(f"{what} has {v4.shape[1]} planes: 1 .. {MAX_DISPARITIES}")
    return v4, v.ndim == 3


def _np_images(img, shape, what):
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise ValueError(f"{what} must be uint8 gray, not {a.dtype}")
    a3 = a[None] if a.ndim == 2 else a
    if a3.ndim != 3 or a3.shape != shape:
        raise ValueError(f"{what} has shape {a.shape}; the volume needs {shape}")
    return a3


def _torch_volume(t, what):
    import torch

    if t.dtype != torch.float32 or t.dim() not in (3, 4) or t.numel() == 0:
        raise ValueError(f"{what} must be a non-empty float32 CUDA tensor [D, H, W] or [N, D, H, W]")
    t4 = (t[None] if t.dim() == 3 else t).contiguous()
    if not 1 <= t4.shape[1] <= MAX_DISPARITIES:
        raise ValueError(f"{what} has {t4.shape[1]} planes: 1 .. {MAX_DISPARITIES}")
    return t4, t.dim() == 3


def _torch_images(imgs, shape, device):
    """uint8 [N, H, W] views or packed copies of one geometry that the C-ABI can address."""
    out = []
    for t in imgs:
        if not _is_torch_cuda(t) or t.device != device:
            raise ValueError("volumes and images must all be CUDA tensors on one device (or all numpy)")
        t3 = McCnnFast._torch_images(t)[0]
        if tuple(t3.shape) != shape:
            raise ValueError(f"an image has shape {tuple(t.shape)}; the volume needs {shape}")
        out.append(t3)
    if any(t.stride() != out[0].stride() for t in out):
        out = [t.contiguous() for t in out]
    return out


def mc_aggregate(vol, a, b, minDisparity: int = 0, params: McCnnStereoParams = None, host: bool = False):
    """The four-path aggregation of ``vol`` (float32 ``[D, H, W]`` or ``[N, D, H, W]``, what
    ``McCnnFast.cost_volume(a, b, D, minDisparity)`` returns): ``a`` is the view's own uint8 image,
    ``b`` the other one.  Returns a new volume of the same shape; numpy in -> numpy out, CUDA tensors
    stay on the device on torch's current stream.  ``host=True``: the CPU twin (numpy only)."""
    prm, m = _params(params).c_struct(), _offset(minDisparity)
    if _is_torch_cuda(vol):
        import torch

        if host:
            raise ValueError("host=True takes numpy arrays")
        v4, single = _torch_volume(vol, "vol")
        n, D, H, W = v4.shape
        a3, b3 = _torch_images((a, b), (n, H, W), v4.device)
        eng = _lib.engine(v4.device.index or 0)
        eng.set_stream(torch.cuda.current_stream(v4.device).cuda_stream)
        agg = torch.empty_like(v4)
        eng.mcsgm_aggregate_device(v4.data_ptr(), a3.data_ptr(), b3.data_ptr(), n, a3.stride(0), H, W, a3.stride(1), D, m,
                                   prm, agg.data_ptr())
        return agg[0] if single else agg
    v4, single = _np_volume(vol, "vol")
    n, D, H, W = v4.shape
    a3, b3 = (np.ascontiguousarray(_np_images(x, (n, H, W), w)) for x, w in ((a, "a"), (b, "b")))
    if host:
        agg = _lib.mcsgm_aggregate_host(v4, a3, b3, H * W, W, m, prm)
    else:
        agg = _lib.engine(0).mcsgm_aggregate(v4, a3, b3, m, prm)
    return agg[0] if single else agg


def mc_cross_arms(img, params: McCnnCrossParams = None, host: bool = False):
    """The arms of every pixel of ``img`` (uint8 ``[H, W]`` or ``[N, H, W]``): uint8 ``[4, H, W]``
    (``[N, 4, H, W]``) in the order left, right, up, down.  numpy in -> numpy out, a CUDA tensor
    stays on the device on torch's current stream.  ``host=True``: the CPU twin (numpy only)."""
    prm = _cross_params(params).c_struct()
    if _is_torch_cuda(img):
        import torch

        if host:
            raise ValueError("host=True takes numpy arrays")
        t3 = McCnnFast._torch_images(img)[0]
        n, H, W = t3.shape
        eng = _lib.engine(t3.device.index or 0)
        eng.set_stream(torch.cuda.current_stream(t3.device).cuda_stream)
        arms = torch.empty((n, 4, H, W), dtype=torch.uint8, device=t3.device)
        eng.mccbca_arms_device(t3.data_ptr(), n, t3.stride(0), H, W, t3.stride(1), prm, arms.data_ptr())
        return arms[0] if img.dim() == 2 else arms
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.size == 0:
        raise ValueError("img must be a non-empty uint8 gray array [H, W] or [N, H, W]")
    a3 = np.ascontiguousarray(a[None] if a.ndim == 2 else a)
    n, H, W = a3.shape
    arms = _lib.mccbca_arms_host(a3, H * W, W, prm) if host else _lib.engine(0).mccbca_arms(a3, prm)
    return arms[0] if a.ndim == 2 else arms


def mc_cross_aggregate(vol, a, b, minDisparity: int = 0, params: McCnnCrossParams = None, iterations: int = 1,
                       host: bool = False):
    """``iterations`` steps of the cross-based cost aggregation of ``vol`` (float32 ``[D, H, W]`` or
    ``[N, D, H, W]``, what ``McCnnFast.cost_volume(a, b, D, minDisparity)`` returns): ``a`` is the view's
    own uint8 image, ``b`` the other one.  Uses ``l1`` and ``tau1`` of ``params``.  Returns a new volume
    of the same shape; numpy in -> numpy out, CUDA tensors stay on the device on torch's current
    stream.  ``host=True``: the CPU twin (numpy only)."""
    prm, m, it = _cross_params(params).c_struct(), _offset(minDisparity), _iterations(iterations)
    if _is_torch_cuda(vol):
        import torch

        if host:
            raise ValueError("host=True takes numpy arrays")
        v4, single = _torch_volume(vol, "vol")
        n, D, H, W = v4.shape
        a3, b3 = _torch_images((a, b), (n, H, W), v4.device)
        eng = _lib.engine(v4.device.index or 0)
        eng.set_stream(torch.cuda.current_stream(v4.device).cuda_stream)
        agg = torch.empty_like(v4)
        eng.mccbca_aggregate_device(v4.data_ptr(), a3.data_ptr(), b3.data_ptr(), n, a3.stride(0), H, W, a3.stride(1), D, m,
                                    prm, it, agg.data_ptr())
        return agg[0] if single else agg
    v4, single = _np_volume(vol, "vol")
    n, D, H, W = v4.shape
    a3, b3 = (np.ascontiguousarray(_np_images(x, (n, H, W), w)) for x, w in ((a, "a"), (b, "b")))
    if host:
        agg = _lib.mccbca_aggregate_host(v4, a3, b3, H * W, W, m, prm, it)
    else:
        agg = _lib.engine(0).mccbca_aggregate(v4, a3, b3, m, prm, it)
    return agg[0] if single else agg


def mc_disparity(agg_l, agg_r, a_l, minDisparity: int = 0, params: McCnnStereoParams = None, host: bool = False,
                 stages: bool = False):
    """The left view's disparity map, float32 ``[H, W]`` (``[N, H, W]`` for batches), from the two
    aggregated volumes (``agg_r`` the right view's, made with :func:`right_min_disparity`) and the
    left image; invalid pixels are ``float(minDisparity - 1)``.  ``stages=True`` returns
    ``(disparity, maps)`` with the maps of :data:`STAGES`: the integer disparities of both views
    after winner-take-all, the status of every left pixel (0 correct, 1 mismatch, 2 occluded), the
    interpolated map, and the maps after the sub-pixel step and the median."""
    p = _params(params)
    prm, m = p.c_struct(), _offset(minDisparity)
    if _is_torch_cuda(agg_l):
        import torch

        if host:
            raise ValueError("host=True takes numpy arrays")
        l4, single = _torch_volume(agg_l, "agg_l")
        if not _is_torch_cuda(agg_r) or agg_r.device != l4.device or tuple(agg_r.shape) != tuple(agg_l.shape):
            raise ValueError("agg_r must be a CUDA tensor of agg_l's shape on its device")
        r4 = _torch_volume(agg_r, "agg_r")[0]
        n, D, H, W = l4.shape
        _check_offset_range(m, D)
        (a3,) = _torch_images((a_l,), (n, H, W), l4.device)
        eng = _lib.engine(l4.device.index or 0)
        eng.set_stream(torch.cuda.current_stream(l4.device).cuda_stream)
        disp = torch.empty((n, H, W), dtype=torch.float32, device=l4.device)
        maps, st = None, None
        if stages:
            maps = {k: torch.empty((n, H, W), dtype=torch.int32 if k in _lib.MCSGM_INT_STAGES else torch.float32,
                                   device=l4.device) for k in STAGES}
            st = _lib.SmMcsgmStages(*[maps[k].data_ptr() for k in STAGES])
        eng.mcsgm_disparity_device(l4.data_ptr(), r4.data_ptr(), a3.data_ptr(), n, a3.stride(0), H, W, a3.stride(1), D, m,
                                   prm, disp.data_ptr(), st)
    else:
        l4, single = _np_volume(agg_l, "agg_l")
        r4 = _np_volume(agg_r, "agg_r")[0]
        if r4.shape != l4.shape:
            raise ValueError("agg_r must have agg_l's shape")
        n, D, H, W = l4.shape
        _check_offset_range(m, D)
        a3 = np.ascontiguousarray(_np_images(a_l, (n, H, W), "a_l"))
        if host:
            disp, maps = _lib.mcsgm_disparity_host(l4, r4, a3, H * W, W, m, prm, stages)
        else:
            disp, maps = _lib.engine(0).mcsgm_disparity(l4, r4, a3, m, prm, stages)
    if single:
        disp = disp[0]
        maps = {k: v[0] for k, v in maps.items()} if maps else maps
    return (disp, maps) if stages else disp


def _check_offset_range(m, D):
    if m < -MAX_OFFSET or m + D > MAX_OFFSET:
        raise ValueError(f"minDisparity {m} with {D} planes leaves [-2^23, 2^23]")


class McCnnStereo:
    """``McCnnStereo(net, params, cross).compute(left, right, numDisparities, minDisparity=0)``
    (``net`` a :class:`McCnnFast` or a :class:`McCnnAccurate`): the features once, the volumes of
    both views, both aggregations, the disparity.  ``cross`` (a
    :class:`McCnnCrossParams`; None: none) adds the cross-based cost aggregation to both views: ``i1``
    iterations before the semi-global matching and ``i2`` after it.  Returns
    ``(disp_left, disp_right_wta)``: the finished left map and the right view's winner-take-all
    disparities as float32 (what the left-right check compared against), both with invalid pixels at
    ``float(minDisparity - 1)``."""

    def __init__(self, net, params: McCnnStereoParams = None, cross: McCnnCrossParams = None):
        if not isinstance(net, (McCnnFast, McCnnAccurate)):
            raise ValueError("net must be a McCnnFast or a McCnnAccurate")
        self.net, self.params = net, _params(params)
        self.cross = None if cross is None else _cross_params(cross)

    def _aggregate(self, vol, a, b, m, host):
        """One view: i1 cross-based iterations, the semi-global matching, i2 more."""
        cross = self.cross
        if cross is not None and cross.i1:
            vol = mc_cross_aggregate(vol, a, b, m, cross, cross.i1, host=host)
        vol = mc_aggregate(vol, a, b, m, self.params, host=host)
        if cross is not None and cross.i2:
            vol = mc_cross_aggregate(vol, a, b, m, cross, cross.i2, host=host)
        return vol

    def compute(self, left, right, numDisparities, minDisparity: int = 0, host: bool = False):
        net = self.net
        D, m = net._check_planes(numDisparities), _offset(minDisparity)
        _check_offset_range(m, D)
        if _is_torch_cuda(left) != _is_torch_cuda(right):
            raise ValueError("both images must be numpy arrays or both torch CUDA tensors")
        if tuple(left.shape) != tuple(right.shape):
            raise ValueError("the two images must have the same shape")
        m_r = right_min_disparity(D, m)
        fl, fr = net.features(left, host=host), net.features(right, host=host)
        # the accurate net's scorer is not symmetric: its join is told the view's role
        role_l, role_r = ({"a_is_left": True}, {"a_is_left": False}) if isinstance(net, McCnnAccurate) else ({}, {})
        agg_l = self._aggregate(net.join(fl, fr, D, m, host=host, **role_l), left, right, m, host)
        agg_r = self._aggregate(net.join(fr, fl, D, m_r, host=host, **role_r), right, left, m_r, host)
        disp, maps = mc_disparity(agg_l, agg_r, left, m, self.params, host=host, stages=True)
        right_wta = maps["wta_right"]
        right_wta = right_wta.float() if _is_torch_cuda(right_wta) else right_wta.astype(np.float32)
        if getattr(left, "ndim", 3) == 2:
            disp, right_wta = disp[0], right_wta[0]
        return disp, right_wta

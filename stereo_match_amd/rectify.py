"""Rectification front end: the reference's ``rectify_opencv``
(``disparity_calculation.py:131-210``) and the gray conversion after it (``:286-287``).

* :func:`stereoRectify` — ``cv2.stereoRectify`` (Bouguet's procedure), on the host in
  numpy float64: a few hundred flops per rig, not a kernel.  ``alpha < 0`` only.
* :func:`initUndistortRectifyMap`, :func:`remap`, :func:`cvtColor` — on the GPU
  (``sm_rectify_map``, ``sm_remap_u8``, ``sm_bgr2gray_u8``).
* :func:`rectify_opencv` — the reference's function, same signature and results.
* :class:`StereoRectifier` — one rig's maps resident on the device; raw frames in,
  ``displ`` / ``filtered`` / rectified colour image / ``Q`` out, the gray images never
  leaving device memory between the remap and the matcher.

The arithmetic is a version-scoped restatement of OpenCV's; parity with OpenCV itself is
unpinned.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import SM_E_UNSUPPORTED, SmError

CALIB_ZERO_DISPARITY = 1024  # cv2.CALIB_ZERO_DISPARITY
CV_32FC1 = 5                 # cv2.CV_32FC1
INTER_LINEAR = 1             # cv2.INTER_LINEAR
COLOR_BGR2GRAY = 6           # cv2.COLOR_BGR2GRAY


def _is_torch_cuda(x) -> bool:
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


# ---- host geometry ---------------------------------------------------------------------

def _mat3(a, name):
    m = np.asarray(a, np.float64)
    if m.shape != (3, 3):
        raise ValueError(f"{name} must be a 3x3 matrix, not shape {m.shape}")
    return m


def _dist5(d, name):
    if d is None:
        return np.zeros(5, np.float64)
    v = np.asarray(d, np.float64).reshape(-1)
    if v.size == 4:
        v = np.concatenate([v, [0.0]])
    if v.size != 5:
        raise ValueError(f"{name} must hold (k1, k2, p1, p2[, k3]), not {v.size} values")
    return v


def _rodrigues_vec(om):
    """Rotation vector -> matrix."""
    om = np.asarray(om, np.float64).reshape(3)
    th = float(np.sqrt(om @ om))
    if th < 2.220446049250313e-16:
        return np.eye(3)
    k = om / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + (1.0 - np.cos(th)) * np.outer(k, k) + np.sin(th) * Kx


def _rodrigues_mat(R):
    """Rotation matrix -> vector."""
    r = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.sqrt(r @ r))
    c = min(1.0, max(-1.0, 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)))
    th = float(np.arctan2(s, c))
    if s < 1e-5:
        if c > 0:
            return r  # theta / sin(theta) -> 1
        # theta near pi: the axis from the symmetric part
        d = np.sqrt(np.maximum((np.diag(R) + 1.0) * 0.5, 0.0))
        if R[0, 1] < 0:
            d[1] = -d[1]
        if R[0, 2] < 0:
            d[2] = -d[2]
        if abs(d[0]) < abs(d[1]) and abs(d[0]) < abs(d[2]) and (R[1, 2] > 0) != (d[1] * d[2] > 0):
            d[2] = -d[2]
        return d * (th / max(float(np.sqrt(d @ d)), 1e-300))
    return r * (th / s)


def _undistort_normalized(px, py, K, d, iters=5):
    """cv2.undistortPoints without R / P: pixel -> normalised, ideal coordinates (the fixed-point
    iteration of the (k1, k2, p1, p2, k3) model, 5 rounds; exact for zero distortion)."""
    k1, k2, p1, p2, k3 = d
    x0 = (px - K[0, 2]) / K[0, 0]
    y0 = (py - K[1, 2]) / K[1, 1]
    x, y = x0, y0
    if not np.any(d):
        return x, y
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return x, y


def stereoRectify(cameraMatrix1, distCoeffs1, cameraMatrix2, distCoeffs2, imageSize, R, T,
                  flags=CALIB_ZERO_DISPARITY, alpha=-1):
    """``cv2.stereoRectify``: returns ``R1, R2, P1, P2, Q, roi1, roi2`` (float64).

    ``alpha < 0`` (what the reference passes) only: ``alpha`` in [0, 1] needs OpenCV's
    inner / outer rectangle search and raises ``SmError(SM_E_UNSUPPORTED)``.  The validity
    ROIs are returned as the full image ``(0, 0, W, H)``."""
    K1, K2 = _mat3(cameraMatrix1, "cameraMatrix1"), _mat3(cameraMatrix2, "cameraMatrix2")
    d1, d2 = _dist5(distCoeffs1, "distCoeffs1"), _dist5(distCoeffs2, "distCoeffs2")
    Rm = np.asarray(R, np.float64)
    if Rm.size == 3:
        Rm = _rodrigues_vec(Rm)
    Rm = _mat3(Rm, "R")
    Tv = np.asarray(T, np.float64)
    if Tv.size != 3:
        raise ValueError(f"T must hold 3 values, not shape {Tv.shape}")
    Tv = Tv.reshape(3)
    if len(imageSize) != 2 or int(imageSize[0]) <= 0 or int(imageSize[1]) <= 0:
        raise ValueError("imageSize must be (width, height) with positive entries")
    if alpha is not None and alpha >= 0:
        raise SmError(SM_E_UNSUPPORTED, f"stereoRectify: alpha={alpha} (the inner / outer rectangle search of "
                      "alpha in [0, 1]) is not implemented; pass alpha=-1 as disparity_calculation.py:184 does")
    nx, ny = float(int(imageSize[0])), float(int(imageSize[1]))

    om = _rodrigues_mat(Rm)
    r_r = _rodrigues_vec(-0.5 * om)  # each camera turns by half of R
    t = r_r @ Tv
    idx = 1 if abs(t[1]) > abs(t[0]) else 0
    c, nt = t[idx], float(np.sqrt(t @ t))
    if nt == 0.0:
        raise ValueError("T must not be zero")
    uu = np.zeros(3)
    uu[idx] = 1.0 if c > 0 else -1.0
    ww = np.cross(t, uu)  # the baseline onto the +-x (or +-y) axis
    nw = float(np.sqrt(ww @ ww))
    if nw > 0.0:
        ww = ww * (np.arccos(min(1.0, abs(c) / nt)) / nw)
    wR = _rodrigues_vec(ww)
    R1 = wR @ r_r.T
    R2 = wR @ r_r
    t = R2 @ Tv

    fc_new = np.inf
    for K, d in ((K1, d1), (K2, d2)):
        fc = K[idx ^ 1, idx ^ 1]
        if d[0] < 0:
            fc = fc * (1.0 + d[0] * (nx * nx + ny * ny) / (4.0 * fc * fc))
        fc_new = min(fc_new, fc)

    cx_ = np.array([0.0, nx - 1.0, 0.0, nx - 1.0])
    cy_ = np.array([0.0, 0.0, ny - 1.0, ny - 1.0])
    cc = np.zeros((2, 2))
    for k, (K, d, Rk) in enumerate(((K1, d1, R1), (K2, d2, R2))):
        xn, yn = _undistort_normalized(cx_, cy_, K, d)
        p = Rk @ np.stack([xn, yn, np.ones(4)])
        u = fc_new * p[0] / p[2]
        v = fc_new * p[1] / p[2]
        cc[k, 0] = (nx - 1.0) / 2.0 - u.sum() / 4.0
        cc[k, 1] = (ny - 1.0) / 2.0 - v.sum() / 4.0
    if int(flags) & CALIB_ZERO_DISPARITY:
        cc[0] = cc[1] = (cc[0] + cc[1]) * 0.5
    elif idx == 0:
        cc[0, 1] = cc[1, 1] = (cc[0, 1] + cc[1, 1]) * 0.5
    else:
        cc[0, 0] = cc[1, 0] = (cc[0, 0] + cc[1, 0]) * 0.5

    P1 = np.array([[fc_new, 0.0, cc[0, 0], 0.0], [0.0, fc_new, cc[0, 1], 0.0], [0.0, 0.0, 1.0, 0.0]])
    P2 = np.array([[fc_new, 0.0, cc[1, 0], 0.0], [0.0, fc_new, cc[1, 1], 0.0], [0.0, 0.0, 1.0, 0.0]])
    P2[idx, 3] = t[idx] * fc_new
    Q = np.array([[1.0, 0.0, 0.0, -cc[0, 0]],
                  [0.0, 1.0, 0.0, -cc[0, 1]],
                  [0.0, 0.0, 0.0, fc_new],
                  [0.0, 0.0, -1.0 / t[idx], (cc[0, idx] - cc[1, idx]) / t[idx]]])
    roi = (0, 0, int(nx), int(ny))
    return R1, R2, P1, P2, Q, roi, roi


def _rectify_cam(K, dist, R, P) -> "_lib.SmRectifyCam":
    K = _mat3(K, "cameraMatrix")
    d = _dist5(dist, "distCoeffs")
    Rm = np.eye(3) if R is None else _mat3(R, "R")
    Pm = K if P is None else np.asarray(P, np.float64)
    if Pm.shape not in ((3, 3), (3, 4)):
        raise ValueError(f"newCameraMatrix must be 3x3 or 3x4, not shape {Pm.shape}")
    iR = np.ascontiguousarray(np.linalg.inv(Pm[:3, :3] @ Rm))
    cam = _lib.SmRectifyCam()
    cam.K[:] = K.reshape(9).tolist()
    cam.dist[:] = d.tolist()
    cam.iR[:] = iR.reshape(9).tolist()
    return cam


def _size(size):
    if len(size) != 2:
        raise ValueError("size must be (width, height)")
    return int(size[0]), int(size[1])


def initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type=CV_32FC1, device=0):
    """``cv2.initUndistortRectifyMap``: float32 ``(mapx, mapy)``, each ``[H, W]`` for
    ``size = (W, H)``.  ``distCoeffs=None`` means zeros; only ``CV_32FC1`` maps are built."""
    if m1type != CV_32FC1:
        raise SmError(SM_E_UNSUPPORTED, "initUndistortRectifyMap: only m1type=CV_32FC1 is implemented")
    W, H = _size(size)
    return _lib.engine(device).rectify_map(_rectify_cam(cameraMatrix, distCoeffs, R, newCameraMatrix), H, W)


def _remap_torch(src, mapx, mapy, want_dst, want_gray):
    import torch

    if not (_is_torch_cuda(mapx) and _is_torch_cuda(mapy)):
        raise ValueError("remap: a CUDA source needs CUDA maps")
    if src.dtype != torch.uint8 or src.dim() not in (2, 3):
        raise ValueError("remap: src must be a uint8 [h, w] or [h, w, c] tensor")
    if mapx.dtype != torch.float32 or mapy.dtype != torch.float32 or mapx.dim() != 2 or mapx.shape != mapy.shape:
        raise ValueError("remap: mapx and mapy must be float32 [H, W] tensors of one shape")
    src, mapx, mapy = src.contiguous(), mapx.contiguous(), mapy.contiguous()
    cn = 1 if src.dim() == 2 else src.shape[2]
    h, w = src.shape[:2]
    H, W = mapx.shape
    dst = torch.empty((H, W) if src.dim() == 2 else (H, W, cn), dtype=torch.uint8, device=src.device) \
        if want_dst else None
    gray = torch.empty((H, W), dtype=torch.uint8, device=src.device) if want_gray else None
    eng = _lib.engine(src.device.index or 0)
    eng.set_stream(torch.cuda.current_stream(src.device).cuda_stream)
    eng.remap_batch_device(src.data_ptr(), 1, 0, h, w, w * cn, cn, mapx.data_ptr(), mapy.data_ptr(), H, W,
                           dst.data_ptr() if want_dst else None, gray.data_ptr() if want_gray else None)
    return dst, gray


def remap(src, map1, map2, interpolation=INTER_LINEAR, device=0):
    """``cv2.remap(src, map1, map2, INTER_LINEAR)`` on uint8 images of 1 or 3 channels,
    constant-0 border.  numpy in -> numpy out (synchronous); torch CUDA tensors in ->
    CUDA tensor on torch's current stream."""
    if interpolation != INTER_LINEAR:
        raise SmError(SM_E_UNSUPPORTED, "remap: only interpolation=INTER_LINEAR is implemented")
    if _is_torch_cuda(src):
        return _remap_torch(src, map1, map2, True, False)[0]
    return _lib.engine(device).remap(np.asarray(src), np.asarray(map1), np.asarray(map2), True, False)[0]


def cvtColor(src, code=COLOR_BGR2GRAY, device=0):
    """``cv2.cvtColor(src, COLOR_BGR2GRAY)`` on uint8 ``[H, W, 3]`` (numpy, or a torch CUDA
    tensor on torch's current stream)."""
    if code != COLOR_BGR2GRAY:
        raise SmError(SM_E_UNSUPPORTED, "cvtColor: only COLOR_BGR2GRAY is implemented")
    if _is_torch_cuda(src):
        import torch

        if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
            raise ValueError("cvtColor: src must be a uint8 [H, W, 3] tensor")
        src = src.contiguous()
        H, W = src.shape[:2]
        gray = torch.empty((H, W), dtype=torch.uint8, device=src.device)
        eng = _lib.engine(src.device.index or 0)
        eng.set_stream(torch.cuda.current_stream(src.device).cuda_stream)
        eng.bgr2gray_batch_device(src.data_ptr(), 1, 0, H, W, 3 * W, gray.data_ptr())
        return gray
    return _lib.engine(device).bgr2gray(np.asarray(src))


def relative_pose(camera_l_pose, camera_r_pose):
    """``rotation, translation`` of ``rectify_opencv`` (disparity_calculation.py:161-162): the
    blocks of ``inv(camera_r_pose) @ camera_l_pose`` for rigid 4x4 poses."""
    pl, pr = np.asarray(camera_l_pose, np.float64), np.asarray(camera_r_pose, np.float64)
    if pl.shape != (4, 4) or pr.shape != (4, 4):
        raise ValueError("camera poses must be 4x4 matrices")
    rotation = pr[:3, :3].transpose().dot(pl[:3, :3])
    translation = pr[:3, :3].transpose().dot(pl[:3, 3] - pr[:3, 3])
    return rotation, translation


def rectify_opencv(camera_l_pose, camera_r_pose, intrinsics_l, intrinsics_r, vis_l, vis_r, dist_coefficients_l=None,
                   dist_coefficients_r=None):
    """The reference's ``rectify_opencv`` (disparity_calculation.py:131-210): returns
    ``(img_rect1, img_rect2, Q)``."""
    if dist_coefficients_l is None:
        dist_coefficients_l = np.array([0.0, 0, 0, 0, 0])
    if dist_coefficients_r is None:
        dist_coefficients_r = np.array([0.0, 0, 0, 0, 0])
    rotation, translation = relative_pose(camera_l_pose, camera_r_pose)
    h, w = vis_l.shape[:2]
    size = (w, h)
    R1, R2, P1, P2, Q, roi1, roi2 = stereoRectify(intrinsics_l, dist_coefficients_l, intrinsics_r,
                                                  dist_coefficients_r, size, rotation, translation,
                                                  flags=CALIB_ZERO_DISPARITY, alpha=-1)
    mapx1, mapy1 = initUndistortRectifyMap(intrinsics_l, dist_coefficients_l, R1, P1, size, CV_32FC1)
    mapx2, mapy2 = initUndistortRectifyMap(intrinsics_r, dist_coefficients_r, R2, P2, size, CV_32FC1)
    img_rect1 = remap(vis_l, mapx1, mapy1, INTER_LINEAR)
    img_rect2 = remap(vis_r, mapx2, mapy2, INTER_LINEAR)
    return img_rect1, img_rect2, Q


class StereoRectifier:
    """One rig: ``R1 / R2 / P1 / P2 / Q`` computed once, both map pairs resident on the device.

    ``size = (W, H)`` is the frame size, also the rectified size (as the reference's
    ``new_size = size``).  Frames are uint8 ``[H, W, 3]`` BGR numpy arrays."""

    def __init__(self, K1, d1, K2, d2, size, R, T, device=0):
        import torch

        self.W, self.H = _size(size)
        self.device = int(device)
        self.R1, self.R2, self.P1, self.P2, self.Q, self.roi1, self.roi2 = stereoRectify(
            K1, d1, K2, d2, (self.W, self.H), R, T, flags=CALIB_ZERO_DISPARITY, alpha=-1)
        self._dev = torch.device("cuda", self.device)
        self._eng = _lib.engine(self.device)
        H, W = self.H, self.W
        self._maps = torch.empty((2, 2, H, W), dtype=torch.float32, device=self._dev)  # [camera][x / y]
        self._stream()
        for k, (K, d, Rk, Pk) in enumerate(((K1, d1, self.R1, self.P1), (K2, d2, self.R2, self.P2))):
            self._eng.rectify_map_device(_rectify_cam(K, d, Rk, Pk), H, W, self._maps[k, 0].data_ptr(),
                                         self._maps[k, 1].data_ptr())

    def _stream(self):
        import torch

        self._eng.set_stream(torch.cuda.current_stream(self._dev).cuda_stream)

    def maps(self):
        """((mapx1, mapy1), (mapx2, mapy2)) as float32 CUDA tensors."""
        return (self._maps[0, 0], self._maps[0, 1]), (self._maps[1, 0], self._maps[1, 1])

    def _upload(self, vis):
        import torch

        if _is_torch_cuda(vis):
            t = vis.contiguous()
        else:
            a = np.ascontiguousarray(vis)
            if a.dtype != np.uint8:
                raise ValueError("frames must be uint8")
            t = torch.from_numpy(a).to(self._dev, non_blocking=True)
        if t.dtype != torch.uint8 or tuple(t.shape) != (self.H, self.W, 3):
            raise ValueError(f"frames must be uint8 [{self.H}, {self.W}, 3] BGR images, not {tuple(t.shape)}")
        return t

    def rectify(self, vis_l, vis_r, want_bgr=(True, True)):
        """(img_rect1, img_rect2, gray_l, gray_r) as device-resident torch tensors (a BGR image
        not asked for in ``want_bgr`` is None); enqueued on torch's current stream."""
        import torch

        H, W = self.H, self.W
        gray = torch.empty((2, H, W), dtype=torch.uint8, device=self._dev)
        rect = [None, None]
        self._stream()
        for k, vis in enumerate((vis_l, vis_r)):
            src = self._upload(vis)
            if want_bgr[k]:
                rect[k] = torch.empty((H, W, 3), dtype=torch.uint8, device=self._dev)
            self._eng.remap_batch_device(src.data_ptr(), 1, 0, H, W, 3 * W, 3, self._maps[k, 0].data_ptr(),
                                         self._maps[k, 1].data_ptr(), H, W,
                                         rect[k].data_ptr() if want_bgr[k] else None, gray[k].data_ptr())
        self._gray = gray  # one allocation: pair stride H*W for the matcher
        return rect[0], rect[1], gray[0], gray[1]

    def compute_disparity(self, vis_l, vis_r, disparity_settings):
        """Raw frames -> ``(displ, filtered, img_rect1, Q)``: upload, remap with the fused gray
        output, ``compute_disparity`` (both matchers + WLS, stereo_vision.py:132-184) on the gray
        device buffers, download of the three results (numpy)."""
        import torch

        from . import wls
        from .stereo_vision import matcher_from_settings

        H, W = self.H, self.W
        left_matcher = matcher_from_settings(disparity_settings, "SGBM", self.device)
        prm = left_matcher.params()  # before createDisparityWLSFilter's mutation, as compute_disparity
        wf = wls.createDisparityWLSFilter(left_matcher)
        wf.setLambda(disparity_settings['lmbda'])
        wf.setSigmaColor(disparity_settings['sigma'])
        wp = wf.params(H, W)
        rect1, _, gray_l, gray_r = self.rectify(vis_l, vis_r, want_bgr=(True, False))
        maps = torch.empty((3, H, W), dtype=torch.int16, device=self._dev)  # displ, dispr, filtered
        self._eng.compute_disparity_batch_device(gray_l.data_ptr(), gray_r.data_ptr(), 1, H * W, H, W, W, prm, wp,
                                                 maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr())
        displ = maps[0].cpu().numpy()
        filtered = maps[2].cpu().numpy()
        return displ, filtered, rect1.cpu().numpy(), self.Q

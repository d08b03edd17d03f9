"""Helpers of test_gpu_strides.py and test_gpu_ctx_reuse.py: image batches embedded in poisoned
device buffers, guarded outputs, and the pairs / oracle results the two files share."""
import functools

import numpy as np

from oracle import bm_np, ref_c, sgm_np, wls_np
from stereo_match_amd import _lib, synthetic

SENTINEL = 12345  # as the existing batch tests fill their outputs
FILLS = (0x00, 0xFF)


def embed(images, stride, pair_stride, base_offset, fill):
    """(buf, ptr): a torch uint8 device buffer holding image i (uint8 [H, W] or [H, W, cn]) at
    lead + base_offset + i * pair_stride with rows `stride` bytes apart, and the device pointer of
    image 0.  Every byte that is no image byte is `fill`: the lead-in (one row at least, a
    multiple of 256 bytes, so that base_offset alone sets the alignment), the row padding, the
    gaps between the pairs and a tail of one row at least."""
    import torch

    H = images[0].shape[0]
    row = int(np.prod(images[0].shape[1:]))
    assert stride >= row and (len(images) == 1 or pair_stride >= (H - 1) * stride + row)
    lead = -(-max(stride, 1) // 256) * 256
    host = np.full(lead + base_offset + len(images) * pair_stride + H * stride + stride, fill, np.uint8)
    for i, img in enumerate(images):
        assert img.dtype == np.uint8 and img.shape == images[0].shape
        at = lead + base_offset + i * pair_stride
        rows = np.lib.stride_tricks.as_strided(host[at:], (H, row), (stride, 1))
        rows[...] = img.reshape(H, row)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0
    buf._host = host  # what the buffer must still hold after the call
    return buf, buf.data_ptr() + lead + base_offset


def unchanged(buf) -> bool:
    return np.array_equal(buf.cpu().numpy(), buf._host)


def guarded(n, H, W):
    """(buf, ptr, G): an int16 device buffer of SENTINEL with G >= W guard elements on either side
    of [n][H][W], and the pointer of the maps (16-byte aligned, as a tensor of its own is)."""
    import torch

    G = -(-max(W, 1) // 64) * 64
    buf = torch.full((2 * G + n * H * W,), SENTINEL, dtype=torch.int16, device="cuda")
    return buf, buf.data_ptr() + 2 * G, G


def maps_of(out, n, H, W):
    """The [n, H, W] maps of a guarded() buffer; asserts both guards still hold SENTINEL."""
    buf, _, G = out
    a = buf.cpu().numpy()
    assert (a[:G] == SENTINEL).all(), "the guard in front of the output was written"
    assert (a[G + n * H * W:] == SENTINEL).all(), "the guard behind the output was written"
    return a[G:G + n * H * W].reshape(n, H, W)


def key(p: dict):
    return tuple(sorted(p.items()))


def sgbm_params(cost, D, mode, **kw):
    """census (headline_params) or the SGBM cost (parity_params) at 5 or 8 paths."""
    return dict(synthetic.headline_params(D) if cost else synthetic.parity_params(D), mode=mode, **kw)


@functools.lru_cache(maxsize=None)
def pairs(H, W, D, n, seed=0):
    out = []
    for i in range(n):
        a, b, _ = synthetic.random_dot_pair(H, W, D, seed=9000 + 31 * seed + i)
        a.setflags(write=False)
        b.setflags(write=False)
        out.append((a, b))
    return tuple(out)


def bgr(gray, seed):
    """A BGR image built from a gray one: the channels differ (as tests/test_gpu_wide.py's)."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 20, gray.shape, dtype=np.uint8)
    return np.ascontiguousarray(np.stack([gray, np.roll(gray, 1, 0) // 2 + noise, 255 - gray], -1))


@functools.lru_cache(maxsize=None)
def bgr_pairs(H, W, D, n, seed=0):
    return tuple((bgr(a, 3 * i + seed), bgr(b, 3 * i + seed)) for i, (a, b) in enumerate(pairs(H, W, D, n, seed)))


@functools.lru_cache(maxsize=None)
def expected(H, W, D, n, pkey, seed=0, channels=1):
    """ref_c.compute of every pair of pairs() / bgr_pairs(), computed once and left unchanged."""
    src = pairs(H, W, D, n, seed) if channels == 1 else bgr_pairs(H, W, D, n, seed)
    out = ref_c.compute_many(list(src), dict(pkey))
    for o in out:
        o.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected_wta(H, W, D, n, pkey, seed=0):
    out = tuple(ref_c.compute_wta(a, b, dict(pkey)) for a, b in pairs(H, W, D, n, seed))
    for d, w in out:
        d.setflags(write=False)
        w.setflags(write=False)
    return out


def bm_params(p: dict) -> _lib.SmBmParams:
    q = bm_np.normalize_bm(p)
    return _lib.SmBmParams(q["minDisparity"], q["numDisparities"], q["blockSize"], q["preFilterType"],
                           q["preFilterSize"], q["preFilterCap"], q["textureThreshold"], q["uniquenessRatio"],
                           q["speckleWindowSize"], q["speckleRange"], q["disp12MaxDiff"])


@functools.lru_cache(maxsize=None)
def expected_bm(H, W, D, n, pkey, seed=0):
    out = tuple(bm_np.stereo_bm(a, b, dict(pkey)) for a, b in pairs(H, W, D, n, seed))
    for o in out:
        o.setflags(write=False)
    return out


def wls_params(p: dict, H, W) -> _lib.SmWlsParams:
    q = wls_np.normalize_wls(p, H, W)
    return _lib.SmWlsParams(q["lmbda"], q["sigma"], q["lrc_thresh"], q["radius"], int(q["use_confidence"]),
                            q["min_disp"], q["left_offset"], q["right_offset"], q["top_offset"],
                            q["bottom_offset"], q["num_iter"], q["attenuation"], q["roll_off"])


@functools.lru_cache(maxsize=None)
def lr_maps(H, W, D, n, pkey, seed=0):
    """(displ, dispr) of every pair as compute_disparity makes them: the left matcher with the WLS
    factory's mutation, the right matcher of the unmutated settings on the swapped pair."""
    s = dict(pkey)
    lp = dict(s, uniquenessRatio=0, disp12MaxDiff=1000000, speckleWindowSize=0)
    rp = sgm_np.right_matcher_params(s)
    src = list(pairs(H, W, D, n, seed))
    dl = ref_c.compute_many(src, lp)
    dr = ref_c.compute_many([(b, a) for a, b in src], rp)
    for o in dl + dr:
        o.setflags(write=False)
    return tuple(dl), tuple(dr)


@functools.lru_cache(maxsize=None)
def expected_wls(H, W, D, n, pkey, wkey, seed=0, conf=True):
    """wls_np.wls_filter of lr_maps() guided by the left images."""
    dl, dr = lr_maps(H, W, D, n, pkey, seed)
    out = tuple(wls_np.wls_filter(dl[i], a, dr[i] if conf else None, dict(wkey))
                for i, (a, _) in enumerate(pairs(H, W, D, n, seed)))
    for o in out:
        o.setflags(write=False)
    return out


def default_wls(settings: dict, lmbda=8000.0, sigma=1.5):
    """(SmWlsParams, oracle dict) of createDisparityWLSFilter(StereoSGBM(settings))."""
    sp = synthetic.to_sm_params(settings)
    wp = _lib.wls_default_params(sp)
    wp.lambda_, wp.sigma_color = lmbda, sigma
    minD, D = settings["minDisparity"], settings["numDisparities"]
    wd = dict(lmbda=lmbda, sigma=sigma, radius=(settings["blockSize"] + 1) // 2, min_disp=minD,
              left_offset=max(0, minD + D), right_offset=max(0, -minD))
    return wp, wd

"""Shared inputs of the tests of MC-CNN's stereo method: seeded scenes and the CPU twin's results, each
computed once per process and never modified."""
import functools

import numpy as np

import stereo_match_amd as sm

# (H, W, D, m): one pixel, one row, one column, more planes than columns, the widths around the
# vertical strip (32) and the horizontal tile (16), 64 / 65 / 256 planes (one, two and four planes
# per lane), negative and positive offsets, the reference's plane count
SHAPES = [(1, 1, 1, 0), (1, 70, 5, 0), (37, 1, 4, 0), (5, 3, 20, 0), (33, 64, 64, 0), (33, 65, 65, 3),
          (40, 131, 37, -4), (9, 130, 256, -100), (20, 200, 228, 0)]
SCENE = (40, 131, 37, -4)  # the shape whose scene meets every condition of test_mcsgm_host.py
SMALL_BLUR = sm.McCnnStereoParams(blur_sigma=1.3, blur_t=0.6)  # a 9 x 9 window, a threshold that rejects taps
DEFAULT = sm.McCnnStereoParams()


def same_bits(a, b):
    """Equal shapes and types, equal NaN masks and the same bits in every other cell (the payload of a
    NaN is all that may differ: no caller can observe it); integer and boolean maps element for
    element."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def right_m(D, m):
    return -(m + D) + 1


def volume(a, b, D, m, rng, noise=1.0):
    """V[d] = |a(x) - b(x - (m + d))| on gray / 4 plus noise, NaN outside the image: costs up to 64, so
    that the default penalties (4 and 55.72) smooth the surfaces without flattening them."""
    H, W = a.shape
    fa, fb = a.astype(np.float32) / np.float32(4), b.astype(np.float32) / np.float32(4)
    V = np.full((D, H, W), np.nan, np.float32)
    xs = np.arange(W)
    for d in range(D):
        c = xs - (m + d)
        ok = (c >= 0) & (c < W)
        V[d][:, ok] = np.abs(fa[:, ok] - fb[:, c[ok]])
    V += (rng.random(V.shape) * noise).astype(np.float32)
    return V


@functools.lru_cache(maxsize=None)
def scene(H, W, D, m, seed=7):
    """(left, right, V_left, V_right): a blocky texture (steps of 0 inside a block, large ones between
    blocks, so all penalty classes occur), a background at disparity m + 2, a foreground band at
    m + D - 1 and a top band at m (the sub-pixel guards at both ends), a right image warped from the
    left one with noise in the holes, 3 % of the pixels with random costs (mismatches)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    base = rng.integers(0, 256, (H // 2 + 1, W // 3 + 1))
    left = np.kron(base, np.ones((2, 3), np.int64))[:H, :W]
    left = np.clip(left + rng.integers(-1, 2, (H, W)), 0, 255).astype(np.uint8)
    truth = np.full((H, W), m + min(2, D - 1))
    truth[H // 4:3 * H // 4, W // 3:2 * W // 3] = m + D - 1
    truth[:max(H // 8, 1)] = m
    right = rng.integers(0, 256, (H, W)).astype(np.uint8)
    for level in sorted(set(truth.ravel().tolist())):  # nearer surfaces overwrite farther ones
        ys, xs = np.nonzero(truth == level)
        ok = (xs - level >= 0) & (xs - level < W)
        right[ys[ok], xs[ok] - level] = left[ys[ok], xs[ok]]
    vl = volume(left, right, D, m, rng)
    vr = volume(right, left, D, right_m(D, m), rng)
    bad = rng.random((H, W)) < 0.03
    vl[:, bad] = np.where(np.isnan(vl[:, bad]), np.nan, (rng.random((D, int(bad.sum()))) * 64).astype(np.float32))
    for arr in (left, right, vl, vr):
        arr.setflags(write=False)
    return left, right, vl, vr


@functools.lru_cache(maxsize=None)
def twin_aggregates(H, W, D, m, params=DEFAULT):
    """(A_left, A_right) of the scene by the CPU twin."""
    left, right, vl, vr = scene(H, W, D, m)
    al = sm.mc_aggregate(vl, left, right, m, params, host=True)
    ar = sm.mc_aggregate(vr, right, left, right_m(D, m), params, host=True)
    for arr in (al, ar):
        arr.setflags(write=False)
    return al, ar


@functools.lru_cache(maxsize=None)
def stage_inputs(H, W, D, m):
    """The aggregated volumes the disparity tests start from: twin_aggregates; in the SCENE shape a few
    pixels' costs are flattened so that the sub-pixel step meets a zero denominator, and some cells
    are removed so that the interpolation meets rows and pixels without support."""
    al, ar = twin_aggregates(H, W, D, m)
    if (H, W, D, m) == SCENE:
        al, ar = al.copy(), ar.copy()
        x0 = 2 * W // 3 + 1  # just right of the foreground band: occluded in the right view
        blk = al[:, H // 2 - 2:H // 2 + 2, x0:x0 + 6]
        blk[...] = np.where(np.isnan(blk), np.nan, np.float32(1.5))
        ar[:, H - 2] = np.nan      # a row without any correct pixel: its pixels keep their values,
        al[:, H - 2, 7] = np.nan   # and this one stays invalid
        ar[:, H - 4, :20] = np.nan  # occluded pixels with correct ones only to their right
        al[:, H - 6, 5] = np.nan   # no plane at all, filled from the left
        for arr in (al, ar):
            arr.setflags(write=False)
    return al, ar


@functools.lru_cache(maxsize=None)
def twin_disparity(H, W, D, m, params=SMALL_BLUR):
    al, ar = stage_inputs(H, W, D, m)
    disp, maps = sm.mc_disparity(al, ar, scene(H, W, D, m)[0], m, params, host=True, stages=True)
    for arr in [disp] + list(maps.values()):
        arr.setflags(write=False)
    return disp, maps

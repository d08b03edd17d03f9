"""Shared inputs of the tests of the cross-based cost aggregation: seeded scenes and
the CPU twin's results, each computed once per process and never modified."""
import functools

import numpy as np

import mcsgm_cases as S
import stereo_match_amd as sm

TILE_W, TILE_H = 64, 32  # k_mcb_agg's tile (32 rows while L1 <= 26)
HALO = 4                 # L1 - 1 of the l1 = 5 every shape runs with: the tile with its halo is 72 x 40
# (H, W, D, m): the shapes of the semi-global matching's tests; widths and heights one below, at and
# one above the tile; one below, at and one above the tile with its halo
SHAPES = list(S.SHAPES) + [(TILE_H - 1, TILE_W - 1, 5, 0), (TILE_H, TILE_W, 5, 1), (TILE_H + 1, TILE_W + 1, 5, -2),
                           (TILE_H + 2 * HALO - 1, TILE_W + 2 * HALO - 1, 4, 0), (TILE_H + 2 * HALO, TILE_W + 2 * HALO, 4, 2),
                           (TILE_H + 2 * HALO + 1, TILE_W + 2 * HALO + 1, 4, -1)]
SCENE = (40, 131, 37, -4)
L1S = (1, 2, 5, 14, 32)  # 32: the 16-row tile
TAU1 = 0.05
same_bits, right_m = S.same_bits, S.right_m


def params(l1=5, tau1=TAU1, **kw):
    return sm.McCnnCrossParams(l1=l1, tau1=tau1, **kw)


@functools.lru_cache(maxsize=None)
def scene(H, W, D, m, seed=7):
    """(left, right, V_left, V_right): a blocky left image (blocks of 9 x 12 with noise of +-2 grey
    levels, so that arms end at the cap, at a border and at tau1), the right image and both volumes
    made from it by the warp and the volume() of mcsgm_cases."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    base = rng.integers(0, 256, (H // 9 + 1, W // 12 + 1))
    left = np.kron(base, np.ones((9, 12), np.int64))[:H, :W] + rng.integers(-2, 3, (H, W))
    left = np.clip(left, 0, 255).astype(np.uint8)
    truth = np.full((H, W), m + min(2, D - 1))
    truth[H // 4:3 * H // 4, W // 3:2 * W // 3] = m + D - 1
    truth[:max(H // 8, 1)] = m
    right = rng.integers(0, 256, (H, W)).astype(np.uint8)
    for level in sorted(set(truth.ravel().tolist())):  # nearer surfaces overwrite farther ones
        ys, xs = np.nonzero(truth == level)
        ok = (xs - level >= 0) & (xs - level < W)
        right[ys[ok], xs[ok] - level] = left[ys[ok], xs[ok]]
    vl = S.volume(left, right, D, m, rng)
    vr = S.volume(right, left, D, right_m(D, m), rng)
    for arr in (left, right, vl, vr):
        arr.setflags(write=False)
    return left, right, vl, vr


@functools.lru_cache(maxsize=None)
def twin_arms(shape, l1=5, tau1=TAU1):
    """uint8 [4, H, W] of the scene's left image by the CPU twin."""
    out = sm.mc_cross_arms(scene(*shape)[0], params(l1, tau1), host=True)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin_cross(shape, l1=5, tau1=TAU1, iterations=1, view=0):
    """The scene's left (view 0) or right volume after `iterations` steps, by the CPU twin."""
    H, W, D, m = shape
    left, right, vl, vr = scene(*shape)
    if view == 0:
        out = sm.mc_cross_aggregate(vl, left, right, m, params(l1, tau1), iterations, host=True)
    else:
        out = sm.mc_cross_aggregate(vr, right, left, right_m(D, m), params(l1, tau1), iterations, host=True)
    out.setflags(write=False)
    return out

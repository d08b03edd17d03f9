"""Inputs the WLS filter's tests share (oracle liveness on the CPU, device parity on the GPU): maps
whose confidence is alive, the case lists of tests/test_gpu_wls.py, and the oracle chain of
compute_disparity for settings away from settings.ini.  Everything is made from seeds.

Why not noise alone: independent uniform noise for displ / dispr has a windowed variance far above
1/roll_off and fails the LR check almost everywhere, so conf = 0, num = den = 0 and the filter's
output is 0 at every ROI pixel whatever the smoother does (tests/test_wls_oracle.py pins this)."""
import functools

import numpy as np

from oracle import wls_np

CONF_LDS_MAX = 65536  # csrc/sm_api.hip run_wls: ca.separable = wls_conf_lds(w, r) <= 65536


def wls_conf_lds(w, r):
    """csrc/sm_wls.hpp wls_conf_lds restated: dynamic LDS bytes of k_wls_conf's separable path
    (tab[256] + confr[w] + confl[w] floats rounded up to 8, then w + 2r column sums of 4 + 8 bytes)."""
    return ((256 + 2 * w) * 4 + 7) // 8 * 8 + (w + 2 * r) * 12 + 16


def separable_limit(r):
    """the widest ROI whose confidence rows still take the separable (LDS column sums) path"""
    w = 1
    while wls_conf_lds(w + 1, r) <= CONF_LDS_MAX:
        w += 1
    return w


def noise_maps(H, W, seed):
    """the independent-noise construction test_gpu_wls.py has always used (dead confidence)"""
    rng = np.random.default_rng(seed)
    displ = rng.integers(-16, 40 * 16, (H, W)).astype(np.int16)
    dispr = (-rng.integers(0, 40 * 16, (H, W))).astype(np.int16)
    guide = rng.integers(0, 256, (H, W)).astype(np.uint8)
    return displ, dispr, guide


@functools.lru_cache(None)
def consistent_maps(H, W, seed, dmax=20):
    """(displ, dispr, guide) that agree with each other the way matcher outputs do.

    displ (x16): a plane rising a quarter unit per column and half a unit per row (windowed variance
    of a few units, so conf = 1 - roll_off * var is fractional at roll_off 0.001), wrapped below
    dmax pixels; fronto-parallel bands three pixels nearer; +-6 units of noise; 2 % outliers anywhere
    in [0, dmax) pixels.  dispr: displ warped forward, dispr[y, x - (displ >> 4)] = -displ[y, x] +- 8
    (collisions and outliers fail the LR check, the rest pass it); columns nothing maps to keep -48.
    guide: noise averaged with its left and upper neighbour over 17 x 11 blocks of three levels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    plane = (xx + 2 * yy) // 4
    d = 48 + plane % (16 * max(dmax - 4, 1))
    band = (xx % 97 > 60) & (yy >= H // 4)
    d[band] += 48
    d += rng.integers(-6, 7, (H, W))
    wild = rng.random((H, W)) < 0.02
    d[wild] = rng.integers(0, 16 * dmax, int(wild.sum()))
    dr = np.full((H, W), -48, np.int64)
    xr = xx - (d >> 4)
    hit = (xr >= 0) & (xr < W)
    dr[yy[hit], xr[hit]] = -d[hit] + rng.integers(-8, 9, int(hit.sum()))
    g = rng.integers(0, 256, (H, W)).astype(np.float64)
    g = (g + np.roll(g, 1, axis=1) + np.roll(g, 1, axis=0) + 40 * ((xx // 17 + yy // 11) % 3)) / 3
    out = d.astype(np.int16), dr.astype(np.int16), np.clip(g, 0, 255).astype(np.uint8)
    for a in out:
        a.setflags(write=False)
    return out


def liveness(displ, dispr, guide, params):
    """What a parity test over these inputs can see, from the oracle alone, over the ROI: the share
    of pixels with 0 < conf < 255, with output != 0, with output != displ, the number of distinct
    output values, and whether the smoothed num / den hold non-finite values."""
    H, W = displ.shape
    p = wls_np.normalize_wls(params, H, W)
    with np.errstate(all="ignore"):
        out, st = wls_np.wls_filter(displ, guide, dispr if p["use_confidence"] else None, params, return_stages=True)
    x0, y0, w, h = p["roi"]
    roi = out[y0:y0 + h, x0:x0 + w]
    res = dict(pixels=int(roi.size), frac_conf=None, nonfinite=False, out=out)
    if roi.size == 0:
        return dict(res, nonzero=0.0, changed=0.0, distinct=0)
    if "conf" in st:
        c = st["conf"][y0:y0 + h, x0:x0 + w]
        res["frac_conf"] = float(((c > 0) & (c < 255)).mean())
        res["live_conf"] = float((c > 0).mean())
        res["nonfinite"] = not (np.isfinite(st["num"]).all() and np.isfinite(st["den"]).all())
    res["nonzero"] = float((roi != 0).mean())
    res["changed"] = float((roi != displ[y0:y0 + h, x0:x0 + w]).mean())
    res["distinct"] = int(len(np.unique(roi)))
    return res


# ---- case lists ------------------------------------------------------------------------------------
def case(name, H, W, nonfinite=False, dead=False, empty=False, **p):
    """one filter call over consistent_maps(H, W): p are wls_np params; nonfinite / dead / empty
    declare what the oracle shows for the case (checked in tests/test_wls_oracle.py)"""
    q = dict(dict(sigma=1.2, lrc_thresh=24, use_confidence=True), **p)
    return dict(id=name, H=H, W=W, p=q, nonfinite=nonfinite, dead=dead, empty=empty)


def case_inputs(c):
    return consistent_maps(c["H"], c["W"], c["H"] * 1000 + c["W"], dmax=min(20, max(2, c["W"] // 4)))


_expected = {}


def case_expected(c):
    """the oracle's map for a case, computed once per process"""
    if c["id"] not in _expected:
        displ, dispr, guide = case_inputs(c)
        with np.errstate(all="ignore"):  # declared non-finite stages (lambda 3e8)
            out = wls_np.wls_filter(displ, guide, dispr if c["p"]["use_confidence"] else None, c["p"])
        out.setflags(write=False)
        _expected[c["id"]] = out
    return _expected[c["id"]]


PIVOT_LAMBDAS = (0.0, 80000.0, 2.0e6, 1.0e7, 3.0e8)
_PIV = dict(radius=3, left_offset=20, num_iter=3)
# 1 + 2 lambda < 2^24 (lambda < 8388607.5) takes rcp + one FMA step, above it IEEE division
PIVOT_CASES = [case(f"lam{lam:g}", 30, 160, nonfinite=lam == 3.0e8, lmbda=lam, **_PIV) for lam in PIVOT_LAMBDAS] + [
    # attenuation: lambda * att^it crosses 2^24 part-way, so wls_fast() must say IEEE for all passes
    case("lam3e6_att2", 30, 160, lmbda=3.0e6, attenuation=2.0, **_PIV),          # 3e6, 6e6, 1.2e7
    case("lam6e6_att2_it2", 30, 160, lmbda=6.0e6, attenuation=2.0, radius=3, left_offset=20, num_iter=2),
    case("lam1e7_att0", 30, 160, lmbda=1.0e7, attenuation=0.0, **_PIV),          # IEEE first, then lambda 0
    case("lam3e6_att1", 30, 160, lmbda=3.0e6, attenuation=1.0, **_PIV),          # fast, never attenuated
    case("lam8e4_att0", 30, 160, lmbda=80000.0, attenuation=0.0, **_PIV),
    case("lam8e4_att1_it8", 30, 160, lmbda=80000.0, attenuation=1.0, radius=3, left_offset=20, num_iter=8),
]

RADIUS_SHAPES = ((2, 20, 6), (3, 24, 64), (1, 40, 5), (5, 2, 9))
RADIUS_CASES = [case(f"{H}x{W}r{r}", H, W, lmbda=8000.0, sigma=1.5, radius=r, num_iter=2) for H, W, r in RADIUS_SHAPES]

# The same shapes with roll_off near 1 / (windowed variance of that map, from the oracle: 11 to 33 units),
# where 1 - roll_off * var crosses 0: a window sum that is off by a few percent flips pixels between
# clipped and live, so the final map depends on which samples the window reflects to.  At roll_off
# 0.001 the confidence of these small maps is about 0.99 everywhere and the 5 x 2 map's output does
# not change with the reflection rule (test_radius_clip_cases_see_the_reflection_rule).
RADIUS_CLIP_ROLL_OFF = {(2, 20, 6): 0.05, (3, 24, 64): 0.03, (1, 40, 5): 0.03, (5, 2, 9): 0.09}
RADIUS_CLIP_CASES = [case(f"{H}x{W}r{r}_rolloff{ro:g}", H, W, lmbda=8000.0, sigma=1.5, radius=r, num_iter=2, roll_off=ro)
                     for (H, W, r), ro in RADIUS_CLIP_ROLL_OFF.items()]

ROLL_OFFS = (0.0, 0.001, 0.02, 10.0)
ROLL_OFF_CASES = [case(f"rolloff{ro:g}", 30, 160, dead=ro == 10.0, lmbda=8000.0, radius=3, left_offset=20, roll_off=ro)
                  for ro in ROLL_OFFS]

# num_iter > 8 (sm_api.hip kWlsMaxPivotIters) leaves the pivot buffers for k_fgs; 8 is the last
# pivot-path count.  70 x 150 with left_offset 20: an ROI of 70 x 130, no multiple of 64 and more
# than one 64-chunk both ways.
_K = dict(radius=2, left_offset=20)
KFGS_CASES = [
    case("it8_conf_fast", 70, 150, lmbda=8000.0, num_iter=8, **_K),
    case("it8_noconf_ieee", 70, 150, lmbda=1.0e7, num_iter=8, use_confidence=False, **_K),
    case("it9_conf_fast", 70, 150, lmbda=8000.0, num_iter=9, **_K),
    case("it9_noconf_fast", 70, 150, lmbda=8000.0, num_iter=9, use_confidence=False, **_K),
    case("it9_conf_ieee", 70, 150, lmbda=1.0e7, num_iter=9, **_K),
    case("it9_noconf_ieee", 70, 150, lmbda=1.0e7, num_iter=9, use_confidence=False, **_K),
    case("it9_conf_att2_ieee_later", 70, 150, lmbda=4.0e4, attenuation=2.0, num_iter=9, **_K),  # 1.024e7 at the end
    case("it12_conf_att1", 70, 150, lmbda=500.0, attenuation=1.0, num_iter=12, **_K),
    case("it12_noconf_att1", 70, 150, lmbda=500.0, attenuation=1.0, num_iter=12, use_confidence=False, **_K),
    case("it12_40x200", 40, 200, lmbda=8000.0, num_iter=12, **_K),
]


def _wide(H, w, r):
    return case(f"{H}x{w}r{r}", H, w + 20, lmbda=8000.0, radius=r, left_offset=20, num_iter=2)


# ROI widths on both sides of the separable limit of their radius (3224 for r = 0, 3221 for r = 3)
WIDE_CASES = [_wide(3, separable_limit(0), 0), _wide(3, separable_limit(0) + 1, 0), _wide(5, separable_limit(3), 3),
              _wide(5, separable_limit(3) + 1, 3), _wide(3, 3300, 3)]


def wide_separable(c):
    p = c["p"]
    return wls_conf_lds(c["W"] - p["left_offset"], p["radius"]) <= CONF_LDS_MAX


_D = dict(lmbda=8000.0, radius=2)
DEGENERATE_CASES = [case(f"empty_w0_min{m}", 10, 40, empty=True, left_offset=30, right_offset=10, min_disp=m, **_D)
                    for m in (-3, 0, 5)] + [
    case(f"empty_wneg3_min{m}", 10, 40, empty=True, left_offset=33, right_offset=10, min_disp=m, **_D) for m in (-3, 0, 5)] + [
    case(f"empty_h0_min{m}", 10, 40, empty=True, top_offset=4, bottom_offset=6, min_disp=m, **_D) for m in (-3, 0, 5)] + [
    case("one_column", 10, 40, left_offset=30, right_offset=9, min_disp=-3, **_D),
    case("one_row", 10, 40, top_offset=4, bottom_offset=5, min_disp=5, **_D),
    case("one_pixel", 10, 40, left_offset=12, right_offset=27, top_offset=4, bottom_offset=5, **_D),
    case("map_h1", 1, 40, **_D),
    case("map_w1", 12, 1, **_D),
    case("map_h1_noconf", 1, 40, use_confidence=False, **_D),
]

CASE_LISTS = dict(pivot=PIVOT_CASES, radius=RADIUS_CASES, radius_clip=RADIUS_CLIP_CASES, roll_off=ROLL_OFF_CASES, kfgs=KFGS_CASES, wide=WIDE_CASES,
                  degenerate=DEGENERATE_CASES)


def hypothesis_maps(kind, H, W, seed):
    return noise_maps(H, W, seed) if kind == "noise" else consistent_maps(H, W, seed, dmax=min(20, max(2, W // 4)))


# ---- compute_disparity away from settings.ini -------------------------------------------------------
CD_H, CD_W, CD_D = 60, 220, 32
# each entry changes one key of dict(DEFAULT_SETTINGS, window_size=5, num_disparities=32); refused: the
# library's message for a setting it does not build (asserted, not skipped)
CD_SETTINGS = [
    dict(id="ws3", change=dict(window_size=3)),
    dict(id="minD-8", change=dict(min_disparity=-8)),
    dict(id="minD+8", change=dict(min_disparity=8)),
    dict(id="bs3", change=dict(block_size=3)),
    dict(id="bs9", change=dict(block_size=9)),
    dict(id="speckle50", change=dict(speckle_window_size=50, speckle_range=2)),
    dict(id="uniq0", change=dict(uniqueness_ratio=0)),
    dict(id="paths8", change=dict(paths=8)),
    dict(id="census8", change=dict(cost="census", paths=8), refused="census mode needs P2 <= 193"),
    # the same mode with penalties the census path takes (window_size 1: P1 24, P2 96), so that it runs too
    dict(id="census8_ws1", change=dict(cost="census", paths=8, window_size=1)),
]
CD_BM = dict(id="bm_bs9_D48", change=dict(block_size=9, num_disparities=48))


def cd_settings(entry):
    from stereo_match_amd import settings

    return dict(dict(settings.DEFAULT_SETTINGS, window_size=5, num_disparities=CD_D), **entry["change"])


@functools.lru_cache(None)
def cd_pair(i=0):
    from stereo_match_amd import synthetic

    left, right, _ = synthetic.random_dot_pair(CD_H, CD_W, CD_D, seed=90 + i)
    return left, right


@functools.lru_cache(None)
def cd_chain(entry_id, i=0):
    """(displ, dispr, filtered, wls params) of the oracle chain, in the reference's order: left matcher
    with createDisparityWLSFilter's mutation (uniqueness 0, disp12MaxDiff 1e6, speckle window 0), right
    matcher from the unmutated settings, WLS with offsets and radius derived here from the settings."""
    from oracle import bm_np, ref_c, sgm_np

    entry = CD_BM if entry_id == CD_BM["id"] else next(e for e in CD_SETTINGS if e["id"] == entry_id)
    s = cd_settings(entry)
    left, right = cd_pair(i)
    minD, D, bs = s["min_disparity"], s["num_disparities"], s["block_size"]
    if entry is CD_BM:
        exp_l = bm_np.stereo_bm(left, right, dict(numDisparities=D, blockSize=bs, textureThreshold=0, uniquenessRatio=0,
                                                  disp12MaxDiff=1000000))
        exp_r = bm_np.stereo_bm(right, left, bm_np.right_matcher_params(dict(numDisparities=D, blockSize=bs)))
        wp = dict(lmbda=float(s["lmbda"]), sigma=s["sigma"], radius=int(np.ceil(0.33 * bs)), min_disp=0,
                  left_offset=D + bs // 2, right_offset=bs // 2, top_offset=bs // 2, bottom_offset=bs // 2)
    else:
        ws = s["window_size"]
        full = dict(minDisparity=minD, numDisparities=D, blockSize=bs, P1=8 * 3 * ws ** 2, P2=32 * 3 * ws ** 2,
                    disp12MaxDiff=s["disp12_max_diff"], uniquenessRatio=s["uniqueness_ratio"],
                    preFilterCap=s["pre_filter_cap"], speckleWindowSize=s["speckle_window_size"],
                    speckleRange=s["speckle_range"], mode=int(s.get("paths", 5)),
                    cost=1 if s.get("cost", "sgbm") == "census" else 0)
        exp_l = ref_c.compute(left, right, dict(full, uniquenessRatio=0, disp12MaxDiff=1000000, speckleWindowSize=0))
        exp_r = ref_c.compute(right, left, sgm_np.right_matcher_params(full))
        wp = dict(lmbda=float(s["lmbda"]), sigma=s["sigma"], radius=-(-bs // 2), min_disp=minD,
                  left_offset=max(0, minD + D), right_offset=max(0, -minD))
    filt = wls_np.wls_filter(exp_l, left, exp_r, wp)
    for a in (exp_l, exp_r, filt):
        a.setflags(write=False)
    return exp_l, exp_r, filt, wp

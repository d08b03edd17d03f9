"""WLS post-filter oracle (oracle/wls_np.py): known-answer tests and a check
that the Thomas restatement solves the fast-global-smoother system.
Parity with ximgproc itself is unpinned (not in the image)."""
import numpy as np
import pytest

from oracle import wls_np
from stereo_match_amd import synthetic


def _laplacian_solve(f, C, lam):
    """Dense float64 solve of (I + lam*L_w) u = f along axis 1 (C = -w)."""
    h, w = f.shape
    out = np.empty((h, w))
    for i in range(h):
        A = np.eye(w)
        for j in range(w - 1):
            wt = -float(C[i, j])
            A[j, j] += lam * wt
            A[j + 1, j + 1] += lam * wt
            A[j, j + 1] -= lam * wt
            A[j + 1, j] -= lam * wt
        out[i] = np.linalg.solve(A, f[i].astype(np.float64))
    return out


def test_thomas_solves_fgs_system():
    rng = np.random.default_rng(0)
    g = rng.integers(0, 256, (6, 40))
    tab = wls_np.weight_table(2.0)
    C = np.zeros(g.shape, np.float32)
    C[:, :-1] = tab[np.abs(np.diff(g, axis=1))]
    f = rng.standard_normal(g.shape).astype(np.float32) * 100
    u = f.copy()
    wls_np._solve_rows([u], C, 50.0)
    ref = _laplacian_solve(f, C, 50.0)
    assert np.allclose(u, ref, rtol=1e-4, atol=1e-3)


def test_weight_table():
    t = wls_np.weight_table(1.2)
    assert t.dtype == np.float32 and t[0] == -1.0
    assert np.all(np.diff(t) >= 0) and np.all(np.diff(t[:80]) > 0) and t[-1] == 0


@pytest.mark.parametrize("conf", [True, False])
def test_constant_disparity_is_fixed_point(conf):
    H, W, D = 30, 80, 16
    displ = np.full((H, W), 5 * 16 + 3, np.int16)
    displ[:, :D] = -16
    dispr = np.full((H, W), -(5 * 16 + 3), np.int16)
    guide = synthetic.random_dot_pair(H, W, D, seed=1)[0]
    p = dict(lmbda=80000.0, sigma=1.2, radius=3, left_offset=D, use_confidence=conf)
    out = wls_np.wls_filter(displ, guide, dispr if conf else None, p)
    assert np.all(out[:, D:] == 5 * 16 + 3)
    assert np.all(out[:, :D] == -16)


def test_confidence_drops_at_discontinuities_and_lr_failures():
    H, W = 20, 60
    displ = np.full((H, W), 160, np.int16)
    displ[:, 40:] = 480  # depth step
    dispr = np.full((H, W), -160, np.int16)
    p = wls_np.normalize_wls(dict(radius=2, left_offset=16), H, W)
    conf = wls_np.confidence_map(displ, dispr, p)
    assert conf[5, 20] == 255.0  # flat and LR-consistent
    assert conf[5, 40] == 0.0  # variance of the step window >> 1/roll_off
    # where dl = 480 the right view says -160: LR check fails → 0
    assert np.all(conf[:, 43:] == 0.0)


def test_fills_holes_inside_roi():
    H, W, D = 24, 70, 16
    displ = np.full((H, W), 8 * 16, np.int16)
    displ[10:14, 30:36] = -16  # invalid hole
    dispr = np.full((H, W), -8 * 16, np.int16)
    guide = np.full((H, W), 100, np.uint8)
    out = wls_np.wls_filter(displ, guide, dispr, dict(lmbda=8000.0, sigma=1.0, radius=3, left_offset=D))
    assert np.all(np.abs(out[10:14, 30:36].astype(int) - 128) <= 2)


def test_empty_roi_is_fill_only():
    d = np.zeros((5, 20), np.int16)
    out = wls_np.wls_filter(d, np.zeros((5, 20), np.uint8), d, dict(left_offset=20, min_disp=-3))
    assert np.all(out == 16 * (-3 - 1))


def test_golden_wls_fixtures_reproduce(golden_wls_cases):
    for name, displ, dispr, guide, p, expected in golden_wls_cases:
        assert np.array_equal(wls_np.wls_filter(displ, guide, dispr, p), expected), name


# ---- the inputs of tests/test_gpu_wls.py must keep the filter alive (tests/wls_cases.py) ----------------
import wls_cases  # noqa: E402

_ALL_CASES = [(name, c) for name, lst in wls_cases.CASE_LISTS.items() for c in lst]


@pytest.mark.parametrize("name,c", _ALL_CASES, ids=[f"{n}-{c['id']}" for n, c in _ALL_CASES])
def test_gpu_case_inputs_are_live(name, c):
    """Conditions that keep a device parity test from passing on dead data, on the oracle alone.
    They are floors, not measurements: over the ROI at least half the outputs are non-zero, a fifth
    of the confidences are fractional (radius >= 1, roll_off 0.001), and ROIs of 1000 pixels or
    more have a tenth of their outputs moved by the filter and 50 distinct values.  A case whose
    point is a dead confidence, non-finite smoother stages or an empty ROI declares it and is
    checked for exactly that."""
    displ, dispr, guide = wls_cases.case_inputs(c)
    p = wls_np.normalize_wls(c["p"], c["H"], c["W"])
    r = wls_cases.liveness(displ, dispr, guide, c["p"])
    assert np.array_equal(r["out"], wls_cases.case_expected(c))
    if c["empty"]:
        assert r["pixels"] == 0 and np.all(r["out"] == 16 * (p["min_disp"] - 1))
        return
    assert r["pixels"] == p["roi"][2] * p["roi"][3] > 0
    assert r["nonfinite"] == c["nonfinite"]
    if c["dead"]:
        assert r["live_conf"] == 0.0 and r["nonzero"] == 0.0
        return
    if c["nonfinite"]:  # lambda 3e8: the float32 pivots cancel; den is inf / nan and the map 0
        assert r["frac_conf"] >= 0.2
        return
    assert r["nonzero"] >= 0.5
    if p["use_confidence"] and p["radius"] >= 1 and p["roll_off"] == 0.001:
        assert r["frac_conf"] >= 0.2
    if r["pixels"] >= 1000:
        assert r["changed"] >= 0.1 and r["distinct"] >= 50


def test_wide_cases_straddle_the_separable_limit():
    """k_wls_conf switches to per-pixel box sums where the column sums no longer fit 64 KiB of
    LDS; the wide cases sit at the limit and one past it for r = 0 and r = 3."""
    assert [wls_cases.separable_limit(r) for r in (0, 3, 5, 64)] == [3224, 3221, 3218, 3148]
    assert [wls_cases.wide_separable(c) for c in wls_cases.WIDE_CASES] == [True, False, True, False, False]
    for c in wls_cases.WIDE_CASES:
        assert c["p"]["left_offset"] == 20 and c["H"] in (3, 5)


def test_radius_clip_cases_see_the_reflection_rule(monkeypatch):
    """The final map of the radius cases with roll_off at the clip depends on the repeated
    reflection: with a single reflection (clamped to stay inside) the oracle's own map changes for
    every shape whose window reflects more than once.  1 x 40 with r = 5 never does (one row; 40
    columns take a single reflection), and at roll_off 0.001 the 5 x 2 map does not notice."""
    def single(i, n):
        if n == 1:
            return np.zeros_like(i)
        i = np.asarray(i)
        return np.clip(np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i)), 0, n - 1)

    def mutated(c):
        displ, dispr, guide = wls_cases.case_inputs(c)
        with monkeypatch.context() as m:
            m.setattr(wls_np, "_reflect101", single)
            return wls_np.wls_filter(displ, guide, dispr, c["p"])

    for c in wls_cases.RADIUS_CLIP_CASES:
        differs = not np.array_equal(mutated(c), wls_cases.case_expected(c))
        assert differs == (c["H"] > 1), c["id"]
    plain = next(c for c in wls_cases.RADIUS_CASES if c["id"] == "5x2r9")
    assert np.array_equal(mutated(plain), wls_cases.case_expected(plain))


@pytest.mark.parametrize("H,W", [(2, 20), (31, 97), (60, 200)])
def test_hypothesis_consistent_maps_are_live(H, W):
    """the corners of test_hypothesis_wls_vs_oracle's shape range, with its default-like parameters"""
    displ, dispr, guide = wls_cases.hypothesis_maps("consistent", H, W, 5)
    r = wls_cases.liveness(displ, dispr, guide, dict(lmbda=8000.0, sigma=1.2, radius=3))
    assert r["nonzero"] >= 0.5 and r["live_conf"] >= 0.5


def test_noise_maps_have_no_confidence():
    """The finding that gave test_wls_pivot_reciprocal_both_paths (and the radius and hypothesis
    tests) a second input kind: with displ, dispr and the guide drawn as independent uniform noise
    the windowed variance is far above 1/roll_off and |dl + dr[ri]| < lrc_thresh almost never
    holds, so conf > 0 at no ROI pixel, num = den = 0 going into the smoother, and the output is 0
    everywhere whatever reciprocal or reflection the device uses.  Those noise cases still guard
    the geometry; only the "consistent" maps put non-zero right-hand sides through the smoother."""
    H, W = 30, 160
    for lam in wls_cases.PIVOT_LAMBDAS:
        displ, dispr, guide = wls_cases.noise_maps(H, W, int(lam) % 1000 + 7)
        p = dict(lmbda=lam, sigma=1.2, lrc_thresh=24, radius=3, use_confidence=True, left_offset=20,
                 right_offset=0, top_offset=0, bottom_offset=0, num_iter=3, min_disp=0)
        with np.errstate(all="ignore"):
            out, st = wls_np.wls_filter(displ, guide, dispr, p, return_stages=True)
        assert not (st["conf"][:, 20:] > 0).any()
        assert not out[:, 20:].any()
    for Hr, Wr, r in wls_cases.RADIUS_SHAPES:
        displ, dispr, guide = wls_cases.noise_maps(Hr, Wr, Hr * 1000 + Wr + r)
        p = dict(lmbda=8000.0, sigma=1.5, lrc_thresh=24, radius=r, num_iter=2)
        out, st = wls_np.wls_filter(displ, guide, dispr, p, return_stages=True)
        assert not (st["conf"] > 0).any() and not out.any()


_CD_RUN = [e for e in wls_cases.CD_SETTINGS if "refused" not in e] + [wls_cases.CD_BM]


@pytest.mark.parametrize("e", _CD_RUN, ids=[e["id"] for e in _CD_RUN])
def test_compute_disparity_settings_chain_is_live(e):
    """the oracle chain of test_compute_disparity_other_settings: real matcher outputs keep the
    filter alive (the output floors of test_gpu_case_inputs_are_live; the fractional-confidence
    floor belongs to the constructed maps' variance and is not asked of matcher outputs)"""
    exp_l, exp_r, filt, wp = wls_cases.cd_chain(e["id"])
    left, _ = wls_cases.cd_pair()
    r = wls_cases.liveness(exp_l, exp_r, left, wp)
    assert np.array_equal(r["out"], filt)
    assert r["nonzero"] >= 0.5 and r["changed"] >= 0.1 and r["distinct"] >= 50 and not r["nonfinite"]


def test_compute_disparity_speckle_case_has_teeth():
    """speckle_window_size 50 changes the left matcher's map, so a library that forgot
    createDisparityWLSFilter's setSpeckleWindowSize(0) would be caught by the displ comparison"""
    from oracle import ref_c

    exp_l = wls_cases.cd_chain("speckle50")[0]
    left, right = wls_cases.cd_pair()
    lp = dict(minDisparity=0, numDisparities=wls_cases.CD_D, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1000000,
              uniquenessRatio=0, preFilterCap=63, speckleWindowSize=0, speckleRange=2, mode=5, cost=0)
    assert np.array_equal(ref_c.compute(left, right, lp), exp_l)
    assert not np.array_equal(ref_c.compute(left, right, dict(lp, speckleWindowSize=50)), exp_l)


def _border_interpolate_101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), scalar form."""
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def test_reflect101_windows_wider_than_image():
    # radius up to 64 over maps as short as 2 rows: reflections repeat (a single
    # reflection would index outside the map)
    for n in (1, 2, 3, 5, 17):
        idx = np.arange(-70, n + 70)
        got = wls_np._reflect101(idx, n)
        assert got.min() >= 0 and got.max() < n
        assert [int(v) for v in got] == [_border_interpolate_101(int(p), n) for p in idx]

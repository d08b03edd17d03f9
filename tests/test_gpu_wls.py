"""GPU parity of the WLS post-filter and of the whole compute_disparity
(left SGBM + right SGBM + WLS) against the CPU restatements.  Bar:
bit-exact int16 (the kernels run the oracle's float32 operation order with
FP contraction off).  Parity with ximgproc itself is unpinned.

Two kinds of synthetic maps (tests/wls_cases.py): "noise", independent uniform noise, whose
confidence is 0 everywhere, so it checks geometry only; and "consistent", whose confidence is
fractional and whose right-hand sides are non-zero (tests/test_wls_oracle.py holds every case
list used here to liveness floors on the oracle alone)."""
import re

import numpy as np
import pytest

import wls_cases
from oracle import ref_c, sgm_np, wls_np
from stereo_match_amd import _lib, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def wls_params(p: dict, H, W) -> _lib.SmWlsParams:
    q = wls_np.normalize_wls(p, H, W)
    return _lib.SmWlsParams(q["lmbda"], q["sigma"], q["lrc_thresh"], q["radius"], int(q["use_confidence"]),
                            q["min_disp"], q["left_offset"], q["right_offset"], q["top_offset"],
                            q["bottom_offset"], q["num_iter"], q["attenuation"], q["roll_off"])


def _check_case(eng, c):
    """one tests/wls_cases.py case on the device against the oracle's map"""
    displ, dispr, guide = wls_cases.case_inputs(c)
    out = eng.wls_filter(displ, guide, dispr if c["p"]["use_confidence"] else None, wls_params(c["p"], c["H"], c["W"]))
    exp = wls_cases.case_expected(c)
    assert np.array_equal(out, exp), f"{c['id']}: {np.sum(out != exp)} px differ"


def _case_ids(cases):
    return [c["id"] for c in cases]


def test_golden_wls_fixtures(eng, golden_wls_cases):
    for name, displ, dispr, guide, p, expected in golden_wls_cases:
        out = eng.wls_filter(displ, guide, dispr, wls_params(p, *displ.shape))
        assert np.array_equal(out, expected), f"{name}: {np.sum(out != expected)} px differ"


def _pair_maps(H, W, D, seed, ws=5, minD=0):
    left, right, gt = synthetic.random_dot_pair(H, W, D, seed=seed)
    settings = dict(synthetic.parity_params(D, window_size=ws), minDisparity=minD)
    lp = dict(settings, uniquenessRatio=0, disp12MaxDiff=1000000)
    displ = ref_c.compute(left, right, lp)
    dispr = ref_c.compute(right, left, sgm_np.right_matcher_params(settings))
    return left, right, gt, settings, displ, dispr


_rng = np.random.default_rng(77)
_CASES = [dict(H=int(_rng.integers(2, 80)), W=int(_rng.integers(40, 260)), D=16 * int(_rng.integers(1, 3)),
               minD=int(_rng.integers(-4, 4)), r=int(_rng.integers(0, 5)), lam=float(_rng.choice([10.0, 8000.0, 80000.0])),
               sigma=float(_rng.choice([0.7, 1.2, 3.0])), top=int(_rng.integers(0, 3)), seed=int(_rng.integers(0, 1 << 30)))
          for _ in range(10)]


@pytest.mark.parametrize("c", _CASES, ids=lambda c: "H{H}W{W}D{D}m{minD}r{r}".format(**c))
def test_wls_random_vs_oracle(eng, c):
    left, _, _, _, displ, dispr = _pair_maps(c["H"], c["W"], c["D"], c["seed"], minD=c["minD"])
    H, W = displ.shape
    p = dict(lmbda=c["lam"], sigma=c["sigma"], radius=c["r"], min_disp=c["minD"],
             left_offset=max(0, c["minD"] + c["D"]), right_offset=max(0, -c["minD"]),
             top_offset=min(c["top"], H - 1), bottom_offset=0)
    out = eng.wls_filter(displ, left, dispr, wls_params(p, H, W))
    assert np.array_equal(out, wls_np.wls_filter(displ, left, dispr, p))


def test_wls_no_confidence(eng):
    left, _, _, _, displ, _ = _pair_maps(50, 160, 32, 5)
    p = dict(lmbda=8000.0, sigma=1.5, use_confidence=False)
    out = eng.wls_filter(displ, left, None, wls_params(p, *displ.shape))
    assert np.array_equal(out, wls_np.wls_filter(displ, left, None, p))


def test_wls_full_size_kitti(eng):
    H, W, D = synthetic.CONFIGS["kitti"]
    left, _, gt, _, displ, dispr = _pair_maps(H, W, D, 42)
    p = dict(lmbda=80000.0, sigma=1.2, radius=3, left_offset=D)
    out = eng.wls_filter(displ, left, dispr, wls_params(p, H, W))
    exp = wls_np.wls_filter(displ, left, dispr, p)
    assert np.array_equal(out, exp), f"{np.sum(out != exp)} px differ"
    roi = out[:, D:]
    assert np.all(roi >= 0)
    assert np.mean(np.abs(((roi.astype(np.int64) + 8) >> 4) - gt[:, D:]) <= 1) > 0.97


def test_compute_disparity_end_to_end():
    """stereo_vision.compute_disparity drop-in: (displ, filtered) vs the
    oracle chain run in the reference's order."""
    import stereo_match_amd as sm

    H, W, D = 96, 300, 64
    left, right, _ = synthetic.random_dot_pair(H, W, D, seed=8)
    s = dict(sm.DEFAULT_SETTINGS, window_size=5, num_disparities=D, lmbda=80000, sigma=1.2)
    displ, filt = sm.compute_disparity(left, right, s)
    lp = dict(synthetic.parity_params(D), blockSize=s["block_size"], uniquenessRatio=0, disp12MaxDiff=1000000,
              minDisparity=s["min_disparity"], preFilterCap=s["pre_filter_cap"], speckleRange=s["speckle_range"])
    settings = dict(lp, uniquenessRatio=s["uniqueness_ratio"], disp12MaxDiff=s["disp12_max_diff"])
    exp_l = ref_c.compute(left, right, lp)
    exp_r = ref_c.compute(right, left, sgm_np.right_matcher_params(settings))
    assert np.array_equal(displ, exp_l)
    wp = dict(lmbda=80000.0, sigma=1.2, radius=-(-s["block_size"] // 2), min_disp=s["min_disparity"],
              left_offset=max(0, s["min_disparity"] + D), right_offset=max(0, -s["min_disparity"]))
    assert np.array_equal(filt, wls_np.wls_filter(exp_l, left, exp_r, wp))
    # the one-call C-ABI flow gives the same maps
    eng = _lib.engine(0)
    sp = synthetic.to_sm_params(settings)
    d2, f2 = eng.compute_disparity(left, right, sp, wls_params(dict(wp), H, W))
    assert np.array_equal(d2, displ) and np.array_equal(f2, filt)
    dw = _lib.wls_default_params(sp)
    assert (dw.left_offset, dw.right_offset, dw.depth_discontinuity_radius, dw.min_disp) == (D, 0, 3, 0)


def test_compute_disparity_batch_device_and_torch():
    import torch

    import stereo_match_amd as sm
    from stereo_match_amd import wls

    H, W, D, n = 64, 220, 32, 3
    pairs = [synthetic.random_dot_pair(H, W, D, seed=50 + i)[:2] for i in range(n)]
    L = torch.tensor(np.stack([a for a, _ in pairs]), device="cuda")
    R = torch.tensor(np.stack([b for _, b in pairs]), device="cuda")
    settings = synthetic.parity_params(D)
    sp = synthetic.to_sm_params(settings)
    wp = _lib.wls_default_params(sp)
    wp.lambda_, wp.sigma_color = 80000.0, 1.2
    outs = [torch.empty((n, H, W), dtype=torch.int16, device="cuda") for _ in range(3)]
    eng = _lib.engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.compute_disparity_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W, sp, wp,
                                       *(o.data_ptr() for o in outs))
    got = [o.cpu().numpy() for o in outs]
    for i, (a, b) in enumerate(pairs):
        d2, f2 = eng.compute_disparity(a, b, sp, wp)
        assert np.array_equal(got[0][i], d2) and np.array_equal(got[2][i], f2), i
    # torch tensors through the Python filter object
    m = sm.StereoSGBM_create(numDisparities=D, blockSize=5, P1=600, P2=2400, disp12MaxDiff=1, uniquenessRatio=15,
                             preFilterCap=63)
    f = wls.createDisparityWLSFilter(m)
    f.setLambda(80000.0)
    f.setSigmaColor(1.2)
    t = f.filter(outs[0][0], L[0], None, outs[1][0])
    assert np.array_equal(t.cpu().numpy(), got[2][0])


def test_wls_bad_args(eng):
    d = np.zeros((10, 40), np.int16)
    g = np.zeros((10, 40), np.uint8)
    with pytest.raises(ValueError):
        eng.wls_filter(d, g, None, wls_params(dict(), 10, 40))  # confidence needs dispr
    with pytest.raises(ValueError):
        eng.wls_filter(d, g, d, wls_params(dict(left_offset=-1), 10, 40))


# the noise cases keep their earlier ids; the consistent ones stand beside them
@pytest.mark.parametrize("H,W,r,maps", [pytest.param(H, W, r, m, id=("" if m == "noise" else m + "-") + f"{H}-{W}-{r}")
                                        for m in ("noise", "consistent") for H, W, r in wls_cases.RADIUS_SHAPES])
def test_wls_radius_wider_than_map(eng, H, W, r, maps):
    """The confidence window reflects more than once (cv::borderInterpolate REFLECT_101).  On the
    noise maps the confidence is 0 whatever reflect101 returns; the consistent maps reach
    conf_row / reflect101 of k_wls_conf with a confidence that depends on every window value."""
    if maps == "consistent":
        return _check_case(eng, next(c for c in wls_cases.RADIUS_CASES if c["id"] == f"{H}x{W}r{r}"))
    displ, dispr, guide = wls_cases.noise_maps(H, W, H * 1000 + W + r)
    p = dict(lmbda=8000.0, sigma=1.5, lrc_thresh=24, radius=r, use_confidence=True, left_offset=0,
             right_offset=0, top_offset=0, bottom_offset=0, num_iter=2, min_disp=0)
    out = eng.wls_filter(displ, guide, dispr, wls_params(p, H, W))
    assert np.array_equal(out, wls_np.wls_filter(displ, guide, dispr, p))


@pytest.mark.parametrize("c", wls_cases.RADIUS_CLIP_CASES, ids=_case_ids(wls_cases.RADIUS_CLIP_CASES))
def test_wls_radius_wider_than_map_at_confidence_clip(eng, c):
    """The same shapes with roll_off where 1 - roll_off * var crosses 0 for these maps' windows, so
    that pixels clip or live by the exact window sum and the final map shows which samples
    reflect101 returned (tests/test_wls_oracle.py: a single reflection changes the oracle's map for
    every shape that reflects more than once, which roll_off 0.001 does not show on the 5 x 2 map)."""
    _check_case(eng, c)


@pytest.mark.parametrize("c", wls_cases.ROLL_OFF_CASES, ids=_case_ids(wls_cases.ROLL_OFF_CASES))
def test_wls_roll_off(eng, c):
    """roll_off away from 0.001 (k_wls_conf's max(1 - roll_off * var, 0)): 0 gives full confidence
    wherever the LR check passes, 0.02 clips most windows to 0, 10 kills the confidence."""
    _check_case(eng, c)


@pytest.mark.parametrize("lam,maps", [pytest.param(lam, m, id=("" if m == "noise" else m + "-") + str(lam))
                                      for m in ("noise", "consistent") for lam in wls_cases.PIVOT_LAMBDAS])
def test_wls_pivot_reciprocal_both_paths(eng, lam, maps):
    """pivots <= 1 + 2*lambda: below 2^24 the smoother uses rcp + one FMA step (exact there,
    tools/ubench/rcp_exact.hip), above it IEEE division; both must equal the oracle.  The noise
    maps give num = den = 0 (any reciprocal passes); the consistent maps put non-zero right-hand
    sides through k_fgs_pivots<*, true> (lambda <= 2e6), k_fgs_pivots<*, false> (1e7, 3e8) and
    k_fgs_solve16.  At lambda 3e8 the float32 pivots cancel: num / den are inf / nan in both."""
    if maps == "consistent":
        return _check_case(eng, next(c for c in wls_cases.PIVOT_CASES if c["id"] == f"lam{lam:g}"))
    H, W = 30, 160
    displ, dispr, guide = wls_cases.noise_maps(H, W, int(lam) % 1000 + 7)
    p = dict(lmbda=lam, sigma=1.2, lrc_thresh=24, radius=3, use_confidence=True, left_offset=20,
             right_offset=0, top_offset=0, bottom_offset=0, num_iter=3, min_disp=0)
    out = eng.wls_filter(displ, guide, dispr, wls_params(p, H, W))
    with np.errstate(all="ignore"):  # lambda 3e8: float32 pivots cancel to 0 (inf/nan) in both
        ref = wls_np.wls_filter(displ, guide, dispr, p)
    assert np.array_equal(out, ref)


_ATT_CASES = wls_cases.PIVOT_CASES[len(wls_cases.PIVOT_LAMBDAS):]


@pytest.mark.parametrize("c", _ATT_CASES, ids=_case_ids(_ATT_CASES))
def test_wls_pivot_attenuation(eng, c):
    """lambda_attenuation away from 0.25.  wls_fast() decides rcp or IEEE division once for all
    iterations from lambda * att^it: with lambda 3e6 and attenuation 2 the first pass alone would
    be fast, the third (1.2e7) is not, so wls_fast returns false because of a later iteration and
    every pass runs k_fgs_pivots<*, false>.  Attenuation 1 keeps lambda, 0 leaves lambda 0 after
    the first pass; num_iter 8 is the last count the pivot buffers hold.  These cases pin the maps,
    not the choice: rcp + one FMA step depends on the pivot's mantissa alone, and a build that
    decided from the first iteration only gave the same maps here."""
    _check_case(eng, c)


@pytest.mark.parametrize("c", wls_cases.KFGS_CASES, ids=_case_ids(wls_cases.KFGS_CASES))
def test_wls_num_iter_beyond_pivot_buffers(eng, c):
    """num_iter > 8 takes run_wls's else branch: k_fgs<NRHS, ROWS, FAST> with the pivots inside
    each pass and the wls_inter buffer, which nothing else launches.  NRHS 2 / 1 (confidence on /
    off), rows and columns, FAST (lambda 8000, 500) and IEEE (1e7; 4e4 doubling to 1.024e7, where
    wls_fast is false because of a later iteration).  The 70 x 130 and 40 x 180 ROIs are no
    multiple of the 64-tile and span several chunks both ways; num_iter 8 pins the last
    pivot-path count beside them."""
    _check_case(eng, c)


@pytest.mark.parametrize("c", wls_cases.WIDE_CASES, ids=_case_ids(wls_cases.WIDE_CASES))
def test_wls_roi_wider_than_separable_limit(eng, c):
    """ROI widths at and one past the largest that k_wls_conf's LDS column sums hold (3224 for
    r = 0, 3221 for r = 3; the launch at the limit asks for 65520 / 65532 of the 65536 bytes), and
    3300: past the limit the per-pixel branch (discontinuity_conf, ca.separable = 0) runs, which no
    narrower map reaches.  left_offset 20 makes rx0 (0) differ from x0."""
    _check_case(eng, c)


@pytest.mark.parametrize("c", wls_cases.DEGENERATE_CASES, ids=_case_ids(wls_cases.DEGENERATE_CASES))
def test_wls_degenerate_roi(eng, c):
    """Offsets that leave no ROI (width 0, width -3, height 0) take the !roi branch of run_wls:
    only k_wls_final runs and fills 16 * (min_disp - 1).  ROIs of one column, one row and one
    pixel, and maps of one row or one column, run every kernel on a single padded tile."""
    _check_case(eng, c)
    if c["empty"]:
        assert np.all(wls_cases.case_expected(c) == 16 * (c["p"]["min_disp"] - 1))


from hypothesis import HealthCheck, given, settings, strategies as st  # noqa: E402


@settings(max_examples=25, deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(H=st.integers(2, 60), W=st.integers(20, 200), lo=st.integers(0, 40), ro=st.integers(0, 10),
       to=st.integers(0, 5), bo=st.integers(0, 5), r=st.integers(0, 6), lam=st.floats(0.0, 1e5),
       sigma=st.floats(0.3, 5.0), lrc=st.integers(0, 64), conf=st.booleans(), it=st.integers(1, 10),
       seed=st.integers(0, 2**31 - 1), kind=st.sampled_from(["noise", "consistent"]),
       att=st.sampled_from([0.25, 0.0, 1.0, 2.0]), roll=st.sampled_from([0.001, 0.0, 0.02]))
def test_hypothesis_wls_vs_oracle(eng, H, W, lo, ro, to, bo, r, lam, sigma, lrc, conf, it, seed, kind, att, roll):
    """Random geometry and parameters over both map kinds; num_iter up to 10 crosses from the
    pivot kernels to k_fgs, and the attenuation and roll_off leave their defaults."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        displ = rng.integers(-16, 40 * 16, (H, W)).astype(np.int16)
        dispr = (-rng.integers(0, 40 * 16, (H, W))).astype(np.int16)
        guide = rng.integers(0, 256, (H, W)).astype(np.uint8)
    else:
        displ, dispr, guide = wls_cases.hypothesis_maps(kind, H, W, seed)
    p = dict(lmbda=float(np.float32(lam)), sigma=float(np.float32(sigma)), lrc_thresh=lrc, radius=r,
             use_confidence=conf, left_offset=lo, right_offset=ro, top_offset=to, bottom_offset=bo, num_iter=it,
             min_disp=int(rng.integers(-3, 3)), attenuation=att, roll_off=roll)
    out = eng.wls_filter(displ, guide, dispr if conf else None, wls_params(p, H, W))
    with np.errstate(all="ignore"):  # attenuation 2 can take lambda to where float32 pivots cancel
        ref = wls_np.wls_filter(displ, guide, dispr if conf else None, p)
    assert np.array_equal(out, ref)


def test_compute_disparity_repeatable_with_side_stream_prepare():
    """The WLS guide-only work (weights, pivots) runs on its own stream beside the two
    matchers; every call must give the filter-alone result.  This caught a store-data
    hazard (sm_wls.hpp tile_store) that only showed with kernels running side by side."""
    import torch

    import stereo_match_amd as sm
    from stereo_match_amd import wls
    from stereo_match_amd.stereo_vision import matcher_from_settings

    for D in (64, 128):
        s = dict(sm.DEFAULT_SETTINGS, window_size=5, num_disparities=D)
        H, W = 120, 420
        gl, gr, _ = synthetic.random_dot_pair(H, W, D, seed=D + 3)
        lm = matcher_from_settings(s)
        prm = lm.params()
        wf = wls.createDisparityWLSFilter(lm)
        wf.setLambda(s["lmbda"])
        wf.setSigmaColor(s["sigma"])
        wp = wf.params(H, W)
        eng = _lib.Engine(0)
        try:
            L = torch.tensor(gl, device="cuda")
            R = torch.tensor(gr, device="cuda")
            dl = torch.empty((H, W), dtype=torch.int16, device="cuda")
            dr = torch.empty_like(dl)
            fo = torch.empty_like(dl)
            first = None
            for i in range(12):
                eng.compute_disparity_batch_device(L.data_ptr(), R.data_ptr(), 1, H * W, H, W, W, prm, wp,
                                                   dl.data_ptr(), dr.data_ptr(), fo.data_ptr())
                eng.synchronize()
                if first is None:
                    first = (dl.cpu().numpy(), dr.cpu().numpy())
                    alone = eng.wls_filter(first[0], gl, first[1], wp)
                assert np.array_equal(fo.cpu().numpy(), alone), (D, i)
        finally:
            eng.close()


def test_compute_disparity_on_caller_stream():
    """After sm_set_stream the right matcher (twin context, own stream) and the WLS
    guide work (third stream) still fork from and join into the caller's stream:
    the maps written there equal the default-stream call's, read right after a
    synchronize of that stream only (twin ordering after sm_set_stream)."""
    import torch

    H, W, D, n = 80, 260, 32, 2
    pairs = [synthetic.random_dot_pair(H, W, D, seed=70 + i)[:2] for i in range(n)]
    sp = synthetic.to_sm_params(synthetic.parity_params(D))
    wp = _lib.wls_default_params(sp)
    wp.lambda_, wp.sigma_color = 8000.0, 1.5
    eng = _lib.Engine(0)
    try:
        L = torch.tensor(np.stack([a for a, _ in pairs]), device="cuda")
        R = torch.tensor(np.stack([b for _, b in pairs]), device="cuda")
        outs = []
        for use_stream in (False, True):
            dl, dr, fo = (torch.full((n, H, W), 99, dtype=torch.int16, device="cuda") for _ in range(3))
            s = torch.cuda.Stream()
            torch.cuda.synchronize()  # the inputs and the 99-filled outputs are in place
            if use_stream:
                eng.set_stream(s.cuda_stream)
            try:
                eng.compute_disparity_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W, sp, wp,
                                                   dl.data_ptr(), dr.data_ptr(), fo.data_ptr())
                if use_stream:
                    s.synchronize()
                else:
                    eng.synchronize()
                outs.append([t.cpu().numpy() for t in (dl, dr, fo)])
            finally:
                eng.set_stream(None)
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
    finally:
        eng.close()


@pytest.mark.gpu
def test_compute_disparity_batch_device_npairs_guard():
    """npairs < 0 -> SM_E_ARG before any launch is sized from it; npairs == 0 is a no-op
    that leaves the outputs untouched (the WLS preparation used to launch first)."""
    import torch

    H, W, D = 40, 120, 16
    sp = synthetic.to_sm_params(synthetic.parity_params(D))
    wp = _lib.wls_default_params(sp)
    L = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    outs = [torch.full((1, H, W), 7, dtype=torch.int16, device="cuda") for _ in range(3)]
    eng = _lib.engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        with pytest.raises(ValueError):
            eng.compute_disparity_batch_device(L.data_ptr(), L.data_ptr(), -1, H * W, H, W, W, sp, wp,
                                               *(o.data_ptr() for o in outs))
        eng.compute_disparity_batch_device(L.data_ptr(), L.data_ptr(), 0, H * W, H, W, W, sp, wp,
                                           *(o.data_ptr() for o in outs))
        eng.synchronize()
        assert all(bool((o == 7).all()) for o in outs)
    finally:
        eng.set_stream(None)


def test_compute_disparity_num_iter_beyond_pivot_buffers():
    """compute_disparity with num_iter 9: the guide-only preparation still runs on the WLS side
    stream, but only the edge weights (wls_prepare returns before the pivots), and run_wls takes
    `prepared && !pivots`: k_wls_conf with ca.weights = 0 over the side stream's Ch / Cv, then the
    smoother passes from k_fgs.  Twice on one engine (buffers reused), against the filter alone on
    the same device maps and against the oracle chain."""
    import stereo_match_amd as sm
    from stereo_match_amd import wls
    from stereo_match_amd.stereo_vision import matcher_from_settings

    H, W, D = 64, 220, 32
    gl, gr, _ = synthetic.random_dot_pair(H, W, D, seed=31)
    s = dict(sm.DEFAULT_SETTINGS, window_size=5, num_disparities=D)
    lm = matcher_from_settings(s)
    prm = lm.params()
    wf = wls.createDisparityWLSFilter(lm)
    wf.setLambda(s["lmbda"])
    wf.setSigmaColor(s["sigma"])
    wp = wf.params(H, W)
    wp.num_iter = 9
    e = _lib.Engine(0)
    try:
        c0 = e.counters()["sweep_fallbacks"]
        d, f = e.compute_disparity(gl, gr, prm, wp)
        d2, f2 = e.compute_disparity(gl, gr, prm, wp)
        dr = e.compute(gr, gl, _lib.right_matcher_params(prm))
        alone = e.wls_filter(d, gl, dr, wp)
        assert e.counters()["sweep_fallbacks"] == c0
    finally:
        e.close()
    assert np.array_equal(d, d2) and np.array_equal(f, f2)
    assert np.array_equal(f, alone)
    hp = synthetic.parity_params(D, 5)
    exp_l = ref_c.compute(gl, gr, dict(hp, uniquenessRatio=0, disp12MaxDiff=1000000))
    exp_r = ref_c.compute(gr, gl, sgm_np.right_matcher_params(hp))
    assert np.array_equal(d, exp_l) and np.array_equal(dr, exp_r)
    wpar = dict(lmbda=80000.0, sigma=1.2, radius=3, min_disp=0, left_offset=D, right_offset=0, num_iter=9)
    assert np.array_equal(f, wls_np.wls_filter(exp_l, gl, exp_r, wpar))


def _cd_device_params(s, H, W):
    """(matcher params before the WLS filter's mutation, WLS params) as compute_disparity builds them"""
    from stereo_match_amd import wls
    from stereo_match_amd.stereo_vision import matcher_from_settings

    lm = matcher_from_settings(s)
    prm = lm.params()
    wf = wls.createDisparityWLSFilter(lm)
    wf.setLambda(s["lmbda"])
    wf.setSigmaColor(s["sigma"])
    return prm, wf.params(H, W)


@pytest.mark.parametrize("entry", wls_cases.CD_SETTINGS, ids=_case_ids(wls_cases.CD_SETTINGS))
def test_compute_disparity_other_settings(entry):
    """compute_disparity with one settings key away from dict(DEFAULT_SETTINGS, window_size=5), through
    the one-call ABI (sm.compute_disparity) and compute_disparity_batch_device with two pairs, against
    the oracle chain of tests/wls_cases.py cd_chain (offsets and radius derived there from the
    settings).  Reaches the right matcher's minDisparity = -(minD + D) + 1 and the WLS offsets
    max(0, minD + D) / max(0, -minD) for minD != 0, the radius ceil(0.5 * blockSize) for block sizes
    3 and 9, createDisparityWLSFilter dropping a non-zero speckle window, and 8 paths / the census
    cost through the twin context, the stagger stream and the WLS side stream.  The census cost
    with window_size 5's P2 = 2400 is refused (its 8-bit path values need P2 <= 193): the refusal and
    its message are asserted; window_size 1 runs the same mode.  No call may move sweep_fallbacks."""
    import torch

    import stereo_match_amd as sm

    s = wls_cases.cd_settings(entry)
    H, W, n = wls_cases.CD_H, wls_cases.CD_W, 2
    pairs = [wls_cases.cd_pair(i) for i in range(n)]
    eng = _lib.engine(0)
    eng.set_stream(None)
    c0 = eng.counters()["sweep_fallbacks"]
    prm, wp = _cd_device_params(s, H, W)
    L = torch.tensor(np.stack([a for a, _ in pairs]), device="cuda")
    R = torch.tensor(np.stack([b for _, b in pairs]), device="cuda")
    outs = [torch.full((n, H, W), 99, dtype=torch.int16, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()

    def batch():
        eng.compute_disparity_batch_device(L.data_ptr(), R.data_ptr(), n, H * W, H, W, W, prm, wp,
                                           *(o.data_ptr() for o in outs))
        eng.synchronize()

    if "refused" in entry:
        for call in (lambda: sm.compute_disparity(*pairs[0], s), batch):
            with pytest.raises(_lib.SmError, match=re.escape(entry["refused"])) as ei:
                call()
            assert ei.value.code == _lib.SM_E_UNSUPPORTED
        assert eng.counters()["sweep_fallbacks"] == c0
        return
    exp_l, exp_r, exp_f, _ = wls_cases.cd_chain(entry["id"])
    displ, filt = sm.compute_disparity(*pairs[0], s)
    assert np.array_equal(displ, exp_l), f"displ: {np.sum(displ != exp_l)} px differ"
    assert np.array_equal(filt, exp_f), f"filtered: {np.sum(filt != exp_f)} px differ"
    assert eng.counters()["sweep_fallbacks"] == c0
    batch()
    got = [o.cpu().numpy() for o in outs]
    for i in range(n):
        for name, g, x in zip(("displ", "dispr", "filtered"), got, wls_cases.cd_chain(entry["id"], i)):
            assert np.array_equal(g[i], x), f"pair {i} {name}: {np.sum(g[i] != x)} px differ"
    assert eng.counters()["sweep_fallbacks"] == c0


def test_compute_disparity_bm_other_settings():
    """method="BM" with block_size 9 and 48 disparities (the three-call path): BM offsets
    max(0, minD + D) + bs/2 and bs/2 on the other sides, radius ceil(0.33 * blockSize)."""
    import stereo_match_amd as sm

    entry = wls_cases.CD_BM
    eng = _lib.engine(0)
    eng.set_stream(None)
    c0 = eng.counters()["sweep_fallbacks"]
    exp_l, _, exp_f, _ = wls_cases.cd_chain(entry["id"])
    displ, filt = sm.compute_disparity(*wls_cases.cd_pair(), wls_cases.cd_settings(entry), method="BM")
    assert np.array_equal(displ, exp_l), f"displ: {np.sum(displ != exp_l)} px differ"
    assert np.array_equal(filt, exp_f), f"filtered: {np.sum(filt != exp_f)} px differ"
    assert eng.counters()["sweep_fallbacks"] == c0
